"""16-bit input: TIFF stacks and arrays of unsigned 16-bit pixels, mapped to the 8 bits everything downstream works in
(include/hydra_mi.h, "16-bit input").

``TiffStack`` maps a TIFF or BigTIFF stack and hands out its pages without reading the file whole.  ``histogram``,
``window``, ``make_lut`` and ``map_video`` are the four steps from a recording to its 8-bit frames: the histogram of every
pixel, one window [lo, hi] for the whole recording from two shares in parts per million, the table the window (and a
gamma) gives, and the frames through the table with what the window clipped, frame by frame.  With ``device=None`` each
runs in NumPy and gives the same bytes: that is the path a machine without a GPU takes.  ``DeepSource`` feeds the
pipeline's frame ring with the 16-bit pixels, 2 bytes a pixel over the bus, and the device writes the ring's three planes.
``load_deep`` is what ``sources.load_video`` and the command-line tools call; ``depth_option`` turns the tools' flags
into the ``depth`` they pass.
"""
import ctypes
import math
import os
import re
import struct

import numpy as np

from . import _lib
from .devbuf import DeviceBuffer

VALUES = 65536
#: the window's shares, parts per million: policy, not measurements
DEFAULT_LO_PPM = 1000
DEFAULT_HI_PPM = 999990
MILLION = 10 ** 6

# ---- TIFF ------------------------------------------------------------------------------------------------------------
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8, 17: 8, 18: 8}
_TYPE_CODE = {1: "B", 3: "H", 4: "I", 16: "Q"}                    # the unsigned integer types, which is all that is read
_T_WIDTH, _T_HEIGHT, _T_BITS, _T_COMPRESSION, _T_PHOTOMETRIC, _T_DESCRIPTION = 256, 257, 258, 259, 262, 270
_T_STRIP_OFFSETS, _T_SAMPLES, _T_ROWS_PER_STRIP, _T_STRIP_COUNTS, _T_TILE_WIDTH, _T_FORMAT = 273, 277, 278, 279, 322, 339


class _Fallback(Exception):
    """the file is a TIFF this reader leaves to PIL (compressed, tiled, ...)"""


class TiffStack:
    """A stack of gray pages in a TIFF file, mapped and not read whole: ``len``, ``.shape`` (H, W), ``.bits`` (8 or 16),
    ``.swap`` (1 when the file's 16-bit samples are big-endian) and ``page(f)``, a view of page f in the file's own byte
    order (dtype uint8, '<u2' or '>u2'; it compares equal to what PIL reads) without a copy.

    Accepted: classic TIFF and BigTIFF in either byte order ('II', 'MM'); one sample per pixel, 8 or 16 bits unsigned,
    uncompressed, in any number of strips (a page whose strips do not follow one another in the file is put together in
    a copy); all pages one size; and the ImageJ convention for stacks past 4 GiB: one IFD, ``images=N`` in its
    description, the pages one behind the other from the first strip on.  A compressed or tiled file, or one with
    min-is-white samples, is read by PIL page by page and gives the same arrays.  A malformed or truncated file raises
    ValueError with the offset at which it went wrong, and nothing else."""

    def __init__(self, path):
        import mmap
        self.path = str(path)
        self._f = open(self.path, "rb")
        self._map = self._view = None
        self._pil = None
        self.pages = []                                           # per page: (offset, None) or (None, [(offset, bytes), ...])
        try:
            try:
                self._map = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
            except ValueError:
                raise ValueError("%s: not a TIFF file: empty at offset 0" % self.path)
            self._view = memoryview(self._map)
            try:
                self._parse()
            except _Fallback:
                self._open_pil()
            except (struct.error, IndexError, OverflowError, MemoryError) as exc:
                raise ValueError("%s: malformed TIFF at offset %d: %s" % (self.path, getattr(self, "_at", 0), exc))
        except Exception:
            self.close()
            raise

    # -- the mapped reader
    def _need(self, off, n, what):
        if off < 0 or n < 0 or off + n > len(self._map):
            raise ValueError("%s: %s at offset %d needs %d bytes, the file has %d" % (self.path, what, off, n, len(self._map)))

    def _unpack(self, fmt, off, what):
        self._at = off
        self._need(off, struct.calcsize(self._bo + fmt), what)
        return struct.unpack_from(self._bo + fmt, self._map, off)

    def _ifd(self, off):
        """-> ({tag: values}, offset of the next IFD)"""
        big = self._big
        (count,) = self._unpack("Q" if big else "H", off, "an IFD")
        esize, head = (20, 8) if big else (12, 2)
        self._need(off + head, count * esize + (8 if big else 4), "the %d entries of the IFD" % count)
        tags = {}
        for i in range(count):
            e = off + head + i * esize
            tag, typ, n = self._unpack("HHQ" if big else "HHI", e, "an IFD entry")
            if tag not in (_T_WIDTH, _T_HEIGHT, _T_BITS, _T_COMPRESSION, _T_PHOTOMETRIC, _T_DESCRIPTION, _T_STRIP_OFFSETS, _T_SAMPLES,
                           _T_ROWS_PER_STRIP, _T_STRIP_COUNTS, _T_TILE_WIDTH, _T_FORMAT):
                continue
            size = _TYPE_SIZE.get(typ)
            if size is None:
                raise ValueError("%s: tag %d at offset %d has the unknown type %d" % (self.path, tag, e, typ))
            room = 8 if big else 4
            at = e + (12 if big else 8)
            if n * size > room:
                (at,) = self._unpack("Q" if big else "I", at, "a value offset")
            self._need(at, n * size, "the %d values of tag %d" % (n, tag))
            if typ == 2:
                tags[tag] = bytes(self._map[at:at + n])
            elif typ in _TYPE_CODE:
                self._at = at
                tags[tag] = np.frombuffer(self._map, np.dtype(self._bo + _TYPE_CODE[typ] if size > 1 else "B"), n, at).astype(np.uint64)
            else:
                raise ValueError("%s: tag %d at offset %d has type %d, not an unsigned integer" % (self.path, tag, e, typ))
        (nxt,) = self._unpack("Q" if big else "I", off + head + count * esize, "the next IFD's offset")
        return tags, nxt

    def _parse(self):
        self._bo, self._at = "<", 0
        self._need(0, 8, "the header")
        order = bytes(self._map[:2])
        if order not in (b"II", b"MM"):
            raise ValueError("%s: not a TIFF file: byte order mark %r at offset 0" % (self.path, order))
        self._bo = "<" if order == b"II" else ">"
        (magic,) = self._unpack("H", 2, "the header")
        if magic == 42:
            self._big = False
            (off,) = self._unpack("I", 4, "the header")
        elif magic == 43:
            self._big = True
            osize, zero, off = self._unpack("HHQ", 4, "the BigTIFF header")
            if osize != 8 or zero != 0:
                raise ValueError("%s: BigTIFF with offsets of %d bytes at offset 4" % (self.path, osize))
        else:
            raise ValueError("%s: not a TIFF file: magic %d at offset 2" % (self.path, magic))
        seen = set()
        first = None
        while off:
            if off in seen:
                raise ValueError("%s: the IFD at offset %d is reached twice" % (self.path, off))
            seen.add(off)
            tags, nxt = self._ifd(off)
            page = self._page_of(tags, off)
            if first is None:
                first = page
                self.shape, self.bits = (page[1], page[0]), page[2]
            elif page[:3] != first[:3]:
                raise ValueError("%s: the page of the IFD at offset %d is %dx%d of %d bits, the first %dx%d of %d"
                                 % ((self.path, off) + page[:3] + first[:3]))
            self.pages.append(page[3])
            off = nxt
        if first is None:
            raise ValueError("%s: no IFD (first IFD offset 0 at offset 4)" % self.path)
        self.swap = 1 if (self.bits == 16 and self._bo == ">") else 0
        self._dtype = np.dtype(np.uint8) if self.bits == 8 else np.dtype(self._bo + "u2")
        m = re.search(rb"images=(\d+)", first[4] or b"")
        if len(self.pages) == 1 and m and int(m.group(1)) > 1:     # ImageJ: the pages follow the first
            n = int(m.group(1))
            start, parts = self.pages[0]
            if start is None:
                raise ValueError("%s: an ImageJ stack of %d pages whose first page at offset %d is not one block"
                                 % (self.path, n, parts[0][0]))
            size = self.shape[0] * self.shape[1] * self.bits // 8
            self._need(start, n * size, "the %d pages of the ImageJ stack" % n)
            self.pages = [(start + i * size, None) for i in range(n)]

    def _page_of(self, tags, off):
        def one(tag, default=None):
            v = tags.get(tag)
            if v is None or isinstance(v, bytes) or len(v) < 1:
                if default is None:
                    raise ValueError("%s: the IFD at offset %d lacks tag %d" % (self.path, off, tag))
                return default
            return int(v[0])
        W, H = one(_T_WIDTH), one(_T_HEIGHT)
        if W < 1 or H < 1:
            raise ValueError("%s: a page of %dx%d in the IFD at offset %d" % (self.path, W, H, off))
        bits, samples, fmt = one(_T_BITS, 1), one(_T_SAMPLES, 1), one(_T_FORMAT, 1)
        if _T_TILE_WIDTH in tags or one(_T_COMPRESSION, 1) != 1 or one(_T_PHOTOMETRIC, 1) != 1:
            raise _Fallback()
        if samples != 1 or bits not in (8, 16) or fmt != 1:
            raise ValueError("%s: the IFD at offset %d holds %d samples of %d bits in format %d per pixel: expected one "
                             "unsigned sample of 8 or 16 bits" % (self.path, off, samples, bits, fmt))
        offs, counts = tags.get(_T_STRIP_OFFSETS), tags.get(_T_STRIP_COUNTS)
        if offs is None or isinstance(offs, bytes) or len(offs) < 1:
            raise ValueError("%s: the IFD at offset %d lacks tag %d" % (self.path, off, _T_STRIP_OFFSETS))
        rows = min(one(_T_ROWS_PER_STRIP, H), H)
        if rows < 1 or len(offs) != (H + rows - 1) // rows:
            raise ValueError("%s: the IFD at offset %d has %d strips of %d rows for %d rows" % (self.path, off, len(offs), rows, H))
        row = W * bits // 8
        parts = []
        for i, o in enumerate(offs):
            n = row * min(rows, H - i * rows)
            if counts is not None and not isinstance(counts, bytes) and i < len(counts) and int(counts[i]) < n:
                raise ValueError("%s: strip %d at offset %d has %d bytes, its rows need %d" % (self.path, i, int(o), int(counts[i]), n))
            self._need(int(o), n, "strip %d of the IFD at offset %d" % (i, off))
            parts.append((int(o), n))
        dense = all(parts[i][0] + parts[i][1] == parts[i + 1][0] for i in range(len(parts) - 1))
        desc = tags.get(_T_DESCRIPTION)
        return W, H, bits, ((parts[0][0], None) if dense else (None, parts)), desc if isinstance(desc, bytes) else None

    # -- the pages PIL reads
    def _open_pil(self):
        try:
            from PIL import Image
            self._pil = Image.open(self.path)
            n = getattr(self._pil, "n_frames", 1)
            first = self._pil_page(0)
        except ValueError:
            raise
        except Exception as exc:                                  # noqa: BLE001 -- whatever PIL makes of a broken file
            raise ValueError("%s: malformed TIFF at offset 0: %s" % (self.path, exc))
        self.pages = [None] * n
        self.shape, self.bits, self.swap = first.shape, 8 * first.dtype.itemsize, 0
        self._dtype = first.dtype

    def _pil_page(self, f):
        try:
            self._pil.seek(f)
            mode = self._pil.mode
            if mode not in ("L", "I;16", "I;16L", "I;16B"):
                raise ValueError("%s: expected 8- or 16-bit gray pages, found mode %s at offset 0" % (self.path, mode))
            a = np.asarray(self._pil)
        except ValueError:
            raise
        except Exception as exc:                                  # noqa: BLE001
            raise ValueError("%s: malformed TIFF at offset 0: page %d: %s" % (self.path, f, exc))
        return np.ascontiguousarray(a, np.uint8 if mode == "L" else np.uint16)

    def __len__(self):
        return len(self.pages)

    def page(self, f):
        if not 0 <= f < len(self.pages):
            raise IndexError("page %d of %d" % (f, len(self.pages)))
        H, W = self.shape
        if self._pil is not None:
            a = self._pil_page(f)
            if a.shape != (H, W):
                raise ValueError("%s: page %d is %r, the first %r (at offset 0)" % (self.path, f, a.shape, (H, W)))
            return a
        start, parts = self.pages[f]
        if parts is None:
            return np.frombuffer(self._view, self._dtype, H * W, start).reshape(H, W)
        raw = np.concatenate([np.frombuffer(self._view, np.uint8, n, o) for o, n in parts])
        return raw.view(self._dtype).reshape(H, W)

    def close(self):
        p, self._pil = getattr(self, "_pil", None), None
        if p is not None:
            p.close()
        v, self._view = getattr(self, "_view", None), None
        if v is not None:
            try:
                v.release()
            except BufferError:                                   # a caller still holds a page: see below
                pass
        m, self._map = getattr(self, "_map", None), None
        if m is not None:
            try:
                m.close()
            except BufferError:                                   # the map stays valid for the pages still held and is
                pass                                              # unmapped when the last of them is dropped
        f, self._f = getattr(self, "_f", None), None
        if f is not None:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---- frames of either kind ---------------------------------------------------------------------------------------------
class _Frames:
    """(frames, H, W) unsigned 16-bit pixels of an array or a TiffStack: ``block(f0, f1)`` -> the frames' bytes as one
    C-contiguous '<u2' array as they lie in memory (a view of an array; pages of a stack are put together), to be read
    with ``swap`` (1: the two bytes of every pixel exchanged); ``values(f0, f1)`` -> the same frames as numbers."""

    def __init__(self, src):
        self.stack = src if isinstance(src, TiffStack) else None
        if self.stack is not None:
            if src.bits != 16:
                raise ValueError("%s: %d-bit pages, expected 16-bit" % (src.path, src.bits))
            self.F, (self.H, self.W), self.swap = len(src), src.shape, src.swap
        else:
            a = np.asarray(src)
            if a.dtype.kind != "u" or a.dtype.itemsize != 2 or a.ndim != 3:
                raise ValueError("expected unsigned 16-bit frames of shape (frames, H, W), got %s %r" % (a.dtype, a.shape))
            self.swap = 0 if a.dtype.byteorder in ("<", "=", "|") else 1
            self.a = np.ascontiguousarray(a).view("<u2")
            self.F, self.H, self.W = a.shape
        if self.F < 1:
            raise ValueError("no frames")

    def block(self, f0, f1):
        if self.stack is None:
            return self.a[f0:f1]
        return np.stack([self.stack.page(f).view("<u2") for f in range(f0, f1)])    # (the bytes as they lie in the file)

    def values(self, f0, f1):
        b = self.block(f0, f1)
        return b.byteswap() if self.swap else b


class _Handle:
    """hm_deep_*: one native handle (include/hydra_mi.h, "16-bit input")."""

    def __init__(self, W, H, run, device):
        self.W, self.H, self.run, self.device = int(W), int(H), int(run), int(device)
        self._h = None
        h = _lib.c_vp()
        _lib.check(_lib.lib().hm_deep_create(self.device, self.W, self.H, self.run, ctypes.byref(h)), "hm_deep_create")
        self._h = h
        _lib.register(self, 2)

    def set_lut(self, lut, lo, hi):
        lut = np.ascontiguousarray(lut, np.uint8)
        if lut.shape != (VALUES,):
            raise ValueError("a table of shape %r, expected (65536,)" % (lut.shape,))
        _lib.check(_lib.lib().hm_deep_set_lut(self._h, _lib.ptr(lut), int(lo), int(hi)), "hm_deep_set_lut")

    def hist_add(self, block, swap):
        _lib.check(_lib.lib().hm_deep_hist_add(self._h, block.shape[0], _lib.ptr(block), int(swap)), "hm_deep_hist_add")

    def hist_reset(self):
        _lib.check(_lib.lib().hm_deep_hist_reset(self._h), "hm_deep_hist_reset")

    def hist_get(self):
        hist = np.zeros(VALUES, np.uint64)
        n = ctypes.c_uint64()
        _lib.check(_lib.lib().hm_deep_hist_get(self._h, _lib.ptr(hist), ctypes.byref(n)), "hm_deep_hist_get")
        return hist, int(n.value)

    def map_run_dev(self, block, swap, d_frame, d_mask, d_shown, stride, threshold, d_status, stream):
        def vp(x):
            return ctypes.c_void_p(int(x)) if x else None
        _lib.check(_lib.lib().hm_deep_map_run_dev(self._h, block.shape[0], _lib.ptr(block), int(swap), vp(d_frame), vp(d_mask),
                                                  vp(d_shown), int(stride), int(threshold), vp(d_status), stream),
                   "hm_deep_map_run_dev")

    def map(self, frame, swap):
        """one frame, synchronous -> ((H, W) uint8, [below lo, above hi])"""
        frame = np.ascontiguousarray(frame).view("<u2")
        out = np.empty((self.H, self.W), np.uint8)
        clip = np.zeros(2, np.uint32)
        _lib.check(_lib.lib().hm_deep_map(self._h, _lib.ptr(frame), int(swap), _lib.ptr(out), _lib.ptr(clip)), "hm_deep_map")
        return out, clip

    def uploaded(self):
        last, total = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(_lib.lib().hm_deep_uploaded(self._h, ctypes.byref(last), ctypes.byref(total)), "hm_deep_uploaded")
        return int(last.value), int(total.value)

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.check(_lib.lib().hm_deep_destroy(h), "hm_deep_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the four steps ----------------------------------------------------------------------------------------------------
def histogram(stack_or_array, device=0, run=8):
    """h[v], v = 0..65535: the pixels of every frame, exact, as uint64.  device=None: np.bincount on the host."""
    fr = stack_or_array if isinstance(stack_or_array, _Frames) else _Frames(stack_or_array)
    if device is None:
        hist = np.zeros(VALUES, np.uint64)
        for f in range(fr.F):
            hist += np.bincount(fr.values(f, f + 1).reshape(-1), minlength=VALUES).astype(np.uint64)
        return hist
    h = _Handle(fr.W, fr.H, run, device)
    try:
        step = run if fr.stack is not None else max(run, (64 << 20) // (2 * fr.W * fr.H))   # (an array is handed over in large pieces)
        for f0 in range(0, fr.F, step):
            h.hist_add(fr.block(f0, min(f0 + step, fr.F)), fr.swap)
        return h.hist_get()[0]
    finally:
        h.close()


def window(hist, lo_ppm=DEFAULT_LO_PPM, hi_ppm=DEFAULT_HI_PPM):
    """The window of a histogram -> (lo, hi), in integers (include/hydra_mi.h, "Window"): lo leaves lo_ppm parts per
    million of the pixels below it, hi at most 10^6 - hi_ppm above it."""
    hist = np.asarray(hist)
    lo_ppm, hi_ppm = int(lo_ppm), int(hi_ppm)
    if hist.shape != (VALUES,) or hist.dtype.kind not in "ui" or (hist.dtype.kind == "i" and (hist < 0).any()):
        raise ValueError("window: a histogram is 65536 non-negative integer counts")
    if not (0 <= lo_ppm <= MILLION and 0 <= hi_ppm <= MILLION):
        raise ValueError("window: lo_ppm %d and hi_ppm %d must lie in 0..1000000" % (lo_ppm, hi_ppm))
    cum = np.cumsum(hist.astype(np.uint64), dtype=np.uint64)
    N = int(cum[-1])
    if N < 1:
        raise ValueError("window: the histogram is empty")
    below = N * lo_ppm // MILLION
    need = max(1, (N * hi_ppm + MILLION - 1) // MILLION)
    lo = min(int(np.searchsorted(cum, np.uint64(below), side="right")), VALUES - 1)      # (lo_ppm = 10^6: no such v)
    hi = int(np.searchsorted(cum, np.uint64(need), side="left"))
    if hi <= lo:
        hi = lo + 1
        if hi > VALUES - 1:
            lo, hi = VALUES - 2, VALUES - 1
    return lo, hi


def make_lut(lo, hi, gamma=1.0):
    """lut[v], v = 0..65535 (include/hydra_mi.h, "Table"): 0 up to lo, 255 from hi, between them (510 t + D) // (2 D)
    for gamma = 1 and floor(255 (t / D)^gamma + 0.5) in binary64 otherwise."""
    lo, hi, gamma = int(lo), int(hi), float(gamma)
    if not 0 <= lo < hi <= VALUES - 1:
        raise ValueError("make_lut: a window needs 0 <= lo < hi <= 65535, got %d, %d" % (lo, hi))
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise ValueError("make_lut: gamma %r is not a positive number" % (gamma,))
    D = hi - lo
    t = np.clip(np.arange(VALUES, dtype=np.int64), lo, hi) - lo
    if gamma == 1.0:
        return ((510 * t + D) // (2 * D)).astype(np.uint8)
    ramp = np.array([math.floor(255.0 * (i / D) ** gamma + 0.5) for i in range(D + 1)], np.int64)
    return ramp[t].astype(np.uint8)


def map_video(stack_or_array, lut, lo, hi, device=0, run=8):
    """Every frame through the table -> (frames (F, H, W) uint8, clipped (F, 2) uint32: a frame's pixels below lo and
    above hi).  device=None: lut[min(max(a, lo), hi)] on the host."""
    fr = stack_or_array if isinstance(stack_or_array, _Frames) else _Frames(stack_or_array)
    lut = np.ascontiguousarray(lut, np.uint8)
    lo, hi = int(lo), int(hi)
    if lut.shape != (VALUES,) or not 0 <= lo < hi <= VALUES - 1:
        raise ValueError("map_video: a table of 65536 bytes and a window 0 <= lo < hi <= 65535, got %r, %d, %d" % (lut.shape, lo, hi))
    out = np.empty((fr.F, fr.H, fr.W), np.uint8)
    clipped = np.zeros((fr.F, 2), np.uint32)
    if device is None:
        for f in range(fr.F):
            a = fr.values(f, f + 1)[0]
            out[f] = lut[np.clip(a, lo, hi)]
            clipped[f] = np.count_nonzero(a < lo), np.count_nonzero(a > hi)
        return out, clipped
    n = fr.H * fr.W
    words = (run * n + 3) & ~3                                    # the clip words, 4-byte aligned behind the frames
    h = _Handle(fr.W, fr.H, run, device)
    buf = DeviceBuffer(words + 8 * run, device)
    L = _lib.lib()
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(int(device), ctypes.byref(stream)), "hm_copy_stream_create")
    try:
        h.set_lut(lut, lo, hi)
        for f0 in range(0, fr.F, run):
            k = min(run, fr.F - f0)
            h.map_run_dev(fr.block(f0, f0 + k), fr.swap, buf.ptr, None, None, n, 0, buf.ptr + words, stream)
            _lib.check(L.hm_copy_stream_sync(int(device), stream), "hm_copy_stream_sync")
            buf.download(out[f0:f0 + k].reshape(-1))
            buf.download(clipped[f0:f0 + k].reshape(-1), words)
    finally:
        L.hm_copy_stream_destroy(int(device), stream)
        buf.close()
        h.close()
    return out, clipped


class DeepSource:
    """A frame source of FlowEKFPipeline over 16-bit frames (an array or a TiffStack): the device maps them through the
    table and writes the ring's raw frame, mask (raw > threshold) and shown frame (mask x raw) itself; 2 W H bytes a
    frame cross the bus, against the 3 W H of three staged 8-bit planes.

    ``len``, ``.shape`` and ``frame_at(f)`` -> host (frame, mask, shown) as VideoStream gives them, taken from ``frames``
    (the mapped video, when the caller holds it anyway) or mapped on the host on demand.  ``upload_run`` is what
    FrameRing.ensure calls instead of staging three planes per frame.  ``.clipped`` (F, 2) uint32 holds a frame's pixels
    below lo and above hi once the frame's upload has been waited for (FrameRing.sync)."""

    def __init__(self, stack_or_array, lut, lo, hi, threshold, device=0, run=8, frames=None):
        self.fr = _Frames(stack_or_array)
        self.lut, self.lo, self.hi = np.ascontiguousarray(lut, np.uint8), int(lo), int(hi)
        self.threshold, self.device, self.run = threshold, int(device), int(run)
        if not 0 <= int(np.floor(threshold)) <= 255:              # (what hm_deep_map_run_dev would refuse, said before anything runs)
            raise ValueError("DeepSource: threshold %r outside 0..255, the scale of the mapped frames" % (threshold,))
        F, H, W = self.fr.F, self.fr.H, self.fr.W
        self.frames = None if frames is None else np.ascontiguousarray(frames, np.uint8)
        if self.frames is not None and self.frames.shape != (F, H, W):
            raise ValueError("DeepSource: frames of shape %r for a video of %r" % (self.frames.shape, (F, H, W)))
        self._pin = None
        self.handle = _Handle(W, H, self.run, device)
        self.handle.set_lut(self.lut, self.lo, self.hi)
        pin = _lib.c_vp()
        _lib.check(_lib.lib().hm_host_alloc(8 * F, ctypes.byref(pin)), "hm_host_alloc")
        self._pin = pin
        ctypes.memset(pin.value, 0, 8 * F)
        self.clipped = np.ctypeslib.as_array(ctypes.cast(pin, ctypes.POINTER(ctypes.c_uint32)), shape=(F, 2))
        _lib.register(self, 3)

    def __len__(self):
        return self.fr.F

    @property
    def shape(self):
        return (self.fr.H, self.fr.W)

    def frame_at(self, f):
        fr = self.frames[f] if self.frames is not None else self.lut[np.clip(self.fr.values(f, f + 1)[0], self.lo, self.hi)]
        mask = (fr > self.threshold).astype(np.uint8)
        return fr, mask, mask * fr

    def upload_run(self, f0, f1, ring):
        """Queue frames f0 .. f1 - 1 into `ring` (a FrameRing) on its copy stream: runs of consecutive slots, one map
        each, then the mirror slots by device-to-device copies.  -> the bytes queued host-to-device, 2 W H per frame."""
        sent = 0
        for f, k, s, mirror in ring.runs(f0, f1, self.run):
            d_raw, d_mask, d_shown, stride, stream = ring.run_dev(s)
            self.handle.map_run_dev(self.fr.block(f, f + k), self.fr.swap, d_raw, d_mask, d_shown, stride,
                                    int(np.floor(self.threshold)), self._pin.value + 8 * f, stream)   # raw > t for integer raw
            sent += self.handle.uploaded()[0]
            ring.mirror(mirror)
        return sent

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h is not None:
            h.close()                                             # (waits for the device: nothing writes the clip words after)
        p, self._pin = getattr(self, "_pin", None), None
        if p is not None:
            self.clipped = np.array(self.clipped)                 # (a copy that outlives the page-locked block)
            _lib.lib().hm_host_free(p)


# ---- what load_video and the command-line tools call -------------------------------------------------------------------
def depth_option(depth_range=None, depth_percentiles=None, depth_gamma=None):
    """The tools' --depth-range LO,HI, --depth-percentiles LO_PPM,HI_PPM and --depth-gamma G (strings or None) -> the
    ``depth`` of load_video: None when none is given, else a dict.  Raises ValueError for what is no pair of integers, a
    range and percentiles together, or a gamma that is no positive number."""
    def pair(s, what):
        m = re.fullmatch(r"\s*(\d+)\s*,\s*(\d+)\s*", str(s))
        if not m:
            raise ValueError("%s takes two whole numbers A,B, not %r" % (what, s))
        return int(m.group(1)), int(m.group(2))
    if depth_range is not None and depth_percentiles is not None:
        raise ValueError("--depth-range gives the window, --depth-percentiles asks for one: not both")
    depth = {}
    if depth_range is not None:
        depth["lo"], depth["hi"] = pair(depth_range, "--depth-range")
    if depth_percentiles is not None:
        depth["lo_ppm"], depth["hi_ppm"] = pair(depth_percentiles, "--depth-percentiles")
    if depth_gamma is not None:
        try:
            depth["gamma"] = float(depth_gamma)
        except (TypeError, ValueError):
            raise ValueError("--depth-gamma takes a positive number, not %r" % (depth_gamma,))
        if not (math.isfinite(depth["gamma"]) and depth["gamma"] > 0.0):
            raise ValueError("--depth-gamma takes a positive number, not %r" % (depth_gamma,))
    return depth or None


def resolve(stack_or_array, depth=None, device=0):
    """``depth`` (None, {lo, hi, gamma} or {lo_ppm, hi_ppm, gamma}; every key optional) -> dict(lo, hi, gamma, lo_ppm,
    hi_ppm, lut).  Without lo and hi the window is that of the histogram of every frame."""
    depth = dict(depth or {})
    unknown = set(depth) - {"lo", "hi", "gamma", "lo_ppm", "hi_ppm"}
    if unknown:
        raise ValueError("depth: unknown keys %s" % sorted(unknown))
    if ("lo" in depth) != ("hi" in depth) or ("lo" in depth and ("lo_ppm" in depth or "hi_ppm" in depth)):
        raise ValueError("depth: give lo and hi, or lo_ppm and hi_ppm, not a mixture")
    gamma = float(depth.get("gamma", 1.0))
    lo_ppm, hi_ppm = int(depth.get("lo_ppm", DEFAULT_LO_PPM)), int(depth.get("hi_ppm", DEFAULT_HI_PPM))
    if "lo" in depth:
        lo, hi = int(depth["lo"]), int(depth["hi"])
    else:
        lo, hi = window(histogram(stack_or_array, device), lo_ppm, hi_ppm)
    return dict(lo=lo, hi=hi, gamma=gamma, lo_ppm=lo_ppm, hi_ppm=hi_ppm, lut=make_lut(lo, hi, gamma))


def default_device():
    """0 with a GPU, None (the host path) without."""
    return 0 if _lib.lib().hm_device_count() > 0 else None


def open_deep(fn):
    """The 16-bit frames behind a file name -> a TiffStack or a (frames, H, W) uint16 array; None when the file holds
    anything else (8-bit frames, colour, an .avi), which load_video reads as ever."""
    name = str(fn).lower()
    if not os.path.isfile(str(fn)):
        return None                                               # (whoever reads the file next says that it is missing)
    if name.endswith((".tif", ".tiff")):
        try:
            st = TiffStack(fn)
        except ValueError:
            return None                                           # (RGB pages and what is no TIFF: load_video says what it is)
        if st.bits == 16 and len(st) >= 1:
            return st
        st.close()
        return None
    def deep(dtype, shape):
        return dtype.kind == "u" and dtype.itemsize == 2 and len(shape) == 3
    if name.endswith(".npy"):
        try:
            a = np.load(fn, mmap_mode="r")                        # (maps the file: the header alone is read)
        except ValueError:
            return None                                           # (an object array: load_video says what it is)
        return a if deep(a.dtype, a.shape) else None
    if name.endswith(".npz"):
        # the first member's header alone: an 8-bit archive is not decompressed here and again by load_video
        with np.load(fn) as z:
            if not z.files:
                return None
            try:
                member = z.zip.open(z.files[0] + ".npy")
            except KeyError:
                return None                                       # (no array member: load_video says what it is)
            with member as f:
                version = np.lib.format.read_magic(f)
                read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
                shape, _, dtype = read(f)
            return z[z.files[0]] if deep(dtype, shape) else None
    return None


def load_deep(fn, depth=None, device="auto"):
    """A 16-bit video through its window -> dict(frames (F, H, W) uint8, clipped (F, 2), source, lo, hi, gamma, lo_ppm,
    hi_ppm, lut), or None when `fn` holds no 16-bit frames.  ``source`` is what DeepSource takes (close it when it is a
    TiffStack)."""
    src = open_deep(fn)
    if src is None:
        return None
    if device == "auto":
        device = default_device()
    fr = _Frames(src)
    win = resolve(fr, depth, device)
    frames, clipped = map_video(fr, win["lut"], win["lo"], win["hi"], device)
    return dict(win, frames=frames, clipped=clipped, source=src)


def clip_warning(clipped, pixels, hi_ppm=DEFAULT_HI_PPM):
    """One line when more than 10 (10^6 - hi_ppm) parts per million of a frame's pixels lie above hi -- ten times the
    share the window itself allows on average -- naming the worst frame and its share; else None."""
    clipped = np.asarray(clipped)
    if clipped.size == 0:
        return None
    worst = int(np.argmax(clipped[:, 1]))
    count = int(clipped[worst, 1])
    if count * MILLION <= 10 * (MILLION - int(hi_ppm)) * int(pixels):
        return None
    return ("Warning: the depth window saturates: %d of %d pixels (%.4f %%) of frame %d lie above hi, more than ten times the "
            "%.4f %% the window allows" % (count, pixels, 100.0 * count / pixels, worst, (MILLION - int(hi_ppm)) / 1e4))
