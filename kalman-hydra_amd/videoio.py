"""Video and image output of the tracker: the library's AVI container, PNG files and the flow tool's preview.

``AviWriter`` wraps hm_avi_open / hm_avi_write / hm_avi_close (uncompressed 24-bit AVI at the reference's 20 frames/s,
src/optical_flow_ext.cpp:358; OpenDML continuation past 1 GiB) and, with codec="mjpeg", hm_avi_open_codec /
hm_avi_write_chunk around the device's JPEG encoder (hm_mjpeg_*); ``read_avi`` gives the frames of either back.  Frames are (H, W, 3) uint8 in B, G, R order, rows top
to bottom, as every view of ``Renderer.view`` is.

Reading: ``AviReader`` maps an AVI of any writer (Motion-JPEG or uncompressed 24-bit), ``MjpegDecoder`` wraps hm_mjpeg_dec_*
(the baseline JPEG decoder on the device, bit-equal to libjpeg), ``decode_avi`` is what ``sources.load_video`` calls for an
MJPG file and ``AviSource`` feeds the pipeline's frame ring with JPEG bytes that the device decodes in place.
"""
import ctypes

import numpy as np

from . import _lib
from .devbuf import DeviceBuffer

#: view names of Renderer.view -> the view ids of hm_view (include/hydra_mi.h)
VIEWS = {"raw": 0, "overlay": 1, "texture": 2, "mask": 3, "flowx": 4, "flowy": 5}


#: codec names of AviWriter -> the codec ids of hm_avi_open_codec
CODECS = {"raw": 0, "mjpeg": 1}
#: bytes a download of an MJPEG stream is rounded up to (VideoTap, BodyTap, AviWriter.write_dev)
MJPEG_GRANULE = 256


class MjpegEncoder:
    """hm_mjpeg_*: the baseline JPEG encoder on the device (include/hydra_mi.h, "Motion-JPEG").  Frames are (H, W, 3) B G R
    or, with channels=1, (H, W) uint8.  ``header`` is SOI through SOS; the device produces the stream that follows."""

    def __init__(self, width, height, channels=3, quality=90, restart_rows=1, device=0):
        self.width, self.height, self.channels, self.device = int(width), int(height), int(channels), int(device)
        self.quality, self.restart_rows = int(quality), int(restart_rows)
        self._h = None
        h = _lib.c_vp()
        L = _lib.lib()
        _lib.check(L.hm_mjpeg_create(self.device, self.width, self.height, self.channels, self.quality, self.restart_rows,
                                     ctypes.byref(h)), "hm_mjpeg_create")
        self._h = h
        n = ctypes.c_uint64()
        _lib.check(L.hm_mjpeg_header(h, None, 0, ctypes.byref(n)), "hm_mjpeg_header")
        buf = np.empty(n.value, np.uint8)
        _lib.check(L.hm_mjpeg_header(h, _lib.ptr(buf), buf.nbytes, ctypes.byref(n)), "hm_mjpeg_header")
        self.header = buf.tobytes()
        self.max_bytes = int(L.hm_mjpeg_max_bytes(h))
        self.max_stream = self.max_bytes - len(self.header)
        _lib.register(self, 2)

    def frame_shape(self):
        return (self.height, self.width, 3) if self.channels == 3 else (self.height, self.width)

    def encode(self, frame, cap=None):
        """A host frame -> the bytes of its JPEG file (cap: the buffer to offer, default max_bytes)."""
        a = np.ascontiguousarray(frame, np.uint8)
        if a.shape != self.frame_shape():
            raise ValueError("frame of shape %r for a %dx%d x %d encoder" % (a.shape, self.width, self.height, self.channels))
        out = np.empty(self.max_bytes if cap is None else int(cap), np.uint8)
        n = ctypes.c_uint64()
        _lib.check(_lib.lib().hm_mjpeg_encode(self._h, _lib.ptr(a), _lib.ptr(out), out.nbytes, ctypes.byref(n)),
                   "hm_mjpeg_encode")
        return out[:n.value].tobytes()

    def encode_dev(self, d_frame, d_out, cap, size_word, stream):
        """Queue the encode of the frame at device address d_frame on `stream`: the stream's bytes to address d_out (device
        or page-locked, cap bytes), its size to the uint32 at address size_word (device or page-locked)."""
        _lib.check(_lib.lib().hm_mjpeg_encode_dev(self._h, ctypes.c_void_p(int(d_frame)), ctypes.c_void_p(int(d_out)), int(cap),
                                                  ctypes.c_void_p(int(size_word)), stream), "hm_mjpeg_encode_dev")

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.check(_lib.lib().hm_mjpeg_destroy(h), "hm_mjpeg_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MjpegSlots:
    """Page-locked landing slots of MJPEG frames for a writer thread: a slot holds the size word, the encoder's header and
    room for a stream, laid out so that header and stream are one JPEG file.  ``finish`` is the writer thread's half: it
    reads the size the device wrote, copies exactly that much of the stream (rounded up to MJPEG_GRANULE) on a copy
    stream of its own and appends the file to the video.

    ``cap`` is what the device may write (the largest stream there is, hm_mjpeg_max_bytes); the page-locked room is
    `room` bytes a slot, by default half the raw frame (at least 64 KiB), since page-locking memory takes time by the
    megabyte and the worst case is 6.5 times the raw frame.  A stream that does not fit the room (noise at quality 100
    can pass the raw frame's size) is copied through ordinary memory instead: slower, the same file."""

    def __init__(self, encoder, slots, device=0, room=None):
        self.enc, self.device, self.slots = encoder, int(device), int(slots)
        g = MJPEG_GRANULE
        hdr = len(encoder.header)
        self.cap = encoder.max_stream
        raw = encoder.width * encoder.height * encoder.channels
        self.room = min(self.cap, max(64 << 10, raw // 2) if room is None else int(room))
        self.room = (self.room + g - 1) // g * g
        self.off = (16 + hdr + g - 1) // g * g                   # the stream's offset in a slot: the header ends there
        self.stride = self.off + self.room
        L = _lib.lib()
        self._pin = _lib.c_vp()
        _lib.check(L.hm_host_alloc(self.slots * self.stride, ctypes.byref(self._pin)), "hm_host_alloc")
        self._stream = _lib.c_vp()
        _lib.check(L.hm_copy_stream_create(self.device, ctypes.byref(self._stream)), "hm_copy_stream_create")
        for s in range(self.slots):
            ctypes.memmove(self._pin.value + s * self.stride + self.off - hdr, encoder.header, hdr)
        self.copied = 0                                           # bytes downloaded so far (tools/mjpeg_cost.py)

    def size_word(self, s):
        return self._pin.value + s * self.stride

    def finish(self, s, d_stream, writer):
        size = ctypes.c_uint32.from_address(self.size_word(s)).value
        if size > self.cap:
            raise RuntimeError("MJPEG: a stream of %d bytes for a slot of %d" % (size, self.cap))
        g = MJPEG_GRANULE
        n = min((size + g - 1) // g * g, self.cap)                # (never past the device's part of the slot)
        base = self._pin.value + s * self.stride
        L = _lib.lib()
        if n > self.room:                                         # through ordinary memory
            buf = np.empty(len(self.enc.header) + size, np.uint8)
            buf[:len(self.enc.header)] = np.frombuffer(self.enc.header, np.uint8)
            _lib.check(L.hm_dev_download(self.device, ctypes.c_void_p(buf.ctypes.data + len(self.enc.header)),
                                         ctypes.c_void_p(int(d_stream)), size), "hm_dev_download")
            self.copied += size
            return writer.write_chunk_ptr(buf.ctypes.data, buf.nbytes)
        _lib.check(L.hm_dev_download_async(self.device, base + self.off, d_stream, n, self._stream), "hm_dev_download_async")
        _lib.check(L.hm_copy_stream_sync(self.device, self._stream), "hm_copy_stream_sync")
        self.copied += n
        hdr = len(self.enc.header)
        writer.write_chunk_ptr(base + self.off - hdr, hdr + size)

    def close(self):
        L = _lib.lib()
        if self._stream:
            L.hm_copy_stream_destroy(self.device, self._stream)
            self._stream = None
        if self._pin:
            L.hm_host_free(self._pin)
            self._pin = None


class AviWriter:
    """with AviWriter("out.avi", W, H) as v: v.write(bgr) ...   (riff_limit: bytes per RIFF, 0 = 1 GiB)

    codec "raw": uncompressed 24-bit frames, as ever.  codec "mjpeg": every frame is coded as a baseline JPEG on the
    device (quality 1..100, restart_rows rows of blocks per restart interval) and the file is Motion-JPEG.  channels=1:
    the frames are grey, (H, W); a raw file still stores them as B = G = R, an MJPEG file codes one component."""

    def __init__(self, path, width, height, fps=20, riff_limit=0, codec="raw", quality=90, channels=3, device=0,
                 restart_rows=1):
        self.path, self.width, self.height = str(path), int(width), int(height)
        if codec not in CODECS:
            raise ValueError("AviWriter: codec %r is none of %s" % (codec, sorted(CODECS)))
        if channels not in (1, 3):
            raise ValueError("AviWriter: %r channels, not 1 or 3" % (channels,))
        self.codec, self.channels, self.device = codec, int(channels), int(device)
        self.frames = 0
        self._h = None
        self.encoder = None
        self._dev = None
        h = _lib.c_vp()
        if codec == "raw":
            _lib.check(_lib.lib().hm_avi_open(self.path.encode(), self.width, self.height, int(fps), int(riff_limit),
                                              ctypes.byref(h)), "hm_avi_open")
        else:
            self.encoder = MjpegEncoder(self.width, self.height, self.channels, quality, restart_rows, device)
            _lib.check(_lib.lib().hm_avi_open_codec(self.path.encode(), self.width, self.height, int(fps), int(riff_limit),
                                                    CODECS[codec], ctypes.byref(h)), "hm_avi_open_codec")
        self._h = h
        _lib.register(self, 4)

    @property
    def mjpeg(self):
        return self.codec == "mjpeg"

    def write(self, bgr):
        if self._h is None:
            raise ValueError("write to a closed AviWriter")
        a = np.ascontiguousarray(bgr, np.uint8)
        if self.mjpeg:
            if a.shape != self.encoder.frame_shape():
                raise ValueError("frame of shape %r for a %dx%d video of %d channels" % (a.shape, self.width, self.height,
                                                                                         self.channels))
            return self.write_chunk(self.encoder.encode(a))
        if self.channels == 1 and a.shape == (self.height, self.width):
            a = np.repeat(a[:, :, None], 3, axis=2)
        if a.shape != (self.height, self.width, 3):
            raise ValueError("frame of shape %r for a %dx%d video" % (a.shape, self.width, self.height))
        _lib.check(_lib.lib().hm_avi_write(self._h, _lib.ptr(a)), "hm_avi_write")
        self.frames += 1

    def write_grey(self, plane):
        """Append a grey frame (H, W): one component in an MJPEG video of channels=1, B = G = R otherwise."""
        a = np.ascontiguousarray(plane, np.uint8)
        self.write(a if self.channels == 1 else np.repeat(a[:, :, None], 3, axis=2))

    def write_ptr(self, address):
        """Append the frame at a host address (H x W x 3 bytes, e.g. a page-locked staging buffer)."""
        _lib.check(_lib.lib().hm_avi_write(self._h, ctypes.c_void_p(int(address))), "hm_avi_write")
        self.frames += 1

    def write_chunk(self, data):
        """Append one compressed frame (the bytes of a whole JPEG file) to an MJPEG video."""
        b = np.frombuffer(bytes(data), np.uint8)
        self.write_chunk_ptr(b.ctypes.data, b.nbytes)

    def write_chunk_ptr(self, address, n):
        _lib.check(_lib.lib().hm_avi_write_chunk(self._h, ctypes.c_void_p(int(address)), int(n)), "hm_avi_write_chunk")
        self.frames += 1

    def write_dev(self, d_frame, stream):
        """Encode the frame at device address d_frame (H x W x channels bytes), queued on `stream`, and append it: the
        frame never reaches the host, only its stream does.  Waits for the stream.  (MJPEG only.)"""
        if not self.mjpeg:
            raise ValueError("AviWriter.write_dev: the video is not MJPEG (codec=%r)" % self.codec)
        if self._h is None:
            raise ValueError("write to a closed AviWriter")
        if self._dev is None:
            self._slots = MjpegSlots(self.encoder, 1, self.device)
            self._dev = DeviceBuffer(self._slots.cap, self.device)
        self.encoder.encode_dev(d_frame, self._dev.ptr, self._slots.cap, self._slots.size_word(0), stream)
        _lib.check(_lib.lib().hm_copy_stream_sync(self.device, stream), "hm_copy_stream_sync")
        self._slots.finish(0, self._dev.ptr, self)

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            try:
                if self._dev is not None:
                    self._slots.close()
                    self._dev.close()
                    self._dev = None
                if self.encoder is not None:
                    self.encoder.close()
            finally:
                _lib.check(_lib.lib().hm_avi_close(h), "hm_avi_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grey_opts(video_opts):
    """AviWriter's codec options for a grey video: an MJPEG video codes one component, a raw one stays as it is."""
    opts = dict(video_opts or {})
    if opts.get("codec", "raw") == "mjpeg":
        opts["channels"] = 1
    return opts


def read_avi(path):
    """The frames of an AVI this library wrote, raw or MJPEG -> a list of (H, W, 3) B G R uint8 arrays, or (H, W) for the
    frames of a one-component MJPEG video.  Walks the 'movi' lists of every RIFF in file order; JPEG chunks are decoded
    by PIL."""
    import struct
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"RIFF" or b[8:12] != b"AVI ":
        raise ValueError("%s is not an AVI file" % path)

    def chunks(start, end):
        p = start
        while p + 8 <= end:
            cc, size = b[p:p + 4], struct.unpack_from("<I", b, p + 4)[0]
            if cc in (b"RIFF", b"LIST"):
                yield b[p + 8:p + 12], p + 12, size - 4
            else:
                yield cc, p + 8, size
            p += 8 + size + (size & 1)

    W = H = None
    mjpg = False
    frames = []
    for _riff, r0, rn in chunks(0, len(b)):
        for cc, c0, cn in chunks(r0, r0 + rn):
            if cc == b"hdrl":
                for cc2, h0, hn in chunks(c0, c0 + cn):
                    if cc2 == b"strl":
                        for cc3, s0, _sn in chunks(h0, h0 + hn):
                            if cc3 == b"strf":
                                _, W, H, _, bits, comp = struct.unpack_from("<IiiHHI", b, s0)
                                mjpg = comp == struct.unpack("<I", b"MJPG")[0]
                                if not mjpg and (comp != 0 or bits != 24):
                                    raise ValueError("%s: neither 24-bit uncompressed nor MJPG" % path)
            elif cc == b"movi":
                for cc2, d0, dn in chunks(c0, c0 + cn):
                    if cc2 == b"00db":
                        stride = (3 * W + 3) & ~3
                        rows = np.frombuffer(b, np.uint8, stride * H, d0).reshape(H, stride)
                        frames.append(np.ascontiguousarray(rows[::-1, :3 * W].reshape(H, W, 3)))
                    elif cc2 == b"00dc":
                        frames.append(decode_jpeg(b[d0:d0 + dn]))
    return frames


def decode_jpeg(data):
    """The bytes of a JPEG file -> (H, W) uint8 for one component, else (H, W, 3) B G R uint8 (PIL)."""
    import io
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    if img.mode == "L":
        return np.asarray(img).copy()
    return np.ascontiguousarray(np.asarray(img.convert("RGB"))[:, :, ::-1])


def write_png(path, bgr):
    """A (H, W, 3) B G R or (H, W) gray uint8 image as PNG (PIL, which sources.load_video uses for TIFF)."""
    from PIL import Image
    a = np.ascontiguousarray(bgr, np.uint8)
    img = Image.fromarray(a[:, :, ::-1].copy() if a.ndim == 3 else a)
    img.save(path, format="PNG")
    return path


def read_png(path):
    """-> (H, W, 3) B G R uint8 (the inverse of write_png)."""
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"))
    return np.ascontiguousarray(a[:, :, ::-1])


def flow_preview(frames, flowx, flowy, device=0):
    """hm_flow_preview: frames (n, H, W) gray or (n, H, W, 3) B G R uint8, flow planes (n, H, W) f32 ->
    (n, H, W, 3) round((2 frame + 3 wheel) / 5), wheel the Middlebury colour code saturating at 15 px
    (reference src/optical_flow_ext.cpp:172-281, 389)."""
    fx = np.ascontiguousarray(flowx, np.float32)
    fy = np.ascontiguousarray(flowy, np.float32)
    f = np.ascontiguousarray(frames, np.uint8)
    if fx.ndim != 3 or fy.shape != fx.shape or f.shape[:3] != fx.shape or f.ndim not in (3, 4) or \
            (f.ndim == 4 and f.shape[3] != 3):
        raise ValueError("flow_preview: frames (n, H, W[, 3]) and flow planes (n, H, W), got %r, %r, %r"
                         % (f.shape, fx.shape, fy.shape))
    ch = 3 if f.ndim == 4 else 1
    n, H, W = fx.shape
    out = np.empty((n, H, W, 3), np.uint8)
    _lib.check(_lib.lib().hm_flow_preview(int(device), n, W, H, ch, _lib.ptr(f), _lib.ptr(fx), _lib.ptr(fy), _lib.ptr(out),
                                          0, None), "hm_flow_preview")
    return out


# ---- reading: the Motion-JPEG decoder on the device and AVI files of any writer --------------------------------------
#: entropy paths of MjpegDecoder -> HM_MJPEG_ENTROPY_*
ENTROPY = {"auto": 0, "host": 1, "device": 2}
#: biCompression values that carry plain baseline JPEG frames
MJPEG_FOURCCS = (b"MJPG", b"mjpg", b"AVI1", b"JPEG", b"jpeg")


class _MjpegInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("W", "H", "components", "hs", "vs", "ri")] + \
               [("intervals", ctypes.c_uint32), ("mcus", ctypes.c_uint32)]


def _bytes_view(data):
    """a uint8 array over bytes, a memoryview (e.g. of a mapped file) or an array, without a copy"""
    return data if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"] \
        else np.frombuffer(data, np.uint8)


def mjpeg_probe(data):
    """hm_mjpeg_probe: what a JPEG file's headers and marker scan say, on the host (no GPU): W, H, components, hs, vs
    (luma blocks of an MCU), ri (the DRI value, 0 without), intervals, mcus.  Raises for a stream the decoder refuses."""
    a = _bytes_view(data)
    info = _MjpegInfo()
    _lib.check(_lib.lib().hm_mjpeg_probe(_lib.ptr(a), a.nbytes, ctypes.byref(info)), "hm_mjpeg_probe")
    return {n: int(getattr(info, n)) for n, _t in _MjpegInfo._fields_}


def mjpeg_intervals(data):
    """hm_mjpeg_intervals: (intervals, 3) uint32: start, end, first MCU of every restart interval."""
    a = _bytes_view(data)
    out = np.zeros((mjpeg_probe(a)["intervals"], 3), np.uint32)
    _lib.check(_lib.lib().hm_mjpeg_intervals(_lib.ptr(a), a.nbytes, _lib.ptr(out), out.shape[0]), "hm_mjpeg_intervals")
    return out


class MjpegDecoder:
    """hm_mjpeg_dec_*: the baseline JPEG decoder on the device (include/hydra_mi.h, "Motion-JPEG, decoding").  A frame
    decodes to its grey plane (H, W) uint8: the one component, or the luma plane of a colour file.  ``entropy``: where the
    Huffman decoding runs, "auto", "host" or "device" (the same result); ``pool``: threads of the host path."""

    probe = staticmethod(mjpeg_probe)

    def __init__(self, width, height, max_run=8, device=0, entropy="auto", pool=4):
        self.width, self.height, self.max_run, self.device = int(width), int(height), int(max_run), int(device)
        self._h = None
        self.last_bad = 0
        if entropy not in ENTROPY:
            raise ValueError("MjpegDecoder: entropy %r is none of %s" % (entropy, sorted(ENTROPY)))
        h = _lib.c_vp()
        _lib.check(_lib.lib().hm_mjpeg_dec_create(self.device, self.width, self.height, self.max_run, ctypes.byref(h)),
                   "hm_mjpeg_dec_create")
        self._h = h
        _lib.register(self, 2)
        self.tune("entropy", ENTROPY[entropy])
        self.tune("pool", pool)

    def tune(self, name, value):
        _lib.check(_lib.lib().hm_mjpeg_dec_tune(self._h, name.encode(), int(value)), "hm_mjpeg_dec_tune")

    def entropy_host(self, data):
        """The host entropy path alone (no GPU): ((luma blocks, 64) int16 in scan and zigzag order, bad intervals)."""
        a = _bytes_view(data)
        cap = 4 * ((self.width + 15) // 16) * ((self.height + 15) // 16)
        coef = np.zeros((cap, 64), np.int16)
        bad = ctypes.c_uint32()
        _lib.check(_lib.lib().hm_mjpeg_dec_entropy_host(self._h, _lib.ptr(a), a.nbytes, _lib.ptr(coef), coef.size,
                                                        ctypes.byref(bad)), "hm_mjpeg_dec_entropy_host")
        info = mjpeg_probe(a)
        return coef[:info["mcus"] * info["hs"] * info["vs"]], int(bad.value)

    def decode(self, data, strict=True):
        """The bytes of a JPEG file -> (H, W) uint8, synchronous.  strict: a frame with bad restart intervals raises;
        otherwise their blocks are grey 128 and ``last_bad`` counts them."""
        a = _bytes_view(data)
        out = np.empty((self.height, self.width), np.uint8)
        bad = ctypes.c_uint32()
        rc = _lib.lib().hm_mjpeg_decode(self._h, _lib.ptr(a), a.nbytes, _lib.ptr(out), 1 if strict else 0, ctypes.byref(bad))
        self.last_bad = int(bad.value)
        _lib.check(rc, "hm_mjpeg_decode")
        return out

    def decode_run_dev(self, chunks, d_frame, d_mask=None, d_shown=None, frame_stride=None, pitch=None, threshold=0,
                       status=None, stream=None):
        """Queue the decode of up to max_run files on `stream`: frame i to device address d_frame + i frame_stride (rows
        `pitch` bytes apart, default dense) and, when given, its mask (frame > threshold) and shown frame (mask x frame)
        likewise; status: the address of len(chunks) uint32 (device or page-locked) that take the frames' bad intervals.
        -> the bytes the call queued from host to device (hm_mjpeg_dec_uploaded): descriptors, and the files with their
        interval tables (device entropy path) or the coefficients, 2 bytes a pixel (host entropy path)."""
        views = [_bytes_view(c) for c in chunks]
        n = len(views)
        files = (_lib.c_vp * n)(*[v.ctypes.data for v in views])
        sizes = (ctypes.c_uint64 * n)(*[v.nbytes for v in views])
        pitch = self.width if pitch is None else int(pitch)
        stride = pitch * self.height if frame_stride is None else int(frame_stride)

        def vp(x):
            return ctypes.c_void_p(int(x)) if x else None
        _lib.check(_lib.lib().hm_mjpeg_decode_run_dev(self._h, n, files, sizes, vp(d_frame), vp(d_mask), vp(d_shown), stride, pitch,
                                                      int(threshold), vp(status), stream), "hm_mjpeg_decode_run_dev")
        sent = ctypes.c_uint64()
        _lib.check(_lib.lib().hm_mjpeg_dec_uploaded(self._h, ctypes.byref(sent), None), "hm_mjpeg_dec_uploaded")
        return int(sent.value)

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.check(_lib.lib().hm_mjpeg_dec_destroy(h), "hm_mjpeg_dec_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AviReader:
    """The first video stream of an AVI file, mapped and not read whole: ``len``, ``shape`` (H, W), ``fps``, ``mjpeg``,
    ``chunk(f)`` (a memoryview of frame f's bytes) and, for uncompressed streams, ``frame_bgr(f)``.

    Walks every RIFF ('AVI ' and the OpenDML 'AVIX' ones) and every 'movi' list with the 'rec ' lists inside it, takes the
    '##dc' / '##db' chunks of the first stream whose strh says 'vids' (## its number in the order of the 'strl' lists) and
    steps over everything else (audio, JUNK, indexes), honouring the padding byte of odd sizes.  A zero-length video chunk
    is a dropped frame: it repeats the frame before it.  The stream is Motion-JPEG (biCompression MJPG, mjpg, AVI1 or JPEG:
    one baseline JPEG file per chunk) or uncompressed 24-bit, bottom-up or (negative biHeight) top-down; anything else is
    refused by name."""

    def __init__(self, path):
        import mmap
        import struct
        self.path = str(path)
        self._f = open(self.path, "rb")
        try:
            self._map = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            self._f.close()
            raise ValueError("%s is not an AVI file" % self.path)
        b, n = self._map, len(self._map)
        if n < 12 or b[:4] != b"RIFF" or b[8:12] != b"AVI ":
            self.close()
            raise ValueError("%s is not an AVI file" % self.path)
        self._view = memoryview(b)
        self.frames = []                                          # (offset, size) per frame
        self.width = self.height = None
        self.fps, self.mjpeg, self.top_down = 0.0, False, False
        stream, streams, usec = None, 0, 0

        def chunks(start, end):
            p = start
            while p + 8 <= end:
                cc, size = b[p:p + 4], struct.unpack_from("<I", b, p + 4)[0]
                size = min(size, end - p - 8)                     # (a file cut short, a size field never patched)
                if cc in (b"RIFF", b"LIST") and size >= 4:
                    yield b[p + 8:p + 12], p + 12, size - 4, True
                else:
                    yield cc, p + 8, size, False
                p += 8 + size + (size & 1)

        def movi(start, end, tags):
            for cc, c0, cn, is_list in chunks(start, end):
                if is_list:
                    if cc == b"rec ":
                        movi(c0, c0 + cn, tags)
                elif cc in tags:
                    if cn == 0:
                        if not self.frames:
                            raise ValueError("%s: the first frame is a dropped frame" % self.path)
                        self.frames.append(self.frames[-1])
                    else:
                        self.frames.append((c0, cn))

        try:
            for form, r0, rn, is_list in chunks(0, n):
                if not is_list or form not in (b"AVI ", b"AVIX"):
                    continue
                for cc, c0, cn, lst in chunks(r0, r0 + rn):
                    if lst and cc == b"hdrl":
                        for cc2, h0, hn, lst2 in chunks(c0, c0 + cn):
                            if cc2 == b"avih" and hn >= 4:
                                usec = struct.unpack_from("<I", b, h0)[0]
                            if not (lst2 and cc2 == b"strl"):
                                continue
                            number, streams = streams, streams + 1
                            kind, strf = None, None
                            for cc3, s0, sn, _l in chunks(h0, h0 + hn):
                                if cc3 == b"strh" and sn >= 28:
                                    kind = b[s0:s0 + 4]
                                    scale, rate = struct.unpack_from("<II", b, s0 + 20)
                                elif cc3 == b"strf":
                                    strf = (s0, sn)
                            if kind != b"vids" or stream is not None:
                                continue
                            if strf is None or strf[1] < 40:
                                raise ValueError("%s: video stream %d has no BITMAPINFOHEADER" % (self.path, number))
                            stream = number
                            _, W, H, _, bits, comp = struct.unpack_from("<IiiHHI", b, strf[0])
                            fourcc = struct.pack("<I", comp)
                            self.mjpeg = fourcc in MJPEG_FOURCCS
                            if not self.mjpeg:
                                if comp != 0:
                                    raise ValueError("%s: codec %r: neither Motion-JPEG nor uncompressed 24-bit"
                                                     % (self.path, fourcc.decode("latin-1")))
                                if bits != 24:
                                    raise ValueError("%s: uncompressed %d-bit%s frames, not 24-bit"
                                                     % (self.path, bits, " palettised" if bits <= 8 else ""))
                            self.width, self.height, self.top_down = W, abs(H), H < 0
                            self.fps = rate / scale if scale and rate else (1e6 / usec if usec else 0.0)
                    elif lst and cc == b"movi":
                        if stream is None:
                            raise ValueError("%s: no video stream before the frames" % self.path)
                        tags = (b"%02ddc" % stream, b"%02ddb" % stream)
                        movi(c0, c0 + cn, tags)
            if stream is None:
                raise ValueError("%s: no video stream" % self.path)
            if self.width < 1 or self.height < 1:
                raise ValueError("%s: frames of %dx%d" % (self.path, self.width, self.height))
        except Exception:
            self.close()
            raise

    def __len__(self):
        return len(self.frames)

    @property
    def shape(self):
        return (self.height, self.width)

    def chunk(self, f):
        off, size = self.frames[f]
        return self._view[off:off + size]

    def frame_bgr(self, f):
        """Frame f of an uncompressed stream -> (H, W, 3) B G R uint8, rows top to bottom."""
        if self.mjpeg:
            raise ValueError("%s is Motion-JPEG: decode chunk(f)" % self.path)
        stride = (3 * self.width + 3) & ~3
        c = self.chunk(f)
        if len(c) < stride * self.height:
            raise ValueError("%s: frame %d has %d bytes, %d are needed" % (self.path, f, len(c), stride * self.height))
        rows = np.frombuffer(c, np.uint8, stride * self.height).reshape(self.height, stride)
        if not self.top_down:
            rows = rows[::-1]
        return np.ascontiguousarray(rows[:, :3 * self.width].reshape(self.height, self.width, 3))

    def close(self):
        v, self._view = getattr(self, "_view", None), None
        if v is not None:
            v.release()
        m, self._map = getattr(self, "_map", None), None
        if m is not None:
            try:
                m.close()
            except BufferError:                                   # a caller still holds a chunk: the map stays valid for it
                pass                                              # and is unmapped when the last such view is dropped
        f, self._f = getattr(self, "_f", None), None
        if f is not None:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def decode_avi(reader, device=0, run=8, entropy="auto"):
    """Every frame of a Motion-JPEG AviReader through the device decoder, `run` frames a call -> (frames, H, W) uint8."""
    H, W = reader.shape
    F = len(reader)
    out = np.empty((F, H, W), np.uint8)
    dec = MjpegDecoder(W, H, run, device, entropy)
    words = (run * H * W + 3) & ~3                                # the status words, 4-byte aligned behind the frames
    buf = DeviceBuffer(words + 4 * run, device)
    L = _lib.lib()
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(int(device), ctypes.byref(stream)), "hm_copy_stream_create")
    try:
        status = np.zeros(run, np.uint32)
        for f0 in range(0, F, run):
            k = min(run, F - f0)
            dec.decode_run_dev([reader.chunk(f) for f in range(f0, f0 + k)], buf.ptr, status=buf.ptr + words, stream=stream)
            _lib.check(L.hm_copy_stream_sync(int(device), stream), "hm_copy_stream_sync")
            buf.download(out[f0:f0 + k].reshape(-1))
            buf.download(status[:k], words)
            if status[:k].any():
                bad = int(np.flatnonzero(status[:k])[0])
                raise ValueError("%s: frame %d has %d bad restart intervals (malformed JPEG data)"
                                 % (reader.path, f0 + bad, status[bad]))
    finally:
        L.hm_copy_stream_destroy(int(device), stream)
        buf.close()
        dec.close()
    return out


class AviSource:
    """A frame source of FlowEKFPipeline over a Motion-JPEG AVI: the device decoder writes the ring's raw frame, mask
    (frame > threshold) and shown frame (mask x frame) itself.  What crosses the bus depends on the entropy path
    (MjpegDecoder): on the device path the JPEG bytes, their interval table and a 5.6 KB descriptor per frame; on the host
    path, which "auto" takes below 512 restart intervals a frame, the Huffman decoding runs on the CPU and the
    coefficients are uploaded, 2 bytes a pixel.  The ring's ``bytes_uploaded`` counts what was really queued.

    ``len``, ``.shape`` and ``frame_at(f)`` -> host (frame, mask, shown) as VideoStream gives them; frame_at takes the
    frames from ``frames`` (the decoded video, when the caller holds it anyway) or decodes on demand.  ``upload_run`` is
    what FrameRing.ensure calls instead of staging three planes per frame."""

    def __init__(self, path, threshold, device=0, frames=None, run=8, entropy="auto"):
        self.reader = AviReader(path)
        if not self.reader.mjpeg:
            self.reader.close()
            raise ValueError("%s is not Motion-JPEG: load it with load_video" % path)
        self.threshold, self.device, self.run = threshold, int(device), int(run)
        H, W = self.reader.shape
        self.decoder = MjpegDecoder(W, H, self.run, device, entropy)
        self.frames = None if frames is None else np.ascontiguousarray(frames, np.uint8)
        if self.frames is not None and self.frames.shape != (len(self.reader), H, W):
            raise ValueError("AviSource: frames of shape %r for a video of %r" % (self.frames.shape, (len(self.reader), H, W)))
        _lib.register(self, 3)

    def __len__(self):
        return len(self.reader)

    @property
    def shape(self):
        return self.reader.shape

    def frame_at(self, f):
        fr = self.frames[f] if self.frames is not None else self.decoder.decode(self.reader.chunk(f))
        mask = (fr > self.threshold).astype(np.uint8)
        return fr, mask, mask * fr

    def upload_run(self, f0, f1, ring):
        """Queue frames f0 .. f1 - 1 into `ring` (a FrameRing) on its copy stream: runs of consecutive slots, one
        decode each, then the mirror slots by device-to-device copies.  -> the bytes queued host-to-device, as the
        decoder counted them."""
        sent = 0
        for f, k, s, mirror in ring.runs(f0, f1, self.run):
            d_raw, d_mask, d_shown, stride, stream = ring.run_dev(s)
            chunks = [self.reader.chunk(i) for i in range(f, f + k)]
            sent += self.decoder.decode_run_dev(chunks, d_raw, d_mask, d_shown, stride, ring.W,
                                                int(np.floor(self.threshold)), None, stream)   # frame > t for integer frames
            ring.mirror(mirror)
        return sent

    def close(self):
        d, self.decoder = getattr(self, "decoder", None), None
        if d is not None:
            d.close()
        r, self.reader = getattr(self, "reader", None), None
        if r is not None:
            r.close()
