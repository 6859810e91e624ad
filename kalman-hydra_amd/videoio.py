"""Video and image output of the tracker: the library's AVI container, PNG files and the flow tool's preview.

``AviWriter`` wraps hm_avi_open / hm_avi_write / hm_avi_close (uncompressed 24-bit AVI at the reference's 20 frames/s,
src/optical_flow_ext.cpp:358; OpenDML continuation past 1 GiB) and, with codec="mjpeg", hm_avi_open_codec /
hm_avi_write_chunk around the device's JPEG encoder (hm_mjpeg_*); ``read_avi`` gives the frames of either back.  Frames are (H, W, 3) uint8 in B, G, R order, rows top
to bottom, as every view of ``Renderer.view`` is.
"""
import ctypes

import numpy as np

from . import _lib

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
            from .pipeline import DeviceBuffer
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
    """A (H, W, 3) B G R or (H, W) gray uint8 image as PNG (PIL, which pipeline.load_video uses for TIFF)."""
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
