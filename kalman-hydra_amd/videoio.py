"""Video and image output of the tracker: the library's AVI container, PNG files and the flow tool's preview.

``AviWriter`` wraps hm_avi_open / hm_avi_write / hm_avi_close (uncompressed 24-bit AVI at the reference's 20 frames/s,
src/optical_flow_ext.cpp:358; OpenDML continuation past 1 GiB).  Frames are (H, W, 3) uint8 in B, G, R order, rows top
to bottom, as every view of ``Renderer.view`` is.
"""
import ctypes

import numpy as np

from . import _lib

#: view names of Renderer.view -> the view ids of hm_view (include/hydra_mi.h)
VIEWS = {"raw": 0, "overlay": 1, "texture": 2, "mask": 3, "flowx": 4, "flowy": 5}


class AviWriter:
    """with AviWriter("out.avi", W, H) as v: v.write(bgr) ...   (riff_limit: bytes per RIFF, 0 = 1 GiB)"""

    def __init__(self, path, width, height, fps=20, riff_limit=0):
        self.path, self.width, self.height = str(path), int(width), int(height)
        self.frames = 0
        self._h = None
        h = _lib.c_vp()
        _lib.check(_lib.lib().hm_avi_open(self.path.encode(), self.width, self.height, int(fps), int(riff_limit),
                                          ctypes.byref(h)), "hm_avi_open")
        self._h = h
        _lib.register(self, 4)

    def write(self, bgr):
        if self._h is None:
            raise ValueError("write to a closed AviWriter")
        a = np.ascontiguousarray(bgr, np.uint8)
        if a.shape != (self.height, self.width, 3):
            raise ValueError("frame of shape %r for a %dx%d video" % (a.shape, self.width, self.height))
        _lib.check(_lib.lib().hm_avi_write(self._h, _lib.ptr(a)), "hm_avi_write")
        self.frames += 1

    def write_ptr(self, address):
        """Append the frame at a host address (H x W x 3 bytes, e.g. a page-locked staging buffer)."""
        _lib.check(_lib.lib().hm_avi_write(self._h, ctypes.c_void_p(int(address))), "hm_avi_write")
        self.frames += 1

    def close(self):
        h, self._h = self._h, None
        if h is not None:
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
