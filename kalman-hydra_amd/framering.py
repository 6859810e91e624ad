"""``FrameRing``: the frames of a source in a ring of device slots, uploaded on a copy stream ahead of their use."""
import ctypes
import threading

import numpy as np

from . import _lib
from .devbuf import DeviceBuffer


def ring_runs(f0, f1, R, extra, run):
    """The frames f0 .. f1 - 1 of a ring of R slots cut into runs of at most `run` frames that do not cross the end of the
    ring -> [(f, k, s, mirror)]: k frames from frame f on land in the slots s .. s + k - 1 (s = f % R); `mirror` is the
    range of those slots below `extra`, which are copied behind the ring (slot R + t for t) once the run has landed."""
    runs, f = [], int(f0)
    while f < f1:
        s = f % R
        k = min(run, f1 - f, R - s)
        runs.append((f, k, s, range(s, min(s + k, extra))))
        f += k
    return runs


class FrameRing:
    """Ring of frame slots in HBM fed from a frame source over a copy stream.

    Frame f lives in slot f % R of each plane (raw frame, mask, and -- when the source has one -- the frame
    shown to the filter).  A flow series reads nb + 1 consecutive frames through one base pointer, so the first
    `extra` slots are mirrored behind the ring (frames that land in slots 0 .. extra-1 are copied twice): any run of up to extra + 1
    frames is contiguous.  Host frames are staged in page-locked memory and copied with hipMemcpyAsync on a
    stream of their own; `sync()` makes what has been queued visible to the other streams (the caller waits
    before it launches work that reads them).  With slots >= len(source) nothing is ever overwritten (the
    resident mode)."""

    def __init__(self, source, slots, extra, device, with_observed):
        self.src, self.device = source, int(device)
        self.F = len(source)
        self.H, self.W = source.shape
        self.n = self.H * self.W
        self.R = int(min(slots, self.F))
        self.extra = int(extra) if self.R < self.F else 0
        total = self.R + self.extra
        self.d_video = DeviceBuffer(total * self.n, device)
        self.d_masks = DeviceBuffer(total * self.n, device)
        self.d_observed = DeviceBuffer(total * self.n, device) if with_observed else self.d_video
        self.planes = 3 if with_observed else 2
        self._lock = threading.RLock()
        self._stream = _lib.c_vp()
        _lib.check(_lib.lib().hm_copy_stream_create(self.device, ctypes.byref(self._stream)), "hm_copy_stream_create")
        self._nstage = max(2, self.extra + 2) if self.R < self.F else min(self.F, 16)                    # frames staged between two waits for the copy stream
        self._stage, self._stage_np = None, None
        if not hasattr(source, "upload_run"):                    # (a source that fills the slots itself stages nothing here)
            self._stage = _lib.c_vp()
            _lib.check(_lib.lib().hm_host_alloc(self._nstage * self.planes * self.n, ctypes.byref(self._stage)), "hm_host_alloc")
            self._stage_np = np.ctypeslib.as_array(ctypes.cast(self._stage, ctypes.POINTER(ctypes.c_uint8)),
                                                   shape=(self._nstage, self.planes, self.n))
        self._staged = 0
        self.synced_hi = 0
        _lib.register(self, 4)
        self.lo = self.hi = 0                                    # frames [lo, hi) are in the ring (queued or there)
        self.bytes_uploaded = 0
        self._fence = None       # a reader queued on another stream: the copy stream waits for it before it overwrites a slot

    def reset(self, first):
        with self._lock:
            self.sync()
            self.lo = self.hi = self.synced_hi = int(first)

    def ptr(self, plane, f):
        """Device address of frame f in plane 0 (raw), 1 (mask) or 2 (shown to the filter)."""
        buf = (self.d_video, self.d_masks, self.d_observed)[plane]
        return buf.ptr + (f % self.R) * self.n

    def fence_after(self, fence):
        """fence(copy stream) makes the copy stream wait on the device for a read of a frame just queued elsewhere (the
        body readout's warp): it is called before the next upload, whichever frame and slot that is (after reset() the
        first uploads may go into slots of frames such a read still has to see)."""
        with self._lock:
            self._fence = fence

    def run_ptr(self, f):
        """Base address of the raw frames f, f + 1, ... (contiguous for extra + 1 frames)."""
        return self.d_video.ptr + (f % self.R) * self.n

    def runs(self, f0, f1, run):
        """ring_runs of this ring: the frames f0 .. f1 - 1 in runs of at most `run` consecutive slots"""
        return ring_runs(f0, f1, self.R, self.extra, run)

    def run_dev(self, s):
        """A run that starts in slot s -> (device address of its raw frames, of its masks, of its shown frames or None
        when the ring has no such plane; bytes from one frame to the next; the copy stream to queue the run on)."""
        off = s * self.n
        return (self.d_video.ptr + off, self.d_masks.ptr + off, self.d_observed.ptr + off if self.planes == 3 else None,
                self.n, self._stream)

    def mirror(self, slots):
        """Queue the device-to-device copies of `slots` (a run's slots below `extra`) behind the ring, on the copy stream."""
        L, n = _lib.lib(), self.n
        for t in slots:
            for buf in (self.d_video, self.d_masks) + ((self.d_observed,) if self.planes == 3 else ()):
                _lib.check(L.hm_dev_copy_async(self.device, buf.ptr + (self.R + t) * n, buf.ptr + t * n, n, self._stream),
                           "hm_dev_copy_async")

    def ensure(self, hi, keep_from):
        """Queue the uploads of the frames up to hi - 1; frames before keep_from may be overwritten."""
        L = _lib.lib()
        with self._lock:
            hi = min(int(hi), self.F)
            if hi - keep_from > self.R:
                raise RuntimeError("frame ring too small: frames %d..%d asked for, %d slots" % (keep_from, hi - 1, self.R))
            if self.hi < hi and hasattr(self.src, "upload_run"):  # a source that fills the slots on the device (AviSource)
                if self._fence is not None:
                    self._fence(self._stream)
                    self._fence = None
                self.bytes_uploaded += self.src.upload_run(self.hi, hi, self)
                self.hi = hi
            while self.hi < hi:
                f = self.hi
                if self._staged == self._nstage:                  # the staging block is full: wait for its copies
                    _lib.check(L.hm_copy_stream_sync(self.device, self._stream), "hm_copy_stream_sync")
                    self._staged = 0
                if self._fence is not None:
                    self._fence(self._stream)
                    self._fence = None
                st = self._stage_np[self._staged]
                fr, mk, ob = self.src.frame_at(f)
                parts = [(self.d_video, fr), (self.d_masks, mk)]
                if self.planes == 3:
                    parts.append((self.d_observed, fr if ob is None else ob))
                s = f % self.R
                for i, (buf, a) in enumerate(parts):
                    st[i][:] = np.asarray(a, np.uint8).reshape(-1)
                    src = self._stage.value + (self._staged * self.planes + i) * self.n
                    _lib.check(L.hm_dev_upload_async(self.device, buf.ptr + s * self.n, src, self.n, self._stream), "hm_dev_upload_async")
                    if s < self.extra:                            # the mirror behind the ring
                        _lib.check(L.hm_dev_upload_async(self.device, buf.ptr + (self.R + s) * self.n, src, self.n, self._stream),
                                   "hm_dev_upload_async")
                    self.bytes_uploaded += self.n
                self._staged += 1
                self.hi = f + 1
            self.lo = max(self.lo, self.hi - self.R)

    def sync(self):
        with self._lock:
            hi = self.hi
            _lib.check(_lib.lib().hm_copy_stream_sync(self.device, self._stream), "hm_copy_stream_sync")
            self._staged = 0
            self.synced_hi = hi              # frames below this are in device memory for certain

    def close(self):
        if getattr(self, "_stream", None) is not None and self._stream:
            _lib.lib().hm_copy_stream_destroy(self.device, self._stream)
            self._stream = None
        if getattr(self, "_stage", None) is not None and self._stage:
            self._stage_np = None
            _lib.lib().hm_host_free(self._stage)
            self._stage = None
        for b in {id(b): b for b in (self.d_video, self.d_masks, self.d_observed)}.values():
            b.close()
