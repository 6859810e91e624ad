"""What leaves the device frame by frame without the frame loop waiting for it: ``SlotRing`` (device slots, a copy stream,
a writer thread), the overlay video ``VideoTap`` on it, and ``write_painted_video`` for the videos of a finished track.
(body.BodyTap is the readout's SlotRing.)"""
import ctypes
import queue
import threading

import numpy as np

from . import _lib
from .devbuf import DeviceBuffer
from .videoio import AviWriter, MjpegSlots


class SlotRing:
    """What VideoTap and body.BodyTap share: a ring of `slots` device slots that the caller's thread fills by queuing work
    on the device, a copy stream that waits for that work and brings a slot's results into page-locked memory, and a
    writer thread that waits for the copy stream and takes the slots in order.  A slot is `dev_bytes` of device memory
    (with `encoder`, an MjpegEncoder: plus room for a stream, which videoio.MjpegSlots lands) and `pin_bytes` of a
    page-locked block (0: none).  A subclass queues into a slot between ``_take`` and ``_submit`` (``_give_back`` when
    queuing failed) and supplies ``_written(item)``, the writer thread's half.  An exception the writer thread meets is
    kept: the slots behind it are skipped, and the next ``_take``, ``drain`` or ``close`` raises it."""

    def __init__(self, name, device, slots, dev_bytes, pin_bytes, encoder=None):
        self.device, self.slots = int(device), int(slots)
        L = _lib.lib()
        self._stream = _lib.c_vp()
        _lib.check(L.hm_copy_stream_create(self.device, ctypes.byref(self._stream)), "hm_copy_stream_create")
        self._mj = None
        if encoder is not None:
            self._mj = MjpegSlots(encoder, self.slots, device)
        self._pin, self._pin_bytes = _lib.c_vp(), int(pin_bytes)
        if self._pin_bytes:
            _lib.check(L.hm_host_alloc(self.slots * self._pin_bytes, ctypes.byref(self._pin)), "hm_host_alloc")
        self._dev = [DeviceBuffer(dev_bytes + (self._mj.cap if self._mj is not None else 0), device) for _ in range(self.slots)]
        self._free = threading.Semaphore(self.slots)
        self._q = queue.Queue()
        self._next = 0
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._write_loop, name=name, daemon=True)
        self._thread.start()
        _lib.register(self, 0)

    def _take(self):
        """-> (s, device address of slot s): the next slot, once the writer has taken what was in it"""
        if self._error is not None:
            raise self._error
        self._free.acquire()
        s = self._next % self.slots
        self._next += 1
        return s, self._dev[s].ptr

    def _give_back(self):
        """the slot just taken, when queuing into it failed"""
        self._next -= 1
        self._free.release()

    def _submit(self, item):
        """hand a filled slot to the writer thread: _written(item) runs once the copy stream has passed"""
        self._q.put(item)

    def _pinned(self, s):
        return self._pin.value + s * self._pin_bytes

    def _download(self, s, nbytes):
        """queue the copy of the first nbytes of device slot s into its page-locked slot"""
        _lib.check(_lib.lib().hm_dev_download_async(self.device, self._pinned(s), self._dev[s].ptr, nbytes, self._stream),
                   "hm_dev_download_async")

    def _write_loop(self):
        L = _lib.lib()
        while True:
            item = self._q.get()
            if item is None:
                return
            try:
                if self._error is None:
                    _lib.check(L.hm_copy_stream_sync(self.device, self._stream), "hm_copy_stream_sync")
                    self._written(item)
            except Exception as e:          # noqa: BLE001 -- reported by the next frame() / drain() / close()
                self._error = e
            finally:
                self._free.release()

    def drain(self):
        """Wait until every slot queued so far has been taken (a video's frames are in the file)."""
        for _ in range(self.slots):
            self._free.acquire()
        for _ in range(self.slots):
            self._free.release()
        if self._error is not None:
            raise self._error

    def close(self):
        if self._closed:
            return
        self._closed = True
        try:
            self._q.put(None)
            self._thread.join()
        finally:
            L = _lib.lib()
            if self._stream:
                L.hm_copy_stream_destroy(self.device, self._stream)
                self._stream = None
            for b in self._dev:
                b.close()
            if self._mj is not None:
                self._mj.close()
            if self._pin:
                L.hm_host_free(self._pin)
                self._pin = None
        if self._error is not None:
            raise self._error


class VideoTap(SlotRing):
    """The overlay video of a pipeline run (FlowEKFPipeline.run(video=...)): after every step the overlay at the state the
    frame ended with is queued on the device (hm_view_dev, on the filter's stream, into a ring of device slots), copied
    into page-locked memory on a copy stream of its own, and appended to the AviWriter by a writer thread.  The filter's
    launches and the flow series never wait for the disk; only when all `slots` are still waiting to be written does the
    next frame wait for the oldest.  close() drains the writer.

    With an MJPEG writer (AviWriter(codec="mjpeg")) the frame never leaves the device: the writer's encoder is queued
    behind the view on the same stream (write into the slot's stream area, size word into page-locked memory), and the
    writer thread, once the stream has passed, copies exactly the stream's bytes (videoio.MjpegSlots) and appends them."""

    def __init__(self, renderer, writer, device=0, slots=4):
        self.r, self.writer = renderer, writer
        self.n = 3 * renderer.nx * renderer.ny
        if (writer.width, writer.height) != (renderer.nx, renderer.ny):
            raise ValueError("a %dx%d video for %dx%d frames" % (writer.width, writer.height, renderer.nx, renderer.ny))
        mjpeg = getattr(writer, "mjpeg", False)
        if mjpeg and writer.channels != 3:
            raise ValueError("VideoTap: the views are B G R, the MJPEG video has %d channel" % writer.channels)
        # (a raw frame is downloaded whole; an MJPEG frame stays in its slot with the stream the encoder makes of it behind it)
        SlotRing.__init__(self, "hydra_mi-video", device, slots, self.n, 0 if mjpeg else self.n, writer.encoder if mjpeg else None)

    @property
    def bus_bytes(self):
        """Bytes of video copied from the device so far: whole frames of a raw video, the streams (rounded up to
        videoio.MJPEG_GRANULE) of an MJPEG one; the frames still in the ring are counted when they are written."""
        return self._mj.copied if self._mj is not None else self.n * self.writer.frames

    def frame(self, X):
        """Queue the overlay of state X as the next video frame."""
        self.push(lambda d, stream: self.r.view_dev(X, "overlay", d, stream))

    def push(self, queue_view):
        """Queue the next video frame: queue_view(d_out, stream) queues a view of the renderer into the device slot d_out
        (W*H*3 bytes) and makes `stream` wait for it, as Renderer.view_dev does."""
        s, d = self._take()
        try:
            queue_view(d, self._stream)
        except Exception:
            self._give_back()
            raise
        if self._mj is not None:
            self.writer.encoder.encode_dev(d, d + self.n, self._mj.cap, self._mj.size_word(s), self._stream)
        else:
            self._download(s, self.n)
        self._submit(s)

    def _written(self, s):
        if self._mj is not None:
            self._mj.finish(s, self._dev[s].ptr + self.n, self.writer)
        else:
            self.writer.write_ptr(self._pinned(s))


def write_painted_video(r, states, source, path, paint, fps=20, video_opts=None, done=None):
    """The video of a finished track that strain.write_video and cellview.write_video write: for every state k, frame k of
    `source` (``frame_at(k)`` -> raw frame, ...; or an array (frames, H, W) uint8) is uploaded into a device buffer and
    ``paint(k, X, d_frame, d_out, stream)`` queues a view of renderer `r` of it behind the upload, into a slot of a
    VideoTap whose writer thread appends it to the AVI `path`: the disk is not waited for.  Tap, buffers and writer are
    closed in that order whatever happens, then done() is called.  -> frames written."""
    frame_at = source.frame_at if hasattr(source, "frame_at") else (lambda k: (source[k],))
    writer = AviWriter(path, r.nx, r.ny, fps=fps, **(video_opts or {}))
    tap = VideoTap(r, writer)
    d_frames = [DeviceBuffer(r.nx * r.ny, tap.device) for _ in range(tap.slots)]     # a frame is read when its view runs
    try:
        for k in range(len(states)):
            X = np.asarray(states[k], np.float64).reshape(-1)
            img = np.ascontiguousarray(np.asarray(frame_at(k)[0], np.uint8).reshape(r.ny, r.nx))

            def queue_view(d_out, stream, k=k, X=X, img=img):
                # the buffer of this frame is free: the view that read the frame uploaded there `slots` frames ago has
                # been waited for by the writer.  upload() waits for the copy; the view is queued behind it.
                d = d_frames[k % tap.slots]
                d.upload(img)
                paint(k, X, d.ptr, d_out, stream)
            tap.push(queue_view)
    finally:
        try:
            tap.close()
        finally:
            for b in d_frames:
                b.close()
            writer.close()
            if done is not None:
                done()
    return writer.frames
