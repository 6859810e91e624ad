"""In-process flow -> EKF streaming.

The reference computes its optical flow in a separate executable and hands it to the tracker
through files (reference README.md:26-31; ``gen_synthetic.py:41-42`` shells out to
``./bin/optical_flow_ext``); the tracker's frame loop then reads one flow file per frame
(reference run_kalmanfilter.py:78-89).  Here both halves run in one process on one GPU:

* the frames (and masks) are read from a frame source (``sources``) one at a time, as the reference's loop does
  (run_kalmanfilter.py:78-89), and uploaded on a copy stream into a ring of frame slots in HBM (``framering``): the
  frames of the next flow series go up while the current series runs (``resident=True`` uploads the
  whole video once instead -- same results, only useful for comparisons);
* the Brox flow of consecutive frame pairs does not depend on the filter, so it is computed ahead
  of it, in launch series of 1, 2, 4, ... up to ``flow_batch`` pairs on the flow handle's own HIP
  stream (a single pair is launch-latency bound; a series amortises the ~900 launches over its
  pairs), double buffered: while the filter works through the pairs of one series, the next series
  runs beside it.  The series are queued from a helper thread -- the C calls drop the GIL -- so the
  filter's thread does not pay for their launches.  How many pairs a series gets is ``flowplan.SeriesPlanner``'s
  decision; this module launches, waits and keeps the books;
* a frame's flow planes are handed to the filter where they are, in device memory
  (``renderer.DeviceObservation`` -> ``hm_set_observation_dev``).

The names of ``sources``, ``devbuf``, ``framering`` and ``taps`` are importable from here as well.
"""
import dataclasses
import gc
import threading
import time

import numpy as np

from . import _lib
from . import brox as _brox
from .body import BodyTap
from .devbuf import DeviceBuffer
from .flowplan import SeriesPlanner
from .framering import FrameRing, ring_runs  # noqa: F401
from .renderer import DeviceObservation
from .sources import ArraySource, VideoStream, load_video, threshold_mask, to_gray  # noqa: F401
from .taps import SlotRing, VideoTap, write_painted_video  # noqa: F401


@dataclasses.dataclass
class Series:
    """A flow series in flight: the pairs lo .. hi - 1, computed into flow buffer `buf` on flow handle `handle`, queued by
    `thread` from `t0` on.  `alone`: nothing runs beside it, so launch -> completion measures a series of that size;
    `opening`: the first series of a phase with two handles; `joined`: it has been waited for already."""
    lo: int
    hi: int
    buf: int
    handle: int
    thread: threading.Thread
    t0: float
    alone: bool
    opening: bool = False
    joined: bool = False


class FlowEKFPipeline:
    """Brox flow of the coming frames overlapped with the filter on the current one.

        pipe = FlowEKFPipeline(kf, video, masks)        # kf: any kalman.*KalmanFilter on the same device
        for k in range(len(video) - 1):
            e = pipe.step(k)                            # frame k+1: flow of (k, k+1), then kf.compute

    ``video``: a frame source (``VideoStream``, ``ArraySource``: ``len()``, ``.shape``, ``.frame_at(f)`` ->
    raw frame, mask, frame shown to the filter or None) or, with ``masks``, (frames, H, W) uint8 host arrays
    (masks in {0,1}).  Frames are read from it one by one and uploaded on a copy stream into a ring of
    ``3 flow_batch + 3`` frame slots (``FrameRing``): the upload of the frames of the next flow series is
    queued right after the launches of the current one.  ``resident=True`` uploads the whole video at
    construction instead.  The flow parameters default to the reference's (src/optical_flow_ext.cpp:453-488).
    The numbers are those of ``bf.calc(video[k], video[k+1])`` followed by
    ``kf.compute(video[k+1], flow, masks[k+1])``: a pair's flow does not depend on the series it is computed in.
    """

    def __init__(self, kf, video, masks=None, flow_batch=8, device=0, brox_params=None, sor_threads=0, maskflow=True,
                 observed=None, return_flow=False, cu_reserve=32, concurrent_series=True, resident=False):
        """return_flow: whether step() brings the rendered flow planes of every frame to the host, as
        KalmanFilter.compute does for the reference's callers (8 MB per 1024^2 frame); a frame loop that
        looks at the error sums and the state only (reference run_kalmanfilter.py:78-89 ignores the return
        value altogether) leaves them on the device.
        observed: the frames the filter is shown, when they differ from the ones the flow is computed on
        (the reference CLI tracks the background-subtracted frame, renderer.py:770-773, while its flow tool
        works on the raw video); default: the video itself."""
        if hasattr(video, "frame_at"):
            if masks is not None or observed is not None:
                raise ValueError("a frame source brings its own masks / observed frames")
            source = video
            with_observed = source.frame_at(0)[2] is not None
        else:
            source = ArraySource(video, masks, observed)
            with_observed = observed is not None
        self.source = source
        self.kf, self.maskflow = kf, maskflow
        kf.return_flow = bool(return_flow)
        self.F = len(source)
        self.H, self.W = source.shape
        self.B = max(1, int(flow_batch))
        self.device = int(device)
        n = self.H * self.W
        self._px = n
        # the filter works on frame k + 1 while up to two series (of at most B pairs each, B + 1 frames) are in
        # flight or ready ahead of it and the next one's frames are being uploaded
        self.ring = FrameRing(source, self.F if resident else 3 * self.B + 3, self.B, device, with_observed)
        if resident:
            self.ring.ensure(self.F, 0)
            self.ring.sync()
        self.resident = bool(resident)
        _lib.register(self, 0)
        self.d_u = DeviceBuffer(3 * self.B * n * 4, device)          # flow planes: one buffer in use, two being filled
        self.d_v = DeviceBuffer(3 * self.B * n * 4, device)
        # concurrent_series: two flow handles (streams), two series in flight at a time -- while the filter works through
        # the pairs of one series the next TWO run beside it, each on a handle of its own.  A phase starts with one pair
        # (the whole chip) and a second series beside it, and the series grow as the planner's next_concurrent sizes them
        # (1, 2, 2, 3, 5, 8 at 1024^2 / 201 vertices): the filter waits ~7 ms for its first pair instead of ~13 for a first
        # series of five, and once the series are full it does not wait at their boundaries any more (one series at a
        # time: 0.3 to 2.7 ms at every boundary, profiles/r04_frame_trace_64.txt).  Driver's bench, 20 frames: 267-270
        # against 261-264 frames/s, 64 frames: 331-333 against 322-325.  (Round 2 measured this mode at 182 against 214
        # frames/s: before the filter's streams had their priority and the flow's its CU mask.)  The results are the same
        # bits either way (tools/determinism_check.py).
        def make_handle():
            bf = _brox.BroxOpticalFlow(self.W, self.H, max_batch=self.B, device=device, **(brox_params or {}))
            bf.tune("sor_threads", sor_threads)         # 0: chosen per series (1024 for one or two pairs, else 512)
            if cu_reserve:
                # the flow streams leave some compute units alone: the filter's short dependent launches find room at
                # once while a series fills the rest (bench: 250 -> 254 frames/s with 32 of 256 reserved)
                bf.tune("cu_reserve", int(cu_reserve))
            return bf
        self._make_handle = make_handle
        self.cu_reserve = int(cu_reserve or 0)
        self.concurrent_series = bool(concurrent_series)
        self.bfs = [make_handle() for _ in range(2 if concurrent_series else 1)]
        self.bf = self.bfs[0]
        # split_start: a phase whose series times are known (an earlier phase measured them) starts with TWO series side by
        # side, on two handles -- a short one (two pairs) so that the filter, which has nothing to do until the first
        # flow arrives, starts soon, and the one the planner's first() sizes behind it.  A lone short series leaves most of
        # the chip idle (it is a chain of ~500 short launches), so the second should cost the first little.  After that one
        # series at a time, as before.  The second handle is created when it is first needed.  Measured at 1024^2 / 201
        # vertices, 20 frames: 212 frames/s against 229 without (the two series slow each other and the filter's first
        # frames more than the earlier start gains: 0.92 instead of 0.73 ms per frame of waiting for flow); 64 frames: 286
        # against 292.  Again at the end of round 3 (calibrated series sizes, the second handle created before the timed region):
        # 249.5 against 254.4 frames/s at 20 frames, three runs each.  Off by default; the results are the same bits either way.
        self.split_start = False
        self.t_flow = self.t_ekf = 0.0
        self.iters = 0
        self.frame_done = []             # perf_counter() at the end of every step (steady-state rates)
        self.profile_full, self.profiled_pairs = False, 0    # set profile_full: the next series of flow_batch pairs is profiled
        self.profile_min_pairs = None    # ... or of at least this many (a series that runs beside the filter, not a phase's first)
        self.profiled_handle = None
        self.trace = None                # callable(str) for per-frame scheduling messages
        # pairs [lo, hi) of `ready` have their flow in buffer `buf`; the series in `_flying` (Series, oldest first) are
        # being computed while the filter works on `ready`
        self._ready, self._buf, self._flying, self._thread_exc = (0, 0), 0, [], None
        self._end = self.F - 1
        self._cursor = 0                 # the oldest frame still needed (the pair the filter is at)
        self.plan = SeriesPlanner()      # sizes the series from measured series / frame times; only this thread uses it
        self.gc_freeze = True            # see run()

    # the planner's knobs that callers set on the pipeline
    first_series = property(lambda self: self.plan.first_series, lambda self, v: setattr(self.plan, "first_series", v))
    model_ramp = property(lambda self: self.plan.model_ramp, lambda self, v: setattr(self.plan, "model_ramp", v))

    # -- flow series ---------------------------------------------------------------------------------
    def _phase_start(self):
        """nothing is ready and nothing in flight: the next series is the first of a phase"""
        return not self._flying and self._ready[0] == self._ready[1]

    def _launch(self, k, end, most, alone=None, whole=None, delay=0.0):
        """Queue the series of pairs k .. k + nb - 1 on a handle and a buffer that are free (`delay`: seconds the helper
        thread waits before it queues the launches) -> its Series."""
        nb = min(most, end - k)
        busy_h = {s.handle for s in self._flying}
        busy_b = {s.buf for s in self._flying} | {self._buf}
        h = next(i for i in range(len(self.bfs)) if i not in busy_h)
        buf = next(i for i in range(3) if i not in busy_b)
        first = self._phase_start() if alone is None else alone      # the first series of a phase: nothing runs beside it
        measured = first and not self.concurrent_series              # (with two handles the second series starts beside the first)
        # the read-ahead is one series: sized here, so that the planner is only ever used from this thread
        ahead = self.plan.next(nb, self.B)
        t = threading.Thread(target=self._queue_series,
                             args=(self.bfs[h], buf, k, nb, first, first if whole is None else whole, delay, ahead))
        s = Series(k, k + nb, buf, h, t, time.perf_counter(), measured)
        t.start()
        self._flying.append(s)
        return s

    def _queue_series(self, bf, buf, k, nb, first, whole, delay, ahead):
        """The helper thread of a series: wait for the uploads of its frames, queue its launches on `bf`, then queue the
        uploads of the `ahead` frames behind it."""
        n, B = self._px, self.B
        try:
            if delay > 0:
                time.sleep(delay)
            self._switch_profiling(bf, nb, first)
            # frames k .. k + nb: normally queued for upload when the previous series was launched; the copy
            # stream is waited for here, on the helper thread, before the flow stream is given work that reads them
            self.ring.ensure(k + nb + 1, self._cursor)
            self.ring.sync()
            if self.cu_reserve:
                # a series the filter waits for with nothing to do (the first of a phase) gets the whole chip, the
                # others leave `cu_reserve` compute units to the filter
                bf.tune("whole_chip", 1 if whole else 0)
            bf.calc_dev(nb, self.ring.run_ptr(k), self.ring.run_ptr(k) + n,
                        self.d_u.ptr + buf * B * n * 4, self.d_v.ptr + buf * B * n * 4)
            # ... and while this series runs, the frames of the next one go up (reference run_kalmanfilter.py:78-89
            # reads one frame per iteration; here the read-ahead is one series)
            nxt = min(self._end, k + nb + ahead)
            self.ring.ensure(min(nxt + 1, self._cursor + self.ring.R), self._cursor)
        except Exception as exc:                    # noqa: BLE001 -- re-raised by the thread that waits
            self._thread_exc = exc

    def _switch_profiling(self, bf, nb, first):
        """hm_brox_profile around the first series of flow_batch (profile_min_pairs) pairs after profile_full was set, not a
        phase's first; off again with the next series on that handle (the totals stay readable: hm_brox_profile_read)"""
        if self.profile_full and self.profiled_pairs == 0 and nb >= (self.profile_min_pairs or self.B) and not first:
            bf.profile(True)
            self.profiled_pairs, self.profiled_handle, self.profile_full = nb, bf, False
        elif bf is self.profiled_handle:
            bf.profile(False)

    def _wait(self, s):
        s.thread.join()
        if self._thread_exc is not None:
            exc, self._thread_exc = self._thread_exc, None
            raise exc
        t1 = time.perf_counter()
        self.bfs[s.handle].sync()
        t2 = time.perf_counter()
        self.plan.note_series(s.hi - s.lo, t2 - s.t0, s.alone, t2 - t1)
        s.joined = True

    def flow_sync(self):
        """Wait for every series in flight (their results stay where they are)."""
        for s in self._flying:
            if not s.joined:
                self._wait(s)

    def calibrate(self, first=0):
        """What a flow series of 2 and of B pairs takes with nothing beside it (seconds, kept by the planner for its
        first / next): three calls on the frames first .. first + B, the first of which also absorbs the
        one-time costs of a handle's first launches (measured as part of a phase's first series they made a series of 2
        pairs look like 9.7 instead of 6.8 ms, and every series after it was sized from that).  ~30 ms at 1024^2, once
        per pipeline, at the start of its first phase."""
        nb = min(self.B, self.F - 1 - first)
        if nb < 2:
            return
        n = self._px
        self.ring.ensure(first + nb + 1, first)
        self.ring.sync()
        bf = self.bfs[0]
        if self.cu_reserve:
            bf.tune("whole_chip", 1)
        for pairs, keep in ((2, False), (2, True), (nb, True)):
            t0 = time.perf_counter()
            bf.calc_dev(pairs, self.ring.run_ptr(first), self.ring.run_ptr(first) + n, self.d_u.ptr, self.d_v.ptr)
            bf.sync()
            if keep:
                self.plan.note_series(pairs, time.perf_counter() - t0)
        self.plan.calibrated = True

    def begin(self, first=0, end=None):
        """Start a phase: the pairs first .. end-1 will be asked for in order."""
        self.flow_sync()
        self._flying = []
        self._end = self.F - 1 if end is None else min(int(end), self.F - 1)
        self._ready = (first, first)
        self._cursor = first
        self.plan.flow_late = False
        self._discard_prepared_mask()
        if not self.resident:
            self.ring.reset(first)               # nothing of an earlier phase is assumed to be in the ring
        if self.plan.model_ramp and self.plan.adaptive_first and not self.plan.calibrated:
            self.calibrate(first)                # (the frames it uploads are the first ones of this phase: they stay)

    def _discard_prepared_mask(self):
        """The filter compares a prepared outline with the next observation's mask by address only (hm_prepare_mask):
        a new phase or random access may put another frame's mask in the slot of the one prepared, and a pipeline made
        after this one may be given the same memory."""
        r = getattr(getattr(self.kf, "state", None), "renderer", None)
        if r is not None and getattr(r, "_h", None) and hasattr(r, "prepare_mask"):
            r.prepare_mask(None)

    def _open_split(self):
        """split_start, at the very start of a phase whose series times are known: two series side by side, two pairs and
        the planner's first series behind them -> whether it applied."""
        if not (self._phase_start() and self.split_start and not self.concurrent_series and self.plan.model() is not None
                and self.B >= 3 and self._end - self._ready[1] >= 4 and not self.first_series):
            return False
        if len(self.bfs) < 2:
            self.bfs.append(self._make_handle())
        k = self._ready[1]
        n1 = max(3, self.plan.first(self.B, False))
        self._launch(k, self._end, 2, alone=False, whole=True)
        self._launch(k + 2, self._end, n1, alone=False, whole=True)
        return True

    def _top_up(self):
        """Keep as many series in flight as there are handles (one unless concurrent_series)."""
        if self._open_split():
            return
        plan, B = self.plan, self.B
        limit = len(self.bfs) if self.concurrent_series else 1
        while len(self._flying) < limit:
            last = self._flying[-1] if self._flying else None
            nxt = last.hi if last else self._ready[1]
            if nxt >= self._end:
                return
            size = (last.hi - last.lo) if last else (self._ready[1] - self._ready[0])
            most = plan.next(size, B) if size else plan.first(B, self.concurrent_series)
            delay = 0.0
            if self.concurrent_series and size:
                flying = [(s.lo, s.hi, s.t0) for s in self._flying]
                most = plan.next_concurrent(time.perf_counter(), self._ready, self._cursor, flying, B, self.trace) or most
                if last is not None and self._ready[0] == self._ready[1] and last.opening:
                    delay = plan.opening_delay()         # the series beside the opening one
            opening = not last and self._ready[0] == self._ready[1]
            s = self._launch(nxt, self._end, most, delay=delay)
            s.opening = opening

    def flow_ready(self, k):
        """Make the flow of pair (k, k+1) available -> (device pointer of u, of v)."""
        if not (0 <= k < self.F - 1):
            raise IndexError("pair %d of a %d-frame video" % (k, self.F))
        if not (self._ready[0] <= k < self._ready[1]):
            if k != self._ready[1] or (self._flying and self._flying[0].lo != k):
                self.begin(k, max(self._end, k + 1))     # random access: start over from k
            elif k >= self._end:
                self._end = min(self.F - 1, k + 1)       # past the end of the phase run() announced: go on pair by pair
            self._cursor = k
            self._top_up()
            s = self._flying.pop(0)
            t_w = time.perf_counter()
            opening = self._ready[0] == self._ready[1]             # the first series of a phase is always waited for
            if not s.joined:
                self._wait(s)
            # (late: the filter waited for this series although it had others to work through before)
            self.plan.note_wait(opening, time.perf_counter() - t_w)
            self._ready, self._buf = (s.lo, s.hi), s.buf
            self._top_up()
        self._cursor = k
        i = k - self._ready[0]
        off = (self._buf * self.B + i) * self._px * 4
        return self.d_u.ptr + off, self.d_v.ptr + off

    def flow_host(self, k):
        """The flow of pair (k, k+1) as an (H, W, 2) host array (for writing .mat files, tests)."""
        pu, pv = self.flow_ready(k)
        out = np.empty((2, self.H, self.W), np.float32)
        _lib.check(_lib.lib().hm_dev_download(self.device, _lib.ptr(out[0]), pu, self._px * 4), "hm_dev_download")
        _lib.check(_lib.lib().hm_dev_download(self.device, _lib.ptr(out[1]), pv, self._px * 4), "hm_dev_download")
        return np.dstack((out[0], out[1]))

    # -- the frame loop of reference run_kalmanfilter.py:78-89 ----------------------------------------------
    def step(self, k):
        """Frame k+1: flow of (k, k+1) -- usually already there -- then kf.compute on it."""
        if not (0 <= k < self.F - 1):
            raise IndexError("pair %d of a %d-frame video" % (k, self.F))
        t0 = time.perf_counter()
        pu, pv = self.flow_ready(k)
        t1 = time.perf_counter()
        # the next frame's mask, when its upload has been waited for already (every flow series is launched behind a wait
        # for the uploads of its frames): the filter queues that mask's outline a frame ahead
        # for frame k + 2, not on the last step of a phase: the phase after it may put another frame in that slot
        nxt = (self.ring.ptr(1, k + 2) if (k + 1 < self._end and k + 2 < self.F and self.ring.lo <= k + 2 < self.ring.synced_hi)
               else None)
        obs = DeviceObservation(self.ring.ptr(2, k + 1), pu, pv, self.ring.ptr(1, k + 1),
                                y_m_host=self.source.frame_at(k + 1)[1], next_mask=nxt)
        e = self.kf.compute(obs, None, None, maskflow=self.maskflow)
        t2 = time.perf_counter()
        self.plan.note_frame(t2 - t1)
        self.t_flow += t1 - t0
        self.t_ekf += t2 - t1
        self.iters += getattr(self.kf, "niter", 1)
        self.frame_done.append(t2)
        if self.trace:
            self.trace("step %d: flow wait %.2f ms, filter %.2f ms (%d iterations), series ready %s in flight %s"
                       % (k, 1e3 * (t1 - t0), 1e3 * (t2 - t1), getattr(self.kf, "niter", 1), self._ready,
                          [(s.lo, s.hi) for s in self._flying]))
        return e

    def run(self, first=0, end=None, on_frame=None, video=None, body=None, smoother=None):
        """compute() for the frames first+1 .. end; on_frame(k, error_tuple) after each.

        video: a videoio.AviWriter of the frame size: after every step the overlay at the state the frame ended with
        (Renderer.view(X, "overlay")) is appended to it, composed on the device and written by a thread of its own
        (VideoTap); run() returns when every frame is in the file.  None: nothing is launched or allocated for it.

        body: a body.BodyReadout of the filter's renderer: after every step the raw frame k+1 is read out at the state the
        frame ended with (the warp queued on the device from the frame ring, its sums and registered frame downloaded by
        a thread of its own: body.BodyTap), one row of body.results() per step; run() returns when every row is in.
        The frame ring overwrites the slot of a frame only after its warp (FrameRing.fence_after).  None: nothing is
        launched or allocated for it.

        smoother: a smooth.RTSSmoother of the filter: after every step the frame is recorded (smoother.record(), device
        copies queued on the filter's stream); run its backward pass after run().  None: nothing is launched or
        allocated for it.

        gc_freeze (attribute, default True; the name is round 3's): the interpreter's automatic collections are switched
        off for the phase (gc.disable) and switched back on at its end if they were on -- a full collection, which the
        frame loop's allocations trigger every ~17 frames, took 6.7 ms inside the Python wrapper of hm_update_run with
        numpy / scipy loaded (one frame in 17 at 8.4 instead of 1.7 ms; longer with torch); the youngest generation is
        collected by hand every 64 frames, which takes microseconds.  Nothing the caller froze or tuned is touched
        (round 3 called gc.freeze() / gc.unfreeze() here, which unfroze the caller's objects as well)."""
        end = self.F - 1 if end is None else min(int(end), self.F - 1)
        quiet = bool(self.gc_freeze) and gc.isenabled()
        if quiet:
            gc.disable()
        try:
            self.begin(first, end)
            tap = None
            if video is not None:
                tap = self._video_tap(video)
            btap = self._body_tap(body) if body is not None else None
            if smoother is not None and smoother.kf is not self.kf:
                raise ValueError("run(smoother=...): the smoother of another filter")
            for k in range(first, end):
                e = self.step(k)
                if smoother is not None:
                    smoother.record()
                if tap is not None:
                    tap.frame(self.kf.state.X)
                if btap is not None:
                    btap.frame(self.kf.state.X, self.ring.ptr(0, k + 1), self.ring)
                if on_frame is not None:
                    on_frame(k, e)
                if quiet and (k - first) % 64 == 63:
                    gc.collect(0)
            if tap is not None:
                tap.drain()
            if btap is not None:
                btap.drain()
        finally:
            if quiet:
                gc.enable()

    @property
    def video_tap(self):
        """The VideoTap of the last run(video=...), None before the first (its bus_bytes: what the video copied)."""
        return getattr(self, "_tap", None)

    def _video_tap(self, writer):
        """the VideoTap of this writer, made on first use and kept across run() calls (closed by close())"""
        tap = getattr(self, "_tap", None)
        if tap is None or tap.writer is not writer:
            if tap is not None:
                tap.close()
            tap = self._tap = VideoTap(self.kf.state.renderer, writer, self.device)
        return tap

    def _body_tap(self, body):
        """the BodyTap of this readout, made on first use and kept across run() calls (closed by close())"""
        tap = getattr(self, "_btap", None)
        if tap is None or tap.b is not body:
            if tap is not None:
                tap.close()
            if body.r is not self.kf.state.renderer:
                raise ValueError("run(body=...): the readout of another filter")
            tap = self._btap = BodyTap(body, self.device)
        return tap

    def close(self):
        """Joins the helper threads of the series in flight, drains and destroys the copy stream, frees the ring, the
        flow planes and the flow handles (idempotent).  The filter is the caller's."""
        if getattr(self, "_closed", False):
            return
        self._closed = True
        try:
            for name in ("_tap", "_btap"):
                tap = getattr(self, name, None)
                setattr(self, name, None)
                if tap is not None:
                    tap.close()
            self.flow_sync()
            self._discard_prepared_mask()
        finally:
            self.ring.close()
            for b in (self.d_u, self.d_v):
                b.close()
            for bf in self.bfs:
                bf.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
