"""How many pairs the next flow series of ``pipeline.FlowEKFPipeline`` gets: the policy, apart from the plumbing.

The Brox flow runs ahead of the filter in launch series of 1 .. ``flow_batch`` pairs.  A series that is too small pays
the launch latency of ~900 launches for few pairs, one that is too large has the filter wait for it.  ``SeriesPlanner``
sizes them from what it has been told: what a series of n pairs took alone (``note_series``), what a frame of the filter
takes (``note_frame``), whether the filter has just waited for the flow (``note_wait``).  It has no clock, no thread and
no native call of its own: a method that needs the time is given it, so every decision can be replayed on any machine
(tests/test_flowplan_cpu.py replays the recorded ones of tests/golden/series_plan.json).  It is used from one thread,
the filter's.
"""
import math


class SeriesPlanner:
    """Measurements (``series_s``: pairs -> seconds a series of that size took alone; ``frame_s``: seconds per frame of
    the filter; ``calibrated``; ``flow_late``), knobs and the sizing rules.  The numbers in the comments are 1024^2
    frames and a 201-vertex mesh on one MI355X, the driver's bench."""

    # -- tuned constants -----------------------------------------------------------------------------
    # the fixed ramp without measurements: a phase starts with two pairs and grows 2, 3, 5, 8 (with two handles: 1, 2, 3,
    # 5, 8).  A series of n pairs takes about 5.3 + 1.45 (n - 1) ms, a frame of the filter about 4 ms, and this ramp is
    # the one with the least waiting for that pair of numbers (1, 2, 4, 8 waits 40 % longer); a ramp that is too steep
    # only costs the wait for its larger series, once.
    RAMP = 1.7
    OPENING_PAIRS = 2                # a phase without measurements starts with two pairs; never one pair behind the opening one
    # a series beside the filter takes ~1.3 x as long as alone ...
    BESIDE_FILTER = 1.3
    # ... but the first series of a phase is sized with 1.25: the choice between 4 and 5 pairs sat exactly on the measured
    # frame time -- 3.17 ms -- and fell either way from run to run: 258-260 frames/s with 4, 250-252 with 5 over the
    # driver's 20 frames
    BESIDE_FILTER_FIRST = 1.25
    # two series in flight share the chip, beside the filter: one is done 1.6 x what its work and the work in front of it
    # take alone after its launch
    SHARED_CHIP = 1.6
    FULL_SERIES = 8                  # without model_ramp the first series is sized for one of at most 8 pairs behind it
    MIN_FRAME_S = 1e-4               # a frame of the filter is never taken to be shorter
    WAITED_S = 2e-4                  # sync() took longer than this: the caller really waited for the series
    LATE_S = 5e-4                    # the filter waited longer than this for a series that was not the opening one: late
    HISTORY = 8                      # frames of the filter the median is taken over
    MEDIAN_FROM = 5                  # with fewer on record the fastest one: the slow ones are the first-use frames
    # one size on record: b as a fifth of a two-pair series (1.45 of 7.2 ms)
    SLOPE_GUESS = 0.2

    def __init__(self):
        self.series_s = {}               # pairs -> seconds a series of that size took alone (calibrate, first series of phases)
        self.frame_s = None              # seconds per frame of the filter (median of the last frames)
        self.frame_hist = []
        self.calibrated = False          # FlowEKFPipeline.calibrate() has run
        self.flow_late = False           # the filter waited for a series although it had others to work through before
        self.adaptive_first = True       # size the series from those measurements
        self.first_series = 0            # > 0: fixed size of the first series of every phase
        # model_ramp: the first series of a phase and the ones after it are sized from measured series / frame times
        # (calibrate: what a series of 2 and of B pairs takes alone; first: the smallest first series the ramp can follow;
        # next: the largest series that is done when the filter is through with the previous one, at least one pair more
        # than that one) instead of a fixed 1.7 x ramp from a first series sized for a full one behind it.
        # Driver's 20-frame bench, three runs each on one box: 255.0 against 244.0 frames/s (waiting for flow 0.62
        # against 0.92 ms per frame: a first series of 4 or 5 pairs instead of 8), 64 frames: 307.7 against 301.3.
        self.model_ramp = True
        # the series beside a phase's opening pair starts this fraction of (a series of two pairs alone) later: 0.3 x 7 ms.
        # Three runs each, 20 frames: 263-264 frames/s with 0 (opening wait 7.0-7.7 ms), 263-274 with 0.2, 266-268 with 0.35
        # (6.1-6.4 ms), 262-266 with 0.5 (the second series is late instead)
        self.second_delay = 0.3

    # -- measurements --------------------------------------------------------------------------------
    def note_frame(self, seconds):
        """A frame of the filter took `seconds`.  frame_s is the median of the last few (the first frames of a filter's
        life carry first-use costs -- allocations, the first launches -- that a running mean drags along for a whole
        phase)."""
        self.frame_hist.append(seconds)
        if len(self.frame_hist) > self.HISTORY:
            self.frame_hist.pop(0)
        hist = sorted(self.frame_hist)
        self.frame_s = ((0.5 * (hist[(len(hist) - 1) // 2] + hist[len(hist) // 2])) if len(hist) >= self.MEDIAN_FROM
                        else hist[0])

    def note_series(self, pairs, seconds, alone=True, waited=None):
        """A series of `pairs` took `seconds` from launch to completion.  It counts when nothing ran beside it (`alone`:
        the first series of a phase) and the caller really waited for it (`waited` seconds in sync(); None: it was
        timed on its own, as calibrate does): then launch -> completion is what a series of that many pairs takes.
        The fastest one per size is kept."""
        if alone and (waited is None or waited > self.WAITED_S):
            self.series_s[pairs] = min(self.series_s.get(pairs, 1e9), seconds)

    def note_wait(self, opening, waited):
        """The filter waited `waited` seconds for the series it needed next (the opening one of a phase is always waited
        for: that is not late)."""
        self.flow_late = (not opening) and waited > self.LATE_S

    # -- sizes ---------------------------------------------------------------------------------------
    def model(self):
        """(a, b, n_a): a series of n pairs alone takes about a + b (n - n_a) seconds, from the smallest and the largest
        size on record (two sizes give a and b, one gives a with b guessed); None without measurements."""
        ts = self.series_s
        if not ts or self.frame_s is None:
            return None
        (n_a, t_a), (n_b, t_b) = sorted(ts.items())[0], sorted(ts.items())[-1]
        if n_b > n_a:
            b = max(0.0, (t_b - t_a) / (n_b - n_a))
        else:
            b = self.SLOPE_GUESS * t_a / (1.0 + self.SLOPE_GUESS * (n_a - 2))
        return t_a, b, n_a

    def _modelled(self):
        """model() when the knobs let the series be sized from it, else None: the fixed ramp"""
        return self.model() if self.adaptive_first and self.model_ramp else None

    def first(self, B, concurrent):
        """Pairs of the first series of a phase (at most B).  The filter waits for that series with nothing to do, so it
        should be just large enough that the series after it, running beside the filter, is done by the time the filter
        is through with these.  With two handles (`concurrent`) a phase opens with one pair, the whole chip, and a second
        series beside it."""
        if concurrent:
            return 1
        default = min(self.OPENING_PAIRS, B)
        if self.first_series:
            return max(1, min(B, int(self.first_series)))
        model = self.model()
        if model is None or not self.adaptive_first:
            return default
        t_a, b, n_a = model
        F = max(self.frame_s, self.MIN_FRAME_S)
        if self.model_ramp:
            # the smallest first series the ramp of next() can follow without shrinking: a series of as many pairs,
            # running beside the filter, is done when the filter is through with these
            for n1 in range(default, B + 1):
                if self.BESIDE_FILTER_FIRST * (t_a + b * (n1 - n_a)) <= n1 * F:
                    return n1
            return B
        # the series after the first need not be a full one (next() ramps up to B)
        t_full = t_a + b * (min(B, self.FULL_SERIES) - n_a)
        n1 = math.ceil(self.BESIDE_FILTER * t_full / F)
        return max(default, min(B, n1))

    def next(self, last, B):
        """Pairs of the series that follows one of `last` pairs, one series at a time (and the frames read ahead)."""
        guess = min(B, max(last + 1, int(self.RAMP * last)))
        model = self._modelled()
        if model is None:
            return guess
        # with measurements: the largest series that is done (beside the filter) by the time the filter is through with
        # the `last` frames it has just been given -- a steeper ramp has the filter wait for it -- but at least one pair
        # more than the last one: larger series cost less per pair, and the wait for a series that is one pair too large
        # is a millisecond or two, once
        a, b, n_a = model
        room = last * self.frame_s / self.BESIDE_FILTER
        n = int(n_a + (room - a) / b) if b > 0 else B
        return min(B, max(last + 1, min(n, 2 * last)))

    def next_concurrent(self, now, ready, cursor, flying, B, trace=None):
        """Pairs of the next series with two handles: the largest series that is done by the time the filter needs its
        first pair.  That moment follows from what is queued in front of it -- the pairs of `ready` (lo, hi) from `cursor`
        on, and the series in flight `flying` ((lo, hi, time of launch), oldest first), each ready when the work of the
        series in front of it and its own are done and then used up at one frame of the filter per pair.
        None without measurements: the fixed ramp of next().  `trace`: callable(str), given the reasoning."""
        # (a ramp sized this way is 1, 2, 2, 3, 3, 3, 4: 9.5 ms of waiting over the driver's 20 frames, 6.4 of them for the
        # opening pair, instead of the 13 + 2 of one series at a time)
        model = self._modelled()
        if model is None:
            return None
        a, b, n_a = model
        F, slow = max(self.frame_s, self.MIN_FRAME_S), self.SHARED_CHIP
        t = now + max(0, ready[1] - cursor) * F
        last, overdue = max(1, ready[1] - ready[0]), bool(self.flow_late)
        ahead = 0.0                                # what the series in flight still have to do, in time alone
        for lo, hi, t0 in flying:
            n = hi - lo
            alone = a + b * (n - n_a)
            overdue = overdue or t0 + slow * alone < now
            # (the series in flight share the chip: one is done when the work in front of it and its own are)
            ahead += max(0.0, alone - (now - t0) / slow)
            t = max(t, now + slow * ahead) + n * F
            last = n
        best = 1
        for n in range(1, B + 1):
            if now + slow * (ahead + a + b * (n - n_a)) <= t:
                best = n
        fit = best
        # (a series of one pair costs 5.3 ms a pair, one of two 3.4: only the opening one)
        best = max(best, last, min(B, self.OPENING_PAIRS))
        if overdue:
            best = max(best, last + 1, int(self.RAMP * last))
        if trace:
            trace("next series: %.1f ms until it is needed, a series of n takes %.2f + %.2f (n - %d) ms alone, a frame %.2f ms: "
                  "%d pairs fit, last %d%s -> %d" % (1e3 * (t - now), 1e3 * a, 1e3 * b, n_a, 1e3 * F, fit, last,
                                                     ", overdue" if overdue else "", min(B, best)))
        return min(B, best)

    def opening_delay(self):
        """Seconds the series beside a phase's opening pair waits before it is queued: the opening pair -- what the filter
        is waiting for, a chain of ~450 short launches -- has the chip to itself for a while first (the second series is
        needed a frame of the filter after that pair, and the two slow each other down)."""
        model = self.model() if self.second_delay else None
        return float(self.second_delay) * model[0] if model is not None else 0.0
