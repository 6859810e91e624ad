"""pipeline.ring_runs: the walk that cuts frames [f0, f1) into runs of consecutive ring slots and names the slots to
mirror behind the ring -- pure integer arithmetic, checked without a GPU: a known answer, its invariants over every small
ring, and the ring filled run by run against the ring filled frame by frame (FrameRing.ensure's staged path)."""
import itertools

from hydra_mi.pipeline import ring_runs


def test_known_answer():
    got = [(f, k, s, list(m)) for f, k, s, m in ring_runs(3, 11, R=5, extra=2, run=3)]
    assert got == [(3, 2, 3, []), (5, 3, 0, [0, 1]), (8, 2, 3, []), (10, 1, 0, [0])]


def _cases():
    for R in range(1, 7):
        for extra, run in itertools.product(range(0, R + 1), range(1, 5)):
            for f0 in range(0, 3 * R + 1):
                for f1 in range(f0, 3 * R + 1):
                    yield R, extra, run, f0, f1


def test_invariants_over_every_small_ring():
    for R, extra, run, f0, f1 in _cases():
        runs = ring_runs(f0, f1, R, extra, run)
        at = f0
        for f, k, s, mirror in runs:
            assert f == at                                  # the runs cover [f0, f1) once, in order
            assert 1 <= k <= run
            assert s == f % R
            assert s + k <= R                               # a run does not cross the end of the ring
            assert list(mirror) == [t for t in range(s, s + k) if t < extra]
            if extra == 0:
                assert len(mirror) == 0
            at = f + k
        assert at == f1
        assert (runs == []) == (f0 == f1)


def test_run_by_run_fills_the_ring_as_frame_by_frame_does():
    for R, extra, run, f0, f1 in _cases():
        staged = {}
        for f in range(f0, f1):                             # FrameRing.ensure, staged frames: slot f % R, and its mirror
            s = f % R
            staged[s] = f
            if s < extra:
                staged[R + s] = f
        by_run = {}
        for f, k, s, mirror in ring_runs(f0, f1, R, extra, run):
            for i in range(k):
                by_run[s + i] = f + i
            for t in mirror:                                # copied behind the ring after the run has landed
                by_run[R + t] = by_run[t]
        assert by_run == staged, (R, extra, run, f0, f1)
