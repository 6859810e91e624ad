"""flowplan.SeriesPlanner (host arithmetic, no GPU): every decision recorded from the pipeline before the planner was split
out of it (tests/golden/series_plan.json: inputs, outputs, the commit they were recorded from) is replayed and must
come out equal -- not close: it is the same arithmetic in the same order -- and the sizes keep their structural
properties whatever the measurements.  Last, no module of the package depends on the order of import."""
import importlib
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SeriesPlanner = importlib.import_module("kalman-hydra_amd.flowplan").SeriesPlanner


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "golden", "series_plan.json")) as fh:
        return json.load(fh)


def planner(table, series=(), frame_s=None, adaptive_first=True, model_ramp=True, first_series=0, flow_late=False,
            second_delay=0.3):
    p = SeriesPlanner()
    p.series_s = {int(n): t for n, t in (table["series"][series] if isinstance(series, str) else series)}
    p.frame_s, p.flow_late = frame_s, flow_late
    p.adaptive_first, p.model_ramp, p.first_series, p.second_delay = adaptive_first, model_ramp, first_series, second_delay
    return p


def cases(table, name):
    """[(case as a dict of the table's axes, recorded output)] in the order the table was recorded in"""
    rec = table[name]
    combos = list(itertools.product(*rec["axes"].values()))
    assert len(combos) == len(rec["out"]) > 0
    return [(dict(zip(rec["axes"], c)), out) for c, out in zip(combos, rec["out"])]


def knobs(c, *more):
    return {k: c[k] for k in ("series", "frame_s", "adaptive_first", "model_ramp") + more if k in c}


def differing(got_and_recorded):
    bad = [(c, got, out) for c, got, out in got_and_recorded if got != out or type(got) is not type(out)]
    return bad[:5], len(bad)


def test_the_table_holds_the_cases_it_should(table):
    assert len(table["parent"]) == 40
    ax = table["next_concurrent"]["axes"]
    assert ax["B"] == [1, 2, 3, 8, 16] and len(ax["series"]) == 5 and ax["flow_late"] == [True, False]
    assert set(ax["frame_s"]) >= {None, 1.7e-3, 3.17e-3, 3.17e-3 * 0.99, 3.17e-3 * 1.01, 4e-3, 12e-3}
    assert table["first"]["axes"]["first_series"] == [0, 1, 5, 99] and table["first"]["axes"]["concurrent"] == [True, False]
    assert {len(flying) for _, _, flying in table["scenes"]} == {0, 1, 2}
    assert [len(h) for h in table["frames"]][:5] == [1, 4, 5, 8, 9]
    # the frame time at which 4 against 5 pairs flips in first() with these series times: the two sides of it are in the table
    first = {(c["frame_s"]): out for c, out in cases(table, "first")
             if (c["B"], c["series"], c["concurrent"], c["adaptive_first"], c["model_ramp"], c["first_series"])
             == (8, "two_eight", False, True, True, 0)}
    assert first[3.03 * 1e-3] == 5 and first[3.04 * 1e-3] == 4


def test_model_equals_the_recorded_one(table):
    bad = differing((c, planner(table, **c).model(), None if out is None else tuple(out)) for c, out in cases(table, "model"))
    assert bad == ([], 0)


def test_first_equals_the_recorded_sizes(table):
    bad = differing((c, planner(table, **knobs(c, "first_series")).first(c["B"], c["concurrent"]), out)
                    for c, out in cases(table, "first"))
    assert bad == ([], 0)


def test_next_equals_the_recorded_sizes(table):
    bad = differing((c, planner(table, **knobs(c)).next(c["last"], c["B"]), out) for c, out in cases(table, "next"))
    assert bad == ([], 0)


def concurrent(table, c, trace=None):
    ready, cursor, flying = table["scenes"][c["scene"]]
    now = table["now"]
    return planner(table, **knobs(c, "flow_late")).next_concurrent(now, tuple(ready), cursor,
                                                                   [(lo, hi, now - age) for lo, hi, age in flying], c["B"], trace)


@pytest.mark.parametrize("name", ["next_concurrent", "next_concurrent_knobs"])
def test_next_concurrent_equals_the_recorded_sizes(table, name):
    bad = differing((c, concurrent(table, c), out) for c, out in cases(table, name))
    assert bad == ([], 0)


def test_next_concurrent_hands_its_reasoning_to_the_callback_and_prints_nothing(table, capsys):
    for c, out in cases(table, "next_concurrent_trace"):
        lines = []
        concurrent(table, dict(c, adaptive_first=True, model_ramp=True), lines.append)
        assert lines == [out], c
    assert capsys.readouterr() == ("", "")


def test_note_frame_equals_the_recorded_medians(table):
    for hist in table["frames"]:
        p = SeriesPlanner()
        for f in hist:
            p.note_frame(f["seconds"])
            assert (p.frame_s, p.frame_hist) == (f["frame_s"], f["hist"])
    slow_first = table["frames"][1]
    assert slow_first[0]["seconds"] > 2 * slow_first[-1]["frame_s"]           # a slow first-use frame in front: not what counts


def test_note_series_and_note_wait_equal_the_recorded_rules(table):
    for c in table["note_series"]:
        p = planner(table, c["before"])
        p.note_series(c["pairs"], c["seconds"], c["alone"], c["waited"])
        assert sorted([n, t] for n, t in p.series_s.items()) == c["after"], c
    for c in table["note_wait"]:
        p = SeriesPlanner()
        p.note_wait(c["opening"], c["waited"])
        assert p.flow_late is c["flow_late"], c
    assert {c["flow_late"] for c in table["note_wait"]} == {True, False}


@pytest.mark.parametrize("name", ["opening", "opening_knobs"])
def test_the_series_beside_the_opening_pair_equals_the_recorded_one(table, name):
    """what the pipeline's _top_up does with the planner beside a pair (0, 1) launched just now"""
    def beside(c):
        p, now, B = planner(table, **knobs(c, "second_delay")), table["now"], c["B"]
        most = p.next(1, B)
        most = p.next_concurrent(now, (0, 0), 0, [(0, 1, now)], B) or most
        return [1, most, p.opening_delay() if c["opening"] else 0.0]
    bad = differing((c, beside(c), out) for c, out in cases(table, name))
    assert bad == ([], 0)


# -- structural properties: no recorded numbers ------------------------------------------------------------------------
SERIES = [{}, {2: 6.8e-3}, {1: 5.3e-3}, {2: 6.8e-3, 8: 15.5e-3}, {2: 7.4e-3, 8: 6.9e-3}, {3: 1e-6, 4: 1.0}, {2: 0.5, 16: 0.6}]
FRAMES = [None, 1e-9, 0.9e-3, 1.7e-3, 3.17e-3, 4e-3, 12e-3, 1.0]
FLYING = [[], [(0, 1, 0.0)], [(3, 5, 7e-3)], [(5, 8, 1.0)], [(6, 9, 12e-3), (9, 14, 2e-3)], [(0, 16, 3e-3), (16, 32, 0.0)]]


def every_planner():
    for series, frame_s, adaptive, ramp, late in itertools.product(SERIES, FRAMES, (True, False), (True, False), (True, False)):
        p = SeriesPlanner()
        p.series_s, p.frame_s, p.adaptive_first, p.model_ramp, p.flow_late = dict(series), frame_s, adaptive, ramp, late
        yield p


def test_every_size_is_between_one_and_B_and_the_ramp_never_shrinks():
    now = 50.0
    for p, B in itertools.product(every_planner(), (1, 2, 3, 8, 16)):
        for first_series in (0, 1, 5, 99):
            p.first_series = first_series
            assert 1 <= p.first(B, False) <= B and p.first(B, True) == 1          # with two handles a phase opens with one pair
        for last in range(1, B + 1):
            assert min(B, last + 1) <= p.next(last, B) <= B
        for flying in FLYING:
            n = p.next_concurrent(now, (1, 3), 2, [(lo, hi, now - age) for lo, hi, age in flying], B)
            assert n is None or 1 <= n <= B
        assert p.opening_delay() >= 0.0


def test_without_measurements_the_fixed_ramp():
    for p in every_planner():
        if p.model() is not None and p.adaptive_first and p.model_ramp:
            continue
        assert [p.next(n, 8) for n in (1, 2, 3, 5, 8)] == [2, 3, 5, 8, 8] and p.next(4, 16) == 6
        assert all(p.next_concurrent(9.0, (0, 2), 1, flying, 8) is None for flying in FLYING)
    p = SeriesPlanner()
    assert p.model() is None and p.first(8, False) == 2 and p.first(1, False) == 1 and p.opening_delay() == 0.0


def test_note_series_keeps_the_fastest_alone_and_waited_for():
    p = SeriesPlanner()
    p.note_series(2, 7.0e-3, alone=True, waited=6e-3)
    p.note_series(2, 6.8e-3, alone=True, waited=6e-3)
    p.note_series(2, 7.5e-3, alone=True, waited=6e-3)
    assert p.series_s == {2: 6.8e-3}
    p.note_series(2, 1e-3, alone=False, waited=6e-3)         # something ran beside it
    p.note_series(2, 1e-3, alone=True, waited=1e-4)          # it was done already: launch -> now is not its duration
    p.note_series(3, 1e-3, alone=False, waited=0.0)
    assert p.series_s == {2: 6.8e-3}
    p.note_series(8, 15.5e-3)                                # timed on its own (calibrate)
    assert p.series_s == {2: 6.8e-3, 8: 15.5e-3} and p.model() is None       # ... no frame of the filter yet
    p.note_frame(4e-3)
    assert p.model() == (6.8e-3, (15.5e-3 - 6.8e-3) / 6, 2)


def test_the_planner_is_plain_arithmetic():
    """no native library, no thread, no clock: what lets it be replayed here"""
    src = open(importlib.import_module("kalman-hydra_amd.flowplan").__file__).read()
    assert "_lib" not in src and "import time" not in src and "threading" not in src and "print(" not in src


# -- no import-order cycle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["sources", "devbuf", "framering", "taps", "flowplan", "pipeline", "videoio", "deepio", "body"])
def test_every_module_imports_first_in_a_fresh_interpreter(first):
    """each of them as the first module of the package a fresh interpreter imports (under the package's own name: the
    hydra_mi alias imports its modules in one fixed order), then under the alias, where it is the same module object"""
    code = ("import importlib, sys; sys.path.insert(0, %r); m = importlib.import_module('kalman-hydra_amd.%s'); "
            "import hydra_mi; assert importlib.import_module('hydra_mi.%s') is m; "
            "from hydra_mi import pipeline, sources, devbuf, framering, taps; "
            "assert all(getattr(pipeline, n) is getattr(o, n) for o, names in ((sources, 'to_gray load_video threshold_mask "
            "VideoStream ArraySource'), (devbuf, 'DeviceBuffer'), (framering, 'ring_runs FrameRing'), (taps, 'SlotRing VideoTap "
            "write_painted_video')) for n in names.split())" % (ROOT, first, first))
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
