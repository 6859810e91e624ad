"""hydra_mi.events on the host: deconvolve equal to the restatement in Python floats (tests/events_ref.py) bit for bit,
optimal and feasible, the decay estimate and the detection of planted events within margins measured beforehand on seeds
0..4 (DESIGN.md section 19 has the tables), and power tables that underflow gracefully."""
import numpy as np
import pytest

import events_ref as ref
from hydra_mi import events

# measured on seeds 0..4 (the tests print the figures again): the worst |estimate_g - 0.9| on ref.planted_trace, and the
# worst pooled precision and recall of binarise on the planted video
G_ERR_WORST = 0.0062059
PRECISION_WORST, RECALL_WORST = 0.632, 0.957


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("F", [1, 2, 3, 37, 300])
def test_deconvolve_equals_the_restatement_bit_for_bit(F):
    rng = np.random.default_rng(F)
    traces = (rng.integers(0, 256, F).astype(np.float64), rng.normal(0.0, 1.0, F) + 3.0 * (rng.random(F) < 0.1),
              np.zeros(F), np.full(F, 100.0))
    for y in traces:
        for g, lam in ((0.8, 0.0), (0.95, 3.0), (0.5, 0.7), (0.9, 1e4)):
            c, s = events.deconvolve(y, g, lam)
            rc, rs = ref.deconvolve(list(y), g, lam)
            assert np.array_equal(_bits(c), _bits(rc)) and np.array_equal(_bits(s), _bits(rs)), (g, lam)
    ys = np.stack(traces[:2])                                               # cells x F, a g and a lam per cell
    c, s = events.deconvolve(ys, [0.8, 0.95], [0.0, 3.0])
    for i, (g, lam) in enumerate(((0.8, 0.0), (0.95, 3.0))):
        rc, rs = ref.deconvolve(list(ys[i]), g, lam)
        assert np.array_equal(_bits(c[i]), _bits(rc)) and np.array_equal(_bits(s[i]), _bits(rs))
    pw, pw2 = events.powers(0.9, F)
    rp, rp2 = ref.powers(0.9, F)
    assert np.array_equal(_bits(pw), _bits(rp)) and np.array_equal(_bits(pw2), _bits(rp2))


def test_noiseless_planted_spikes_come_back():
    """lam = 0 and a trace built from spikes through the AR(1) recursion: the spikes to 1e-9 (all but frame 0, whose
    event the rule leaves in c_0)"""
    rng = np.random.default_rng(3)
    for g in (0.5, 0.8, 0.95):
        sp = (rng.random(400) < 0.05) * rng.uniform(0.5, 2.0, 400)
        sp[0] = 1.0
        y = np.array(ref.ar1(list(sp), g))
        c, s = events.deconvolve(y, g, 0.0)
        assert np.abs(c - y).max() <= 1e-9 and np.abs(s[1:] - sp[1:]).max() <= 1e-9 and s[0] == 0.0


def test_feasible_and_no_worse_than_200_feasible_perturbations():
    rng = np.random.default_rng(4)
    for g, lam in ((0.8, 0.5), (0.95, 2.0), (0.6, 0.0)):
        sp = (rng.random(120) < 0.08) * rng.uniform(1.0, 3.0, 120)
        y = np.array(ref.ar1(list(sp), g)) + rng.normal(0.0, 0.3, 120)
        c, s = events.deconvolve(y, g, lam)
        assert (s >= 0.0).all() and (c >= 0.0).all()
        assert np.abs(c[1:] - g * c[:-1] - s[1:]).max() <= 1e-9
        best = ref.objective(list(c), list(y), g, lam)
        s_full = np.concatenate(([c[0]], s[1:]))                            # (c_0 is free: its "event" is c_0 itself)
        for _ in range(200):
            sq = np.maximum(s_full + rng.normal(0.0, 0.05, 120) * (rng.random(120) < 0.3), 0.0)
            cq = ref.ar1(list(sq), g)                                       # feasible by construction
            assert best <= ref.objective(cq, list(y), g, lam) + 1e-9


def test_estimate_g_on_a_long_planted_trace():
    worst = 0.0
    for seed in range(5):
        y = ref.planted_trace(seed)[0]
        g = events.estimate_g(y)
        assert abs(g - ref.estimate_g(y)) <= 1e-12
        err = g - ref.PLANTED_TRACE["g"]
        print("estimate_g seed %d: %.6f (error %+.6f), noise %.4f" % (seed, g, err, events.noise(y)))
        worst = max(worst, abs(err))
        assert abs(err) <= 2.0 * G_ERR_WORST
        assert abs(events.noise(y) - ref.PLANTED_TRACE["sigma"]) <= 0.1 * ref.PLANTED_TRACE["sigma"]
    print("worst %.7f" % worst)
    assert events.estimate_g(np.zeros(100)) == events.G_MIN and events.estimate_g([1.0, 2.0]) == events.G_MIN


def detection(seed):
    """-> ((precision, recall) of binarise with the defaults, {z: (precision, recall) of dF/F >= z sigma}) pooled over the
    cells of the planted video, a found frame right and a planted one found within one frame"""
    v, cs, _, ev = ref.planted_events(seed)
    dff = ref.disc_dff(v, cs)
    dec, thr = [], {2.0: [], 3.0: [], 4.0: []}
    for i in range(len(cs)):
        g, sg = events.estimate_g(dff[i]), events.noise(dff[i])
        s = events.deconvolve(dff[i], g, events.default_lam(g, sg))[1]
        dec.append((events.binarise(s, events.default_smin(sg)), ev[i]))
        for z in thr:
            thr[z].append((dff[i] >= z * sg, ev[i]))
    return ref.pooled(dec), {z: ref.pooled(p) for z, p in thr.items()}


@pytest.mark.parametrize("seed", range(5))
def test_detection_on_the_planted_video(seed):
    (p, r), thr = detection(seed)
    print("seed %d: deconvolved precision %.3f recall %.3f; thresholded %s" % (
        seed, p, r, ", ".join("%g sigma: %.3f / %.3f" % ((z,) + thr[z]) for z in sorted(thr))))
    assert p >= PRECISION_WORST - 0.05 and r >= RECALL_WORST - 0.05


def test_power_tables_underflow_gracefully():
    pw, pw2 = events.powers(0.5, 3000)
    assert np.isfinite(pw).all() and pw[-1] == 0.0 and pw2[-1] == 0.0 and (pw >= 0.0).all()
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, 3000).astype(np.float64)
    y[1:2500] = 0.0                                                         # a pool longer than the table's range: pw = 0
    for lam in (0.0, 2.0):
        c, s = events.deconvolve(y, 0.5, lam)
        assert np.isfinite(c).all() and np.isfinite(s).all() and (s >= 0.0).all()
        rc, rs = ref.deconvolve(list(y), 0.5, lam)
        assert np.array_equal(_bits(c), _bits(rc)) and np.array_equal(_bits(s), _bits(rs))
