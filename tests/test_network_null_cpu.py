"""Significance of co-activity maps against circularly shifted traces, on the CPU: the two forms of the restatement
(tests/network_null_ref.py) against each other, the host functions of hydra_mi.network against the restatement bit for bit
(the device's reduction supplied by the restatement), the rules of shifts, coactivity_null and ensembles(p=...) on
hand-made cases, and the planted video with ensembles, where every planted centre has to be significant in its own
ensemble's map."""
import numpy as np
import pytest

import network_null_ref as nref
import network_ref as ref
import roi_ref
from test_network_cpu import ROI_THR, SEEDS, THR, _Body, _same, _small, _Sums

NULL_TOP = 0.52       # the largest maximum of a surrogate's map over SEEDS, 0.5163 (seed 4), rounded up
OWN = 0.81            # the lowest map value of its own ensemble at a planted centre, 0.8120 (seed 1), rounded down


class _NullSums(_Sums):
    """the two reductions of the device, computed by the restatement on a video in host memory"""

    def body_rec_trace_null(self, q, vb, want=("tmax", "tmin", "ge", "le")):
        assert q.dtype == np.int32 and q.flags["C_CONTIGUOUS"] and q.shape[0] == self.regs.shape[0] and 2 <= q.shape[1] <= 4096
        assert vb.shape == (q.shape[1],) and vb.dtype == np.float64
        o = self.reduce(self.regs, self.m, q, vb)
        return {k: o[k] for k in want}


def _body(regs, m, reduce):
    b = _Body(regs, m)
    b.r = _NullSums(regs, m)
    b.r.reduce = reduce
    return b


def test_shifts_all_sampled_and_too_few(hm):
    from hydra_mi import network
    for f in (network.shifts, nref.shifts):
        every = f(40, 100, 5)                                       # 6 .. 34: all 29 of them
        assert every.dtype == np.int64 and np.array_equal(every, np.arange(6, 35))
        assert np.array_equal(f(40, 29, 5), every)                  # exactly as many as asked for: still all
        assert np.array_equal(f(300, 1000, 10), np.arange(11, 290)) and len(f(300, 1000, 10)) == 279
        some = f(40, 20, 5, seed=3)
        assert len(some) == 20 and np.array_equal(some, np.unique(some)) and np.isin(some, every).all()
        assert np.array_equal(some, f(40, 20, 5, seed=3)) and not np.array_equal(some, f(40, 20, 5, seed=4))
        assert np.array_equal(f(30, 19, 5), np.arange(6, 25))       # 19 candidates: the fewest
        assert np.array_equal(f(20, 50, 0), np.arange(1, 20))       # no guard: every shift but 0
        with pytest.raises(ValueError):
            f(30, 19, 6)                                            # 7 .. 23: 17
        with pytest.raises(ValueError):
            f(19, 19, 0)                                            # 1 .. 18
    for n, guard, seed in ((20, 5, 3), (19, 0, 0), (25, 2, 11)):
        assert np.array_equal(network.shifts(40, n, guard, seed), nref.shifts(40, n, guard, seed))
    with pytest.raises(ValueError, match=r"17 circular shifts of 30 frames beyond a guard of 6 \(need at least 19\)"):
        network.shifts(30, 19, 6)


def test_surrogates_are_rolls(hm):
    from hydra_mi import network
    q = np.array([5, -32767, 0, 32767, 7, 7, -1], np.int32)
    sh = np.array([1, 3, 6])
    got = network.surrogates(q, sh)
    assert got.dtype == np.int32 and got.shape == (7, 4) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, nref.surrogates(q, sh))
    assert np.array_equal(got[:, 0], q) and got[:, 1].tolist() == [-1, 5, -32767, 0, 32767, 7, 7]
    assert all(np.array_equal(got[:, 1 + j], np.roll(q, s)) for j, s in enumerate(sh))


def test_the_two_restatements_agree(hm):
    """Python integers pixel by pixel against vectorised int64, with a column equal to column 0 (a tie counts in both
    planes), an all-zero column (vb = 0: rho 0), +-32767 throughout, a constant pixel (both counts L - 1)."""
    regs, m, x = _small()
    q = ref.quantise(x)
    Q = nref.surrogates(q[0], np.arange(6, 35))
    Q[:, 3] = Q[:, 0]
    Q[:, 4] = 0
    Q[:, 5], Q[:, 6] = 32767, -32767
    Q[::3, 6] = 32767
    vb = np.array([nref.vb_of(Q[:, s]) for s in range(Q.shape[1])])
    assert vb[4] == 0.0 and vb[5] == 0.0 and vb[6] > 0.0
    a, b = nref.trace_null(regs, m, Q, vb), nref.trace_null_np(regs, m, Q, vb)
    assert all(_same(a[k], b[k]) for k in ("tmax", "tmin")) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.uint32 for k in ("ge", "le"))
    L = Q.shape[1]
    assert a["ge"][2, 3] == L - 1 and a["le"][2, 3] == L - 1       # the constant pixel: every num is 0
    assert not a["ge"][~m].any() and not a["le"][~m].any()
    assert ((a["ge"].astype(int) + a["le"])[m] >= L - 1 + 1).all()  # (column 3 ties everywhere)
    assert a["tmax"][4] == 0.0 and a["tmin"][4] == 0.0 and a["tmax"][5] == 0.0 and a["tmax"][3] == a["tmax"][0]
    rho = ref.maps(regs, m, x[:1])
    assert a["tmax"][0] == np.nanmax(rho) and a["tmin"][0] == np.nanmin(rho)


def test_map_null_equals_the_restatement(hm):
    from hydra_mi import network
    regs, m, x = _small()
    for n, seed in ((100, 0), (20, 7)):                              # all 29 shifts beyond the guard, 20 drawn from them
        got = network.map_null(_body(regs, m, nref.trace_null), x, n=n, guard=5, seed=seed, alpha=0.1)
        want = nref.map_null(regs, m, x, n=n, guard=5, seed=seed, alpha=0.1, reduce=nref.trace_null)
        S = min(n, 29)
        assert np.array_equal(got["shifts"], want["shifts"]) and got["rho_max"].shape == (5, S) and got["p_map"].shape == (5,) + m.shape
        for k in ("rho", "rho_max", "rho_min", "p_map", "p_pix"):
            assert _same(got[k], want[k]), k
        assert got["sig"].dtype == bool and np.array_equal(got["sig"], want["sig"])
        assert np.isnan(got["p_map"][:, ~m]).all() and np.isnan(got["p_pix"][:, ~m]).all() and not got["sig"][:, ~m].any()
        assert (got["p_map"][1][m] == 1.0).all() and (got["rho_max"][1] == 0.0).all()       # the zero trace: every rho is 0
        assert (got["p_pix"][:, 2, 3] == 1.0).all()                                           # the constant pixel
        assert got["p_map"][2, 3, 3] == 1.0 / (S + 1) and got["sig"][2, 3, 3]                # the trace that is a pixel, there
        assert (got["p_map"][:, m] >= 1.0 / (S + 1)).all() and (got["p_map"][:, m] <= 1.0).all()
        assert np.array_equal(got["sig"], np.where(np.isnan(got["p_map"]), False, got["p_map"] <= 0.1))
    with pytest.raises(RuntimeError, match="without keep=True"):
        network.map_null(type("B", (), {"keep": False})(), x)
    with pytest.raises(ValueError, match="need at least 19"):
        network.map_null(_body(regs, m, nref.trace_null), x, guard=11)


def test_coactivity_null_with_a_tie(hm):
    """Forty frames, every shift 1..39.  Cells 0 and 1 fire in frames 0 and 20: moved by 20 frames cell 1 is itself, a tie
    with the observed value that counts (p = 2 / 40); cell 2 fires in frames 5 and 25: against cell 0 the observed sum of
    products is 0, no surrogate is below it (p = 1), and moved by 15 or 35 it meets cell 0."""
    from hydra_mi import network
    F = 40
    x = np.zeros((5, F))
    x[0, [0, 20]] = 2.0
    x[1, [0, 20]] = 0.5
    x[2, [5, 25]] = 1.0
    x[3] = np.sin(np.arange(F))
    x[4] = x[3]
    x[4, 7] = np.nan
    sh = np.arange(1, F)
    for f in (network.coactivity_null, nref.coactivity_null):
        p = f(x, sh)
        assert p.shape == (5, 5) and p.dtype == np.float64
        assert p[0, 1] == 2.0 / 40.0 and p[1, 0] == 2.0 / 40.0
        assert p[0, 2] == 1.0 and p[2, 0] == 1.0
        assert np.isnan(np.diag(p)).all() and np.isnan(p[4]).all() and np.isnan(p[:, 4]).all() and not np.isnan(p[:4, :4][~np.eye(4, dtype=bool)]).any()
    assert _same(network.coactivity_null(x, sh), nref.coactivity_null(x, sh))
    few = np.array([3, 20, 21])
    assert _same(network.coactivity_null(x, few), nref.coactivity_null(x, few)) and network.coactivity_null(x, few)[0, 1] == 2.0 / 4.0
    rng = np.random.default_rng(5)
    y = rng.normal(0.0, 1.0, (4, 33))
    assert _same(network.coactivity_null(y, np.arange(4, 30)), nref.coactivity_null(y, np.arange(4, 30)))


@pytest.fixture(scope="module")
def planted():
    m = roi_ref.planted_map()
    out = {}
    for seed in SEEDS:
        v, cs, act = ref.planted_video(seed)
        out[seed] = (v, cs, roi_ref.extract(v, m, cs, thr=ROI_THR))
    return m, out


def test_ensembles_with_p_values(hm, planted):
    from hydra_mi import network
    m, runs = planted
    x = runs[1][2]["dff"].T
    r0 = ref.coactivity(x)[:, :, 0]
    old = ref.ensembles(r0, THR)
    assert np.array_equal(network.ensembles(r0), old) and np.array_equal(network.ensembles(r0, p=None), old)
    assert np.array_equal(network.ensembles(r0, THR, None, 0.05), old) and np.array_equal(old, ref.planted_labels())
    sh = network.shifts(x.shape[1], 50, 10)
    p = network.coactivity_null(x, sh)
    assert _same(p, nref.coactivity_null(x, sh))
    same = old[:, None] == old[None, :]
    assert (p[same & ~np.eye(12, dtype=bool)] == 1.0 / 51.0).all()   # within an ensemble no shifted trace does as well
    assert np.array_equal(network.ensembles(r0, p=p), old)
    # an edge needs its p-value too: one direction is enough, NaN is none
    r1 = np.eye(4)
    r1[0, 1] = r1[1, 0] = r1[2, 3] = r1[3, 2] = r1[1, 2] = r1[2, 1] = 0.9
    p1 = np.full((4, 4), 0.5)
    p1[0, 1], p1[3, 2], p1[1, 2], p1[2, 1] = 0.05, 0.01, 0.06, np.nan
    assert network.ensembles(r1, 0.6).tolist() == [0, 0, 0, 0]
    assert network.ensembles(r1, 0.6, p=p1).tolist() == [0, 0, 1, 1]
    assert network.ensembles(r1, 0.6, p=p1, alpha=0.06).tolist() == [0, 0, 0, 0]
    assert network.ensembles(r1, 0.6, p=p1, alpha=0.02).tolist() == [-1, -1, 0, 0]


def test_planted_centres_are_significant(hm, planted):
    """On the planted video with ensembles (seeds 0..4), the ensemble traces of roi_ref.extract against all 279 circular
    shifts beyond a guard of 10 frames, by the exact rule of the restatement.  Measured, per seed: the largest maximum of a
    surrogate's map 0.4797, 0.5124, 0.4976, 0.5049, 0.5163; the lowest map value of its own ensemble at a planted centre
    0.8364, 0.8120, 0.8519, 0.8145, 0.8461.  Asserted: both figures, and with them that every planted centre is
    significant in its own ensemble's map at alpha 0.05 on every seed, at the smallest p-value there is, 1 / 280.
    Pixels away from the cells are not asserted to be insignificant: on seeds 2 and 4 the neuropil does correlate with
    an ensemble's trace.  On seed 1 hydra_mi.network equals the restatement bit for bit."""
    from hydra_mi import network
    m, runs = planted
    for seed in SEEDS:
        v, cs, e = runs[seed]
        ens = ref.ensemble_traces(e["dff"].T, ref.planted_labels())
        o = nref.map_null(v, m, ens, n=1000, guard=10, alpha=0.05)
        assert len(o["shifts"]) == 279 and o["rho_max"].shape == (3, 279)
        top = o["rho_max"].max()
        own = [o["rho"][ref.planted_ensemble(i), r, c] for i, (c, r) in enumerate(cs)]
        print("seed %d: the largest null maximum %.4f, the lowest own-map value at a centre %.4f, %s significant pixels" % (
            seed, top, min(own), o["sig"].sum((1, 2)).tolist()))
        assert top <= NULL_TOP and min(own) >= OWN
        for i, (c, r) in enumerate(cs):
            assert o["sig"][ref.planted_ensemble(i), r, c] and o["p_map"][ref.planted_ensemble(i), r, c] == 1.0 / 280.0
        if seed == 1:
            got = network.map_null(_body(v, m, nref.trace_null_np), ens, n=1000, guard=10)
            for k in ("rho", "rho_max", "rho_min", "p_map", "p_pix"):
                assert _same(got[k], o[k]), k
            assert np.array_equal(got["sig"], o["sig"]) and np.array_equal(got["shifts"], o["shifts"])
