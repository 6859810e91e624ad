"""The exact reference of the measurement sums (tests/measure_exact_ref.py) on its own, without a GPU: the binary64
oracle lies within the entrywise bound (n + C) u M on every entry of every case -- the bound is attainable --, known
answers on the two-triangle square, the reference's two code paths against each other, and planted faults: what the
bound rejects and what the suite's earlier bar, 1e-9 of the largest entry of an array, lets through."""
from fractions import Fraction

import numpy as np
import pytest

import measure_exact_ref as mx
from oracle import ekf_ref, partitions_ref


def _report(case, got, sums):
    out, reports = mx.check_measure(case, got, sums)
    print(case["name"], " ".join("%s %.3f" % kv for kv in out.items()))
    assert not reports, "\n".join(reports[:10])
    return out


@pytest.mark.parametrize("name", mx.CASES)
def test_oracle_is_within_the_bound(name):
    """every case of the table: the precondition of exactness holds, the C twin of the oracle is within the bound at
    every entry of Hz, Hzc and HTH, and where the mass is zero it is exactly zero"""
    case = mx.make_case(name)
    ex, sums = mx.exact_of(case)
    ref, pert = ex.coverage()
    assert ref <= 1 and pert <= 2, (name, ref, pert)
    got = mx.oracle_measure(case)
    _report(case, got, sums)
    assert np.all(got[2][~mx.pattern(case)] == 0)
    assert any(s is not None and s.n > 0 for s in sums[2].ravel())
    if "oracle" in case:                                              # the numbers of the golden file as well
        _report(case, case["oracle"], sums)
    if name == "pool_growth":
        area, cap = mx.pool_demand(case)
        assert area > cap


def test_cases_that_break_the_precondition_are_recognised():
    """the pool-growth mesh at the default delta: three triangles over a pixel of a perturbed configuration"""
    case = mx.make_case("pool_growth")
    ex = mx.Exact(case["p"], case["t"], case["tex"], case["X"], case["y_im"], case["flow"], case["y_m"], delta=2.0)
    assert not mx.precondition_holds(ex)


# ---- known answers ----------------------------------------------------------------------------------------------------
EPS_KNOWN = (2.0 ** -10, 1.0, 4.0)


def _square():
    """the square [10, 30)^2 of a constant texture 100, velocity (0.5, 0.25) everywhere, observed moved by one pixel in
    x with zero flow: r is 100 / 0.5 / -0.25 / 255 on columns and rows 10..29; z_im = +-100 and z_m = +-255 on columns
    30 and 10, z_fx = -0.5 and z_fy = -0.25 inside r"""
    from hydra_mi import mesh
    dm = mesh.square4_mesh(10, 30)
    tex = np.full((64, 64), 100, np.uint8)
    X = np.concatenate((dm.p.reshape(-1), np.tile([0.5, 0.25], 4)))
    Xo = X.copy()
    Xo[0:8:2] += 1.0
    y_im, _, _, ym = ekf_ref.render(Xo, 4, dm.t, dm.p, tex, 64, 64)
    return mx.Exact(dm.p, dm.t, tex, X, y_im, np.zeros((64, 64, 2), np.float32), ym // 255, EPS_KNOWN), X


def test_known_answers_on_the_square():
    ex, X = _square()
    eZ, eJ, eM = (Fraction(e) for e in EPS_KNOWN)
    # the whole square moved by 2 px in x: D = +(100, 0.5, -0.25, 255) on columns 30, 31 and the negative on 10, 11
    Xp = X.copy()
    Xp[0:8:2] += 2.0
    tot, c = ex.jz(Xp)
    want = (Fraction(2 * 20 * 100 * 100, 255 * 255) / eZ,       # columns 30 and 10, 20 rows each
            Fraction(40) * Fraction(1, 4) / eJ,                 # columns 10, 11: (-0.5)(-0.5)
            Fraction(40) * Fraction(1, 16) / eJ,                # -(0.25)(-0.25) on columns 10, 11
            Fraction(40) / eM)                                  # columns 30 and 10: 255 * 255 / 255^2
    for s, w, n in zip(c, want, (40, 40, 40, 40)):
        assert s.S == w and s.M == w and s.n == n
        assert s.big == w / n
    assert tot.S == sum(want) and tot.n == 160 and tot.M == sum(want)
    # ... and moved by 2 px in y in the other state: the two differences meet on columns 10, 11 x rows 10, 11
    Xq = X.copy()
    Xq[1:8:2] += 2.0
    s = ex.j_states(Xp, Xq)
    want = Fraction(4 * 100 * 100, 255 * 255) / eZ + Fraction(4) * Fraction(1, 4) / eJ + Fraction(4) * Fraction(1, 16) / eJ \
        + Fraction(4) / eM
    assert s.S == want and s.M == want and s.n == 16
    # two states moved off r to either side: their differences meet on r's own pixels only, where both are -r
    far = X.copy()
    far[0:8:2] += 25.0
    far2 = X.copy()
    far2[0:8:2] -= 25.0                                         # (leaves the frame in part)
    e = ex.j_states(far, far2)
    assert e.S == Fraction(400 * 100 * 100, 255 * 255) / eZ + 100 / eJ + 25 / eJ + 400 / eM and e.n == 1600
    efx, efy = ex.error_flow(X)
    assert (efx.S, efx.n, efy.S, efy.n) == (100, 400, 25, 400)
    # measure: the velocity rows hold a flow term only, and nothing couples vx to vy
    Hz, Hzc, HTH = ex.measure()
    for v in range(4):
        assert all(Hzc[8 + 2 * v, ch].n == 0 for ch in (0, 2, 3)) and Hzc[8 + 2 * v, 1].n > 0
        assert all(Hzc[9 + 2 * v, ch].n == 0 for ch in (0, 1, 3)) and Hzc[9 + 2 * v, 2].n > 0
        assert HTH[8 + 2 * v, 9 + 2 * v].n == 0 and HTH[8 + 2 * v, 9 + 2 * v].S == 0
    assert HTH[0, 2] is HTH[2, 0]


def test_measure_agrees_with_the_single_operators():
    """Exact.measure (difference images cropped to their support, sums over unions and intersections of boxes) against
    Exact.jz / Exact.j (whole frames) on the golden case: the same exact sums up to the one math.fsum rounding each
    takes per flow channel; the same masses; n of a central difference at most the two jz together"""
    case = mx.make_case("golden")
    ex, (Hz, Hzc, HTH) = mx.exact_of(case)
    N, d = ex.N, Fraction(ex.delta)
    for k in (0, 1, 7, 2 * N - 1, 2 * N, 2 * N + 5, 4 * N - 1):
        Xp, Xm = ex.X.copy(), ex.X.copy()
        Xp[k] += ex.delta
        Xm[k] -= ex.delta
        (tp, cp), (tm, cm) = ex.jz(Xp), ex.jz(Xm)
        for ch in range(4):
            s = Hzc[k, ch]
            assert abs(s.S - (cp[ch].S - cm[ch].S) / d / 2) <= 3 * mx.U * s.M, (k, ch)
            assert abs(s.M - (cp[ch].M + cm[ch].M) / d / 2) <= 3 * mx.U * s.M
            assert max(cp[ch].n, cm[ch].n) <= s.n <= cp[ch].n + cm[ch].n
        assert Hz[k].n == sum(Hzc[k, ch].n for ch in range(4))
    pat = mx.pattern(case)
    for i, j in ((0, 0), (0, 1), (1, 2 * N + 1), (2 * N, 2 * N), (2 * N, 2 * N + 1), (3, 3)):
        s = ex.j(i, j)
        assert pat[i, j]
        assert abs(HTH[i, j].S - s.S / d / d) <= 3 * mx.U * HTH[i, j].M and HTH[i, j].n == s.n, (i, j)
    # off the pattern there is no entry; the dense _hessian of the reference would find exact zeros there
    i, j = np.argwhere(~pat)[0]
    assert HTH[i, j] is None and ex.j(int(i), int(j)).M == 0


def test_label_sums_and_error_sums_against_the_oracle():
    """jz_multi / j_multi per label and the flow sums of error: the binary64 oracle within the bound, labels and pixel
    counts identical; the labels of a partition add up to the whole jz"""
    case = mx.make_case("golden")
    ex, _ = mx.exact_of(case)
    N = ex.N
    meas = ekf_ref.Measurement(N, case["t"], case["p"], case["tex"], *case["eps"])
    meas.initjacobian(case["X"], case["y_im"], case["flow"], case["y_m"])
    E, labels = partitions_ref.jacobian_partitions(N, case["t"])
    Q, EH, EHi, lh = partitions_ref.hessian_partitions(N, case["t"])
    worst = 0.0
    for idx in (0, len(E) - 1):
        e = np.asarray(E[idx])
        for comp, delta in ((0, 2.0), (2 * N + 1, -2.0), (0, 9.0)):
            Xp = ex.X.copy()
            Xp[comp + 2 * e] += delta
            hz, hzc = ex.jz_multi(Xp, labels[:, idx], N)
            rhz, rhzc = meas.jz_multi(Xp, labels[:, idx], N)
            w1, bad1 = mx.ratios(rhz, hz)
            w2, bad2 = mx.ratios(rhzc, hzc)
            assert not bad1 and not bad2, (idx, comp, bad1, bad2)
            worst = max(worst, w1, w2)
            whole, _ = ex.jz(Xp)
            unl = np.asarray(labels[:, idx]) < 0
            if not unl.any():                                   # every triangle labelled: nothing falls between the labels
                assert abs(sum(s.S for s in hz) - whole.S) <= 8 * mx.U * whole.M
                assert sum(s.n for s in hz) == whole.n
    for idx in (0, len(EH) - 1):
        e = np.asarray(EH[idx]).reshape(-1, 2)
        for o1, o2 in ((0, 0), (1, 2 * N), (2 * N, 2 * N + 1)):
            ee = np.column_stack((2 * e[:, 0] + o1, 2 * e[:, 1] + o2))
            h, cnt, hc = ex.j_multi(ee, lh[:, idx], len(Q))
            rh, rnz, rhc = meas.j_multi(2.0, ee, lh[:, idx], len(Q))
            assert np.array_equal(cnt, rnz.astype(np.int64))
            w1, bad1 = mx.ratios(rh, h)
            w2, bad2 = mx.ratios(rhc, hc)
            assert not bad1 and not bad2, (idx, o1, o2)
            worst = max(worst, w1, w2)
    efx, efy = ex.error_flow(case["X"])
    r = meas.error(case["X"], case["y_im"], case["flow"], case["y_m"])
    for got, s in ((r[1], efx), (r[2], efy)):
        ratio, bad = mx.ratio_one(got, s)
        assert not bad
        worst = max(worst, ratio)
    print("oracle, label and error sums: largest error / bound %.3f" % worst)


# ---- planted faults ---------------------------------------------------------------------------------------------------
def _entries(ex, sums):
    """every entry of the three arrays with n >= 1: (array name, index, Sum, mirror Sum, unit fault)"""
    Hz, Hzc, HTH = sums
    n4 = 4 * ex.N
    for k in range(n4):
        if Hz[k].n:
            yield "Hz", (k,), Hz[k], Hz[k ^ 1], ex.unit_fault_hz(k)
        for ch in range(4):
            if Hzc[k, ch].n:
                yield "Hzc", (k, ch), Hzc[k, ch], Hzc[k ^ 1, ch], ex.unit_fault_hz(k) if ch == 0 else None
    for i in range(n4):
        for j in range(i, n4):
            if HTH[i, j] is not None and HTH[i, j].n:
                yield "HTH", (i, j), HTH[i, j], HTH[i ^ 1, j ^ 1], ex.unit_fault_hth(i, j)


def test_planted_faults_are_rejected_and_the_old_bar_passes_them():
    """On the golden case, for every entry with n >= 1 of Hz, Hzc and HTH (upper triangle of the pattern):
      dropped   the entry's largest product left out.  It is at least M / (2 n) (M / n where the sum is not a central
                difference), beyond the bound whenever 2 n (n + C + 1) < 2^53: no entry may be left out;
      unit      one image difference D+ off by one unit of 1/255, at the pixel where that changes the entry least (entries
                without an image term on the other factor are not changed by it and not counted);
      binary32  the entry's terms accumulated in binary32 (an entry whose binary32 sum is the exact value is no fault);
      mirror    the entry of the mirror job, x and y swapped (Hz[x_v] for Hz[y_v], HTH[x_v, y_w] for HTH[y_v, x_w]; where
                both are the same entry, or the same value, nothing was swapped).
    The bound rejects every one.  The earlier bar of the suite, 1e-9 of the largest entry of the array, is counted beside
    it: the number of these faults it lets through is printed, and is the reason for these tests."""
    case = mx.make_case("golden")
    ex, sums = mx.exact_of(case, keep_terms=True)
    scale = {"Hz": max(abs(float(s.S)) for s in sums[0]), "Hzc": max(abs(float(s.S)) for s in sums[1].ravel()),
             "HTH": max(abs(float(s.S)) for s in sums[2].ravel() if s is not None)}
    planted = {"dropped": 0, "unit": 0, "binary32": 0, "mirror": 0}
    passed_old = dict(planted)
    entries = 0

    def plant(kind, what, idx, s, value):
        err = abs(Fraction(value) - s.S)
        assert err > s.bound(), (kind, what, idx, float(err), float(s.bound()), s.n)
        planted[kind] += 1
        if float(err) <= 1e-9 * scale[what]:
            passed_old[kind] += 1

    for what, idx, s, mirror, unit in _entries(ex, sums):
        entries += 1
        assert s.big != 0 and 2 * s.n * (s.n + mx.C + 1) < 2 ** 53
        plant("dropped", what, idx, s, float(s.S - s.big))
        if what != "Hzc" and all(k < 2 * ex.N for k in idx):       # position entries all have an image term
            assert unit is not None, (what, idx)
        if unit is not None:
            plant("unit", what, idx, s, float(s.S + unit))
        t32 = np.float32(0)
        for t in s.terms.astype(np.float32):
            t32 = np.float32(t32 + t)
        if Fraction(float(t32)) != s.S:
            plant("binary32", what, idx, s, float(t32))
        if mirror is not s and mirror is not None and mirror.S != s.S:
            plant("mirror", what, idx, s, float(mirror.S))
    assert planted["dropped"] == entries
    assert planted["binary32"] > 0.9 * entries and planted["mirror"] > 0.9 * entries
    total = sum(passed_old.values())
    print("golden case, %d entries: planted %s; the bar 1e-9 x max lets through %s = %d of %d" % (
        entries, planted, passed_old, total, sum(planted.values())))
    assert total > 0


def test_the_old_bar_on_the_golden_file():
    """what the issue states about tests/golden/measure_64.npz: the spread of the entries, and how many of them the bar
    1e-9 x max holds to worse than 1e-6 of their own size"""
    case = mx.make_case("golden")
    Hz, Hzc, HTH = case["oracle"]
    nz = np.abs(HTH[HTH != 0])
    assert nz.size == 1372 and 3800 < nz.max() < 3900 and nz.min() < 2e-3
    assert np.count_nonzero(nz < 1e-4 * nz.max()) == 270
    worse = {k: mx.old_bar_worse_than(a) for k, a in (("Hz", Hz), ("Hzc", Hzc), ("HTH", HTH))}
    print("entries the bar 1e-9 x max holds to worse than 1e-6 relative:", worse)
    assert worse["HTH"] > 0
