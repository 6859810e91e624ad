"""The measurement on the device -- k_star_regions, k_measure_vertex, k_measure_edge, k_hth_scatter through
Renderer.measure; k_jz, k_j, k_jz_multi, k_j_multi and the flow terms of k_render_iter through the single operators --
against the exact reference of tests/measure_exact_ref.py, entry by entry:

    |device - exact| <= (n + C) u M,    u = 2^-53, C = 11

n the entry's non-zero terms, M their absolute mass, C derived in the reference's docstring from the operation counts.
An entry of zero mass is exactly 0 on the device; HTH is exactly 0 off the pattern and symmetric bit for bit.  Every
entry of Hz, of each channel of Hzc and of HTH on the pattern is checked; the largest error / bound per case and array is
printed, and recorded in profiles/measure_precision.md (tools/measure_precision_table.py).

The cases (measure_exact_ref.CASES) are the smallest shapes at which the structure of the kernels changes.  Each one
satisfies the precondition of exactness -- one triangle over a pixel in the reference configuration, at most two in a
perturbed one (tests/test_measure_exact_cpu.py asserts it) -- under which the star sums of k_measure_vertex are the full
renders bit for bit.  Cases that break it stay with the tests that compare against the binary64 oracle at 1e-9 of the
largest entry and are not repeated here: the `folded` states of tests/measure_cases.py, `saturated` at pos_sigma = 3 and
`folded` of test_ekf_gpu.test_measure_edge_cases_match_oracle, and the pool-growth mesh at delta = 2 (here it is
measured at delta = 1.5)."""
import numpy as np
import pytest

import measure_exact_ref as mx
from oracle import partitions_ref

pytestmark = pytest.mark.gpu


def _hold(case, got, sums, label=""):
    """the three arrays against the reference; prints the largest ratios, fails with the per-entry reports"""
    Hz, Hzc, HTH = got
    out, reports = mx.check_measure(case, got, sums)
    print("%s%s: error / bound  %s" % (case["name"], label, "  ".join("%s %.3f" % kv for kv in out.items())))
    assert np.all(HTH[~mx.pattern(case)] == 0), case["name"]
    assert np.array_equal(HTH, HTH.T), case["name"]
    assert not reports, "%d entries out of bounds:\n%s" % (len(reports), "\n".join(reports[:12]))


@pytest.mark.parametrize("name", mx.CASES)
def test_measure_is_within_the_entrywise_bound(hm, name, monkeypatch, capfd):
    case = mx.make_case(name)
    _, sums = mx.exact_of(case)
    if name == "pool_growth":
        monkeypatch.setenv("HYDRA_MI_TRACE", "1")
    got = mx.device_measure(case)                                  # a fresh context
    if name == "pool_growth":                                      # ... whose first measurement found the pool too small
        area, cap = mx.pool_demand(case)
        assert "difference-image pool %d -> %d pixels" % (cap, area + area // 4) in capfd.readouterr().err
    _hold(case, got, sums)


@pytest.mark.parametrize("key,value", [("measure_split", v) for v in mx.MEASURE_SPLITS] + [("edge_split", v) for v in mx.EDGE_SPLITS])
@pytest.mark.parametrize("name", mx.SPLIT_CASES)
def test_every_split_is_within_the_bound(hm, name, key, value):
    """the partial sums of the vertex jobs and of the edge jobs split over 1 .. 16 workgroups: every setting against the
    exact reference, none against another"""
    case = mx.make_case(name)
    _, sums = mx.exact_of(case)
    _hold(case, mx.device_measure(case, {key: value}), sums, " %s=%d" % (key, value))


def _one(what, got, s, worst):
    r, bad = mx.ratio_one(got, s)
    assert not bad, "%s: device %r exact %r error / bound %.3f n %d M %.6e" % (what, got, float(s.S), r, s.n, float(s.M))
    return max(worst, r)


def test_single_operators_are_within_the_bound(hm):
    """Renderer.jz (total and components) for the perturbations of test_ekf_gpu.test_jz_j_error_match_cpu_twin and
    Renderer.j for its pairs, on the golden case"""
    case = mx.make_case("golden")
    ex, _ = mx.exact_of(case)
    N, X = ex.N, case["X"]
    R = mx.device_renderer(case)
    try:
        R.update_vertex_buffer(X[:2 * N].reshape(-1, 2), X[2 * N:].reshape(-1, 2))
        R.initjacobian(case["y_im"], case["flow"], case["y_m"])
        worst = 0.0
        for k in (0, 1, 2 * N - 1, 2 * N, 4 * N - 1):
            Xp = X.copy()
            Xp[k] += 2.0
            got, gc = R.jz(mx.St(Xp))
            tot, c = ex.jz(Xp)
            worst = _one("jz %d" % k, got, tot, worst)
            for ch in range(4):
                worst = _one("jz %d %s" % (k, mx.CHANNELS[ch]), gc[ch], c[ch], worst)
        print("golden jz: error / bound %.3f" % worst)
        worst = 0.0
        for i, j in [(0, 0), (0, 1), (1, 2 * N + 1), (2 * N, 2 * N), (2 * N, 2 * N + 1), (3, 3)]:
            worst = _one("j %d %d" % (i, j), R.j(mx.St(X), 2.0, i, j), ex.j(i, j), worst)
        print("golden j: error / bound %.3f" % worst)
    finally:
        R.close()


def test_label_sums_are_within_the_bound(hm):
    """jz_multi / j_multi per label on the golden case with the partitions and the perturbations of
    test_ekf_gpu.test_jz_multi_and_j_multi_match_oracle (the 9 px one folds triangles: ids add and saturate; every state is
    rendered in full, so the precondition does not enter)"""
    case = mx.make_case("golden")
    ex, _ = mx.exact_of(case)
    N, X = ex.N, case["X"]
    E, labels = partitions_ref.jacobian_partitions(N, case["t"])
    Q, EH, EHi, lh = partitions_ref.hessian_partitions(N, case["t"])
    R = mx.device_renderer(case)
    try:
        R.labels, R.labels_hess, R.Q = labels, lh, Q
        R.update_vertex_buffer(X[:2 * N].reshape(-1, 2), X[2 * N:].reshape(-1, 2))
        R.initjacobian(case["y_im"], case["flow"], case["y_m"])
        worst = 0.0
        for idx, e in enumerate(E):
            e = np.asarray(e)
            for comp, delta in ((0, 2.0), (1, -2.0), (2 * N, 2.0), (2 * N + 1, -2.0), (0, 9.0)):
                Xp = X.copy()
                Xp[comp + 2 * e] += delta
                R.update_vertex_buffer(Xp[:2 * N].reshape(-1, 2), Xp[2 * N:].reshape(-1, 2), idx)
                hz, hzc = R.jz_multi(mx.St(Xp))
                ehz, ehzc = ex.jz_multi(Xp, labels[:, idx], N)
                for lab in range(N):
                    worst = _one("jz_multi %d %d label %d" % (idx, comp, lab), hz[lab, 0], ehz[lab], worst)
                    for ch in range(4):
                        worst = _one("jz_multi %d %d label %d %s" % (idx, comp, lab, mx.CHANNELS[ch]), hzc[lab, ch],
                                     ehzc[lab, ch], worst)
        print("golden jz_multi: error / bound %.3f" % worst)
        worst = 0.0
        for idx in (0, len(EH) // 2, len(EH) - 1):
            e = np.asarray(EH[idx]).reshape(-1, 2)
            for o1, o2 in ((0, 0), (1, 2 * N), (2 * N, 2 * N + 1)):
                ee = np.column_stack((2 * e[:, 0] + o1, 2 * e[:, 1] + o2))
                h, hist, hc = R.j_multi(mx.St(X), 2.0, ee, idx)
                eh, cnt, ehc = ex.j_multi(ee, lh[:, idx], len(Q))
                assert np.array_equal(hist, cnt > 0)
                for lab in range(len(Q)):
                    worst = _one("j_multi %d label %d" % (idx, lab), h[0, lab], eh[lab], worst)
                    for ch in range(4):
                        worst = _one("j_multi %d label %d %s" % (idx, lab, mx.CHANNELS[ch]), hc[lab, ch], ehc[lab, ch], worst)
        print("golden j_multi: error / bound %.3f" % worst)
    finally:
        R.close()


@pytest.mark.parametrize("rows", [16, 8])
def test_flow_terms_of_error_are_within_the_bound(hm, rows):
    """e[1], e[2] of Renderer.error (k_render_iter, strips of 16 and of 8 rows, the two-level sum of the strip partials)
    on the golden case"""
    case = mx.make_case("golden")
    ex, _ = mx.exact_of(case)
    R = mx.device_renderer(case)
    try:
        R.tune("render_rows", rows)
        e = R.error(mx.St(case["X"]), case["y_im"], case["flow"], case["y_m"])
        efx, efy = ex.error_flow(case["X"])
        worst = _one("e_fx", e[1], efx, 0.0)
        worst = _one("e_fy", e[2], efy, worst)
        print("golden error, render_rows %d: error / bound %.3f" % (rows, worst))
    finally:
        R.close()
