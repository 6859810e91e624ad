"""Demixing on the CPU: the restatement (tests/demix_ref.py) against np.linalg.solve and against the seed sums, the host
arithmetic of hydra_mi.demix against the restatement bit for bit (the device's sums supplied by the restatement), and the
paired video, which has to show that demixing beats the ROI traces where cells overlap, does no harm where they hardly
do, settles, and needs its support rule."""
import numpy as np
import pytest

import demix_ref as ref
import roi_ref

THR = 0.47            # hydra_mi.roi.DEFAULT_THR
BOUND = 0.9234        # the worst cell of the restatement over six seeds of paired_video(seed, 4), 0.9434, minus 0.02
CONVERGED = 7.6e-3    # ten times the largest last-round change over those six seeds, 7.59e-4
MARGIN = 0.02         # what a change of seed moves the worst cell by (DESIGN.md section 10's margin)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class _Sums:
    """the reductions of the device, computed by the restatements on a video in host memory"""

    def __init__(self, regs, inmap):
        self.regs, self.m = regs, inmap

    def body_rec_count(self):
        return self.regs.shape[0]

    def body_rec_seed_sums(self, seeds, r_disc, r_in, r_out, R):
        return roi_ref.seed_sums(self.regs, self.m, seeds, r_disc, r_in, r_out, R)

    def body_rec_label_sums(self, labels, L):
        return roi_ref.label_sums(self.regs, self.m, labels, L)

    def body_rec_weighted_sums(self, seeds, weights, R):
        return roi_ref.weighted_sums(self.regs, self.m, seeds, weights, R)

    def body_rec_trace_products(self, seeds, q, R):
        return ref.trace_products(self.regs, self.m, seeds, q, R)


class _Body:
    keep = True

    def __init__(self, regs, inmap):
        self.r = _Sums(regs, inmap)
        self.tri_of_pixel = np.where(inmap, 0, -1).astype(np.int32)


def _same(got, want):
    for key in ("shapes", "C", "dff_demixed", "demix_change", "F_roi", "F_np", "dff"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    for key in ("shapes_q", "demix_D", "demix_M", "demix_G", "demix_kept", "roi_labels"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


def test_cholesky_solve_matches_linalg(hm):
    """G of the paired video is well conditioned (measured: condition numbers 1.7 .. 2.2 over the seeds), so the written
    out factorisation and substitutions agree with LAPACK's to rounding: 1e-10 relative leaves four digits to spare."""
    from hydra_mi import demix
    e = ref.paired_run(0, 4)[3]
    G = e["demix_G"].astype(np.float64)
    cond = np.linalg.cond(G)
    print("condition number of G: %.3g" % cond)
    assert cond < 10.0
    d = np.random.default_rng(0).normal(0.0, 1e9, (40, G.shape[0]))
    want = np.linalg.solve(G, d.T).T
    L = ref.cholesky(G.tolist())
    x = np.array([ref.chol_solve(L, row) for row in d.tolist()])
    assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max()
    Lp, bad = demix.cholesky(G)
    assert bad == -1 and np.array_equal(_bits(Lp), _bits(np.array(L)))
    assert np.array_equal(_bits(demix.solve(Lp, d)), _bits(x))
    # a matrix that does not factor, and the pair that is named for it
    Gs = np.array([[4, 0, 0], [0, 9, 9], [0, 9, 9]], np.int64)
    assert demix.cholesky(Gs.astype(np.float64)) == (None, 2) and ref.cholesky(Gs.astype(np.float64).tolist()) == 2
    assert demix._worst_pair(Gs) == ((1, 2), 1.0)


def test_trace_products_reproduce_the_seed_sums(hm):
    """With the seed trace U itself as q (it fits int32 here) the trace products are seed_sums' c; with U scaled to
    +-2^20 and rounded they are c scaled, to within half a unit of q per frame: |m D - 2^20 c| <= m w1 / 2 in integers."""
    v, cs, _, _ = ref.paired_video(1, 4)
    v, m = v[:60], roi_ref.planted_map()
    ss = roi_ref.seed_sums(v, m, cs, 3.0, 6.0, 8.5, 8)
    U = ss["U"]
    assert np.abs(U).max() < 2 ** 31
    assert np.array_equal(ref.trace_products(v, m, cs, U.astype(np.int32), 8), ss["c"])
    q = np.zeros(U.shape, np.int32)
    mag = [int(np.abs(U[:, s]).max()) for s in range(len(cs))]
    for s in range(len(cs)):
        q[:, s] = [(2 * int(u) * 2 ** 20 + mag[s]) // (2 * mag[s]) for u in U[:, s]]      # rounded in whole numbers
    D = ref.trace_products(v, m, cs, q, 8)
    assert np.abs(q).max() == 2 ** 20
    for s in range(len(cs)):
        for d, c, w1 in zip(D[s].ravel().tolist(), ss["c"][s].ravel().tolist(), ss["w1"][s].ravel().tolist()):
            assert 2 * abs(mag[s] * d - 2 ** 20 * c) <= mag[s] * w1
    assert D.any() and not D[0][~(roi_ref.window(128, 128, cs[0], 8)[2])].any()
    one = ref.trace_products(v, m, cs[:1], np.full((60, 1), -2 ** 31, np.int32), 0)
    assert one.shape == (1, 1, 1) and one[0, 0, 0] == -2 ** 31 * int(v[:, cs[0][1], cs[0][0]].astype(np.int64).sum())


@pytest.mark.parametrize("seed", range(6))
def test_paired_video_4px_demixing_beats_the_roi_trace(hm, seed):
    """paired_video(seed, 4): six pairs of cells 4 px apart.  Measured on the restatement, seeds 0..5, worst-cell
    correlation with the planted activity: the ROI trace F_roi - F_np 0.9540 0.9397 0.9402 0.9088 0.8702 0.9644, the
    demixed trace C after six rounds 0.9855 0.9745 0.9790 0.9481 0.9434 0.9767; the last round changes C by 1.5e-4 ..
    7.6e-4.  BOUND is 0.9434 - 0.02 and CONVERGED ten times 7.59e-4.  The host arithmetic of the product on the same
    sums gives the restatement's numbers bit for bit."""
    from hydra_mi import demix
    v, cs, act, e = ref.paired_run(seed, 4)
    roi_worst = ref.worst_cell(e["F_roi"] - e["F_np"], act)
    worst = ref.worst_cell(e["C"], act)
    print("seed %d: ROI trace %.4f, demixed %.4f, last change %.2e, rounds %s" %
          (seed, roi_worst, worst, e["demix_change"][-1], " ".join("%.4f" % ref.worst_cell(c, act) for c in e["C_rounds"])))
    assert worst > roi_worst
    assert worst > BOUND
    assert e["demix_change"][-1] < CONVERGED
    assert not e["demix_kept"].any() and not e["seed_fallback"].any()
    assert e["shapes"].max(axis=(1, 2)).tolist() == [1.0] * 12 and (e["shapes"][:, 8, 8] > 0).all()
    assert np.isfinite(e["dff_demixed"]).all() and ref.worst_cell(e["dff_demixed"], act) > BOUND
    got = demix.extract(_Body(v, roi_ref.planted_map()), cs + 0.5, alpha=1.0)
    _same(got, e)
    assert got["shapes_q"].dtype == np.uint16 and got["demix_change"].shape == (6,)


@pytest.mark.parametrize("seed", range(6))
def test_paired_video_6px_demixing_does_no_harm(hm, seed):
    """At 6 px the ROI traces are good already (0.9829 .. 0.9917); demixing gives 0.9825 .. 0.9929, never below the ROI
    trace by more than the margin of a change of seed."""
    v, cs, act, e = ref.paired_run(seed, 6)
    roi_worst = ref.worst_cell(e["F_roi"] - e["F_np"], act)
    worst = ref.worst_cell(e["C"], act)
    print("seed %d: ROI trace %.4f, demixed %.4f" % (seed, roi_worst, worst))
    assert worst > roi_worst - MARGIN
    assert e["demix_change"][-1] < CONVERGED


def test_without_the_support_rule_the_iteration_decays(hm):
    """keep = 0 on seed 0: the worst cell reaches 0.9890 in round 2 and falls to 0.8907 by round 6 (the shapes spread
    over the neighbour and the background): the support rule is part of the algorithm."""
    from hydra_mi import demix
    v, cs, act, e = ref.paired_run(0, 4, 6, 0.0)
    per = [ref.worst_cell(c, act) for c in e["C_rounds"]]
    print("keep 0: " + " ".join("%.4f" % x for x in per))
    assert per[5] < per[1]
    _same(demix.extract(_Body(v, roi_ref.planted_map()), cs + 0.5, iters=6, keep=0.0, alpha=1.0), e)


def test_argument_errors(hm):
    from hydra_mi import demix
    v, cs, _, _ = ref.paired_video(0, 4)
    b = _Body(v[:10], roi_ref.planted_map())
    with pytest.raises(ValueError, match="iters 0"):
        demix.extract(b, cs + 0.5, iters=0)
    with pytest.raises(ValueError, match="keep 1"):
        demix.extract(b, cs + 0.5, keep=1.0)
    with pytest.raises(ValueError, match="seed 1 has no ROI pixel of its own"):
        demix.extract(b, np.array([cs[0], cs[0]]) + 0.5)
    b.keep = False
    with pytest.raises(RuntimeError, match="without keep=True"):
        demix.extract(b, cs + 0.5)
