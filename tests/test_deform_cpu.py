"""The correction of the kept video for tissue compression without a device (`pytest -m "not gpu"`): the identities of the
restatement (tests/deform_ref.py) that the device is compared with, the host arithmetic of hydra_mi.deform at its edges,
and the recovery of the planted activity from the planted video under a planted contraction."""
import numpy as np
import pytest

import deform_ref as ref
from hydra_mi import deform


def _small(seed=0, F=4, H=5, W=6, T=3):
    rng = np.random.default_rng(seed)
    tri_of = rng.integers(-1, T, (H, W))
    tri_of[0, 0], tri_of[H - 1, W - 1] = -1, T - 1
    regs = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    regs[0, H - 1, W - 1] = 255
    return regs, tri_of


def test_restatement_identities():
    regs, tri_of = _small()
    F, T = regs.shape[0], 3
    on = tri_of >= 0
    rec = np.where(on[None], regs, 0).astype(np.uint8)
    out, clipped = ref.tri_gain(regs, tri_of, np.full((F, T), 4096))
    assert np.array_equal(out, rec) and clipped == 0                     # the identity, for every byte 0..255
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert np.array_equal(ref.tri_gain(ramp, np.zeros((16, 16), int), np.array([[4096]]))[0], ramp)
    out, clipped = ref.tri_gain(regs, tri_of, np.zeros((F, T), int))
    assert not out.any() and clipped == 0
    out, clipped = ref.tri_gain(regs, tri_of, np.full((F, T), 65535))
    assert out[0, -1, -1] == 255 and clipped == int((((rec.astype(np.int64) * 65535 + 2048) >> 12) > 255).sum()) and clipped > 0
    assert (out[:, ~on] == 0).all()
    one = np.full((1, 1, 1), 255, np.uint8)
    out, clipped = ref.tri_gain(one, np.zeros((1, 1), int), np.array([[65535]]))
    assert out[0, 0, 0] == 255 and clipped == 1
    assert ref.tri_gain(one, np.zeros((1, 1), int), np.array([[4097]]))[1] == 0          # 255.06 rounds to 255: not clipped
    # tri_maps: q = 1 gives c = w1; off the map all three are 0
    c, w1, w2 = ref.tri_maps(regs, tri_of, np.ones((F, T), int))
    assert c.dtype == np.int64 and w1.dtype == np.uint64 and w2.dtype == np.uint64
    assert np.array_equal(c, w1.astype(np.int64)) and np.array_equal(w1, rec.astype(np.uint64).sum(0))
    assert not c[~on].any() and not w1[~on].any() and not w2[~on].any()
    # ... and c against a loop in Python integers on the 6 x 5 box
    q = np.random.default_rng(1).integers(-32767, 32768, (F, T))
    q[0, 0], q[1, 1] = 32767, -32767
    c, w1, w2 = ref.tri_maps(regs, tri_of, q)
    for y in range(tri_of.shape[0]):
        for x in range(tri_of.shape[1]):
            t = int(tri_of[y, x])
            want = sum(int(regs[k, y, x]) * int(q[k, t]) for k in range(F)) if t >= 0 else 0
            assert int(c[y, x]) == want
            assert int(w2[y, x]) == (sum(int(regs[k, y, x]) ** 2 for k in range(F)) if t >= 0 else 0)


def test_overflow_bound_arithmetic():
    """The call refuses F x F x 255 x 32767 >= 2^63.  The first F it refuses is 1 050 647, far beyond what a record holds in
    the tests and nothing there fakes a frame count, so the bound's arithmetic is checked here in Python integers."""
    import math
    F = math.isqrt((2 ** 63 - 1) // (255 * 32767))
    assert F == 1050646 and ref.overflow_bound(F) < 2 ** 63 <= ref.overflow_bound(F + 1)
    # below it the host's numerator F c - w1 u1 stays inside int64 at the extremes of both terms
    assert F * (F * 255 * 32767) < 2 ** 63 and (F * 255) * (F * 32767) < 2 ** 63


def test_gains_and_covariate_edges():
    J = np.array([[1.0, np.nan, 0.5, 1.0], [1.0, 2.0, 0.0, 1e-9], [1.0, 2.0, -1.0, 1.0], [4.0, 2.0, 0.5, 1.0], [0.25, np.inf, 0.5, 1e9]])
    m = deform.gains(J, 1.0)
    assert m.dtype == np.uint16 and m.shape == J.shape
    assert m[:3, 0].tolist() == [4096] * 3 and m[3, 0] == 16384 and m[4, 0] == 1024            # Jref 1
    assert m[:, 1].tolist() == [4096] * 5                                                     # NaN, inf: 4096; Jref 2
    assert m[:, 2].tolist() == [4096] * 5                                                     # 0, negative: 4096; Jref 0.5
    assert m[1, 3] == 1 and m[4, 3] == 65535                                                  # the clip bounds
    assert (deform.gains(J, 0.0) == 4096).all()
    assert deform.gains(J, 2.0)[3, 0] == 65535 and deform.gains(J, 3.0)[4, 0] == 64
    assert (deform.gains(np.full((3, 2), np.nan), 1.0) == 4096).all()                         # no finite frame at all
    q = deform.covariate(J)
    assert q.dtype == np.int32 and q.shape == J.shape
    assert q[:3, 0].tolist() == [0, 0, 0] and q[3, 0] == -12288 and q[4, 0] == 32767           # 16384 (1/4 - 1); 16384 x 3 clipped
    assert q[:, 1].tolist() == [0] * 5 and q[:, 2].tolist() == [0] * 5
    assert q[1, 3] == 32767 and q[4, 3] == -16384
    assert np.abs(q).max() <= 32767


def test_fit_gamma_without_deformation_and_small_triangles():
    rng = np.random.default_rng(0)
    F, T = 40, 5
    M = rng.uniform(50, 100, (F, T))
    n = np.array([20, 20, 20, 20, 20])
    fit = deform.fit_gamma(M, n, np.full((F, T), 0.9))
    assert fit["gamma"] == 0.0 and fit["fitted"] is False and fit["used"] == F * T
    # a planted exponent comes back; a triangle under n_min that says otherwise is not looked at
    J = np.exp(rng.uniform(-0.5, 0.0, (F, T)))
    M = 80.0 * J ** -1.5
    M[:, 4] = 80.0 * J[:, 4] ** 2.0
    n[4] = 7
    fit = deform.fit_gamma(M, n, J)
    assert fit["fitted"] and abs(fit["gamma"] - 1.5) < 1e-9 and fit["r2"] > 1.0 - 1e-9 and fit["used"] == F * 4
    assert np.allclose(fit["slopes"][:4], 1.5) and np.isnan(fit["slopes"][4])
    n[4] = 8
    fit = deform.fit_gamma(M, n, J)
    assert fit["gamma"] < 1.4 and abs(fit["slopes"][4] + 2.0) < 1e-9
    # frames without a finite positive J or M are left out; the clip to 0..3
    J2, M2 = J.copy(), M.copy()
    J2[0, 0], J2[1, 0], M2[2, 0] = np.nan, -1.0, 0.0
    assert deform.fit_gamma(M2, np.array([20, 20, 20, 20, 0]), J2)["used"] == F * 4 - 3
    assert deform.fit_gamma(80.0 * J ** -5.0, n, J)["gamma"] == 3.0 and deform.fit_gamma(80.0 * J ** 2.0, n, J)["gamma"] == 0.0


# the worst of the five seeds, measured with the restatement (the table of DESIGN.md section 20):
# |gamma - 1| 0.1448 (seed 2), corrected mean r(activity) 0.7709 (seed 0), corrected mean |r(J)| 0.1211 (seed 3)
GAMMA_ERR = 2 * 0.1448
R_ACT = 0.7709 - 0.05
R_J = 0.1211 + 0.05


@pytest.fixture(scope="module")
def planted():
    out = {}
    for seed in range(5):
        d = ref.contracting_video(seed, 1.0)
        b = ref.RefBody(d["video"], d["tri_of"], J=d["J"])
        res = deform.correct(b, np.zeros((d["J"].shape[0], 12)))
        out[seed] = (d, b, res)
    return out


def test_planted_contraction_is_taken_out(planted):
    print("seed gamma   r2 | r(activity) mean, min: clean, contracted, corrected | mean |r(J)|: clean, contracted, corrected")
    for seed, (d, b, res) in planted.items():
        assert d["saturated"] < 0.01 and 0.55 <= d["J"].min() and d["J"].max() <= 1.05
        args = (d["tri_of"], d["centres"], d["activity"], d["J"])
        clean, con, cor = (ref.figures(v, *args) for v in (d["clean"], d["video"], b.regs))
        print("%d %.4f %.3f | %.4f %.4f  %.4f %.4f  %.4f %.4f | %.4f %.4f %.4f" % (
            seed, res["gamma"], res["fit_r2"], clean[0], clean[1], con[0], con[1], cor[0], cor[1], clean[2], con[2], cor[2]))
        assert res["fitted"] and abs(res["gamma"] - 1.0) <= GAMMA_ERR
        assert cor[0] >= R_ACT and cor[2] <= R_J
        assert cor[0] >= con[0] + 0.15 and cor[2] < 0.5 * con[2]
        assert res["gain"].dtype == np.uint16 and res["gain"].shape == d["J"].shape and res["clipped"] < 0.01 * d["video"].size


def test_artifact_map(planted):
    for seed, (d, b, res) in planted.items():
        on = d["tri_of"] >= 0
        before, after = res["r_before"], res["r_after"]
        assert before.shape == on.shape and np.isnan(before[~on]).all() and np.isnan(after[~on]).all()
        assert np.isfinite(before[on]).all() and np.abs(before[on]).max() <= 1.0 + 1e-12
        mb, ma = np.median(np.abs(before[on])), np.median(np.abs(after[on]))
        print("seed %d: median |r| over the map %.4f before, %.4f after" % (seed, mb, ma))
        assert ma < mb
    # the map against plain Pearson's r at a few pixels; NaN for a constant pixel and a constant covariate
    d, _, res = planted[0]
    q = res["q"].astype(np.float64)
    for y, x in ((30, 40), (64, 64), (100, 21)):
        t = d["tri_of"][y, x]
        assert abs(res["r_before"][y, x] - np.corrcoef(d["video"][:, y, x].astype(np.float64), q[:, t])[0, 1]) < 1e-12
    regs = d["video"][:8].copy()
    regs[:, 30, 40] = 7
    qq = res["q"][:8].copy()
    qq[:, d["tri_of"][64, 64]] = 5
    r = deform.artifact_map(ref.RefBody(regs, d["tri_of"], J=d["J"][:8]), qq)
    assert np.isnan(r[30, 40]) and np.isnan(r[64, 64]) and np.isfinite(r[100, 21])


def test_refusals_of_the_module():
    d = ref.contracting_video(0, 1.0)
    b = ref.RefBody(d["video"][:6], d["tri_of"], J=d["J"][:6])
    with pytest.raises(ValueError, match="5 states for a record of 6"):
        b5 = ref.RefBody(d["video"][:6], d["tri_of"], J=d["J"][:5])
        deform.correct(b5, np.zeros((5, 12)))
    with pytest.raises(ValueError, match="gamma .* outside 0..3"):
        deform.correct(b, np.zeros((6, 12)), gamma=4.0)
    b.keep = False
    with pytest.raises(RuntimeError, match="without keep=True"):
        deform.triangle_means(b)
    # gamma given: the fit is skipped, gamma 0 changes no byte
    b = ref.RefBody(d["video"][:6], d["tri_of"], J=d["J"][:6])
    res = deform.correct(b, np.zeros((6, 12)), gamma=0.0)
    assert (res["gain"] == 4096).all() and res["clipped"] == 0 and res["fitted"] is False
    assert np.array_equal(b.regs, np.where((d["tri_of"] >= 0)[None], d["video"][:6], 0))
    assert np.array_equal(res["r_before"], res["r_after"], equal_nan=True)
    # exclude: the pixels left out do not count
    ex = np.zeros(d["tri_of"].shape, bool)
    ex[:64] = True
    M, n = deform.triangle_means(b, exclude=ex)
    assert n.sum() == ((d["tri_of"] >= 0) & ~ex).sum() and np.isnan(M[:, n == 0]).all() and np.isfinite(M[:, n > 0]).all()
