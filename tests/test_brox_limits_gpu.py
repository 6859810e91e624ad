"""The Brox path at its structural limits (tests/brox_cases.py): every operator at frames narrower than its stencil,
the whole flow over the case table -- each halo layout of both SOR tiles, last tiles of 1 and 2 px, the deep plan on
and off, the fused passes, the k_coarse split up to the 128-level cap -- with the per-level SOR launches the host
restatement predicts, the tuning knobs, omega, and the refusal of a pyramid level of one pixel.

The bar is the one of test_brox_gpu.py: BIT-EXACT equality with oracle/brox_ref.c (np.array_equal), and a finite flow.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import brox_cases as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = [(1, 2), (2, 1), (2, 2), (3, 5), (5, 3), (5, 5), (15, 15), (16, 16)]
FIT_X = [(1, 300), (2, 200), (33, 129), (64, 65)]        # sor_plan: fits the tile on x, not on y
FIT_Y = [(300, 1), (129, 33)]
SCALES = (0.8, 0.5, 0.2, 0.1)                             # blur radius 2, 4, 9 and the clamp 16


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


def _smooth(shape, seed):
    from scipy import ndimage
    return ndimage.gaussian_filter(np.random.default_rng(seed).random(shape), 2.0).astype(np.float32)


def _level_fields(oracle_brox, w, h, seed):
    I0, I1 = _smooth((h, w), seed), _smooth((h, w), seed + 1)
    Ix0, Iy0 = oracle_brox.deriv(I0)
    I1x, I1y = oracle_brox.deriv(I1)
    I1xx, I1xy = oracle_brox.deriv(I1x)
    _, I1yy = oracle_brox.deriv(I1y)
    return (I0, Ix0, Iy0, I1, I1x, I1y, I1xx, I1xy, I1yy, _rand((h, w), seed + 2, -3, 3), _rand((h, w), seed + 3, -3, 3))


def _same(got, want, what):
    for i, (g, r) in enumerate(zip(got, want)):
        assert np.isfinite(g).all(), (what, i)
        assert np.array_equal(g, r), (what, i)


# ---- the single operators ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SMALL + FIT_X + FIT_Y)
def test_image_operators_at_small_shapes_and_large_radii(hm, oracle_brox, w, h):
    from hydra_mi import brox
    img, img1 = _smooth((h, w), 1), _smooth((h, w), 2)
    for scale in SCALES:
        _same([brox.op_blur(img, scale)], [oracle_brox.blur(img, scale)], ("blur", scale))
        wd, hd = max(1, int(np.ceil(w * scale))), max(1, int(np.ceil(h * scale)))
        want = oracle_brox.resample(oracle_brox.blur(img, scale), wd, hd, 1.0)
        _same([brox.op_pyr_down(img, wd, hd, scale)], [want], ("pyr_down", scale))
    _same(brox.op_deriv(img), oracle_brox.deriv(img), "deriv")
    Ix0, Iy0 = oracle_brox.deriv(img)
    I1x, I1y = oracle_brox.deriv(img1)
    I1xx, I1xy = oracle_brox.deriv(I1x)
    _, I1yy = oracle_brox.deriv(I1y)
    _same(brox.op_deriv_all(img, img1), (Ix0, Iy0, I1x, I1y, I1xx, I1xy, I1yy), "deriv_all")


@pytest.mark.parametrize("w,h", SMALL + FIT_X + FIT_Y)
def test_warp_and_prepare_at_small_shapes(hm, oracle_brox, w, h):
    from hydra_mi import brox
    f = _level_fields(oracle_brox, w, h, 10)
    ref = oracle_brox.warp(*f)
    for window in (False, True):
        _same(brox.op_warp(*f, window=window), ref, ("warp", window))
    du, dv = _rand((h, w), 20, -0.5, 0.5), _rand((h, w), 21, -0.5, 0.5)
    for alpha, gamma in ((0.197, 50.0), (0.1, 100.0), (0.4, 25.0)):
        _same(brox.op_prepare(f[9], f[10], du, dv, ref, alpha, gamma),
              oracle_brox.prepare(f[9], f[10], du, dv, ref, alpha, gamma), ("prepare", alpha, gamma))


@pytest.mark.parametrize("w,h", SMALL + FIT_X + FIT_Y)
@pytest.mark.parametrize("fuse", [0, 1, 2, 5, 105, 205, 10, 210])
def test_sor_at_small_shapes(hm, oracle_brox, w, h, fuse):
    from hydra_mi import brox
    f = _level_fields(oracle_brox, w, h, 30)
    warped = oracle_brox.warp(*f)
    du, dv = _rand((h, w), 40, -0.5, 0.5), _rand((h, w), 41, -0.5, 0.5)
    coef = oracle_brox.prepare(f[9], f[10], du, dv, warped, 0.197, 50.0)
    _same(brox.op_sor(du, dv, coef, 10, fuse=fuse), oracle_brox.sor(du, dv, coef, 10), ("sor", fuse))


# ---- the whole flow over the case table ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the case's pairs and the oracle's flow of each (computed once, reused by every knob setting)"""
    from oracle import brox_oracle
    c = bc.CASES_BY_NAME[name]
    F0, F1 = bc.frames(c)
    ref = [brox_oracle.calc(F0[i], F1[i], **bc.oracle_kw(c)) for i in range(c["n"])]
    for u, v in ref:
        assert np.isfinite(u).all() and np.isfinite(v).all(), name
    return F0, F1, ref


def _flow(bf, c, F0, F1):
    if c["n"] == 1:
        u, v = bf.calc(F0[0], F1[0])
        return u[None], v[None]
    return bf.calc_batch(F0, F1)


def _check(U, V, ref, what):
    for i, (ru, rv) in enumerate(ref):
        assert np.isfinite(U[i]).all() and np.isfinite(V[i]).all(), (what, i)
        assert np.array_equal(U[i], ru) and np.array_equal(V[i], rv), (what, i)


def _handle(c):
    from hydra_mi import brox
    bf = brox.BroxOpticalFlow(c["W"], c["H"], max_batch=c["n"], **bc.create_kw(c))
    p = bc.oracle_kw(c)
    assert bf.levels() == bc.levels(c["W"], c["H"], p["scale"], p["outer"])
    for k, v in c["knobs"].items():
        bf.tune(k, v)
    return bf


@pytest.mark.parametrize("name", [c["name"] for c in bc.CASES])
def test_calc_over_the_case_table(hm, name):
    """every case at coarse_max 0, 32 and 64 (its small levels through the per-operator path, k_coarse<32> and
    k_coarse<64>): the oracle's bits, and exactly the SOR launches per level the restated plan predicts"""
    c = bc.CASES_BY_NAME[name]
    d = bc.derived(c, _cus())
    for k, v in c["expect"].items():          # the branch holds on this device's CU count too
        assert d[k] == v, (name, k, d[k], v)
    F0, F1, ref = _reference(name)
    bf = _handle(c)
    for cmax in (0, 32, 64):
        bf.tune("coarse_max", cmax)
        bf.profile(True)
        U, V = _flow(bf, c, F0, F1)
        per_level = [lv["launches"] for lv in bf.profile_levels()]
        _, total, _, _ = bf.profile_read()
        bf.profile(False)
        _check(U, V, ref, (name, cmax))
        want = bc.launches(c, _cus(), coarse_max=cmax)
        assert per_level == want, (name, cmax, per_level, want)
        assert total == sum(want), (name, cmax, total)
    bf.close()


SWEEP = [("coarse_max", 0), ("sor_fuse", 1), ("sor_fuse", 2), ("sor_fuse", 5), ("sor_threads", 256), ("sor_threads", 512),
         ("sor_fuse", 0), ("sor_threads", 1024), ("sor_deep", 0), ("sor_deep", 8), ("sor_fuse", 10), ("sor_threads", 0),
         ("sor_deep", 1), ("sor_wide", 64), ("sor_wide", 0), ("warp_window", 1), ("warp_window", 0), ("coarse_max", 32)]


@pytest.mark.parametrize("name", [c["name"] for c in bc.CASES if c["sweep"]])
def test_knob_sweep_at_the_new_shapes(hm, name):
    """the sweep of test_calc_batch_and_tuning_do_not_change_results at the fits-x-only / fits-y-only shapes and the
    wide tile: every setting the oracle's bits"""
    c = bc.CASES_BY_NAME[name]
    F0, F1, ref = _reference(name)
    bf = _handle(c)
    for key, val in SWEEP:
        bf.tune(key, val)
        U, V = _flow(bf, c, F0, F1)
        _check(U, V, ref, (name, key, val))
    bf.close()


@pytest.mark.parametrize("name", ["last_1x_2y:K10:73x74", "wide_fit_x:100x300", "small:5x5"])
def test_omega(hm, oracle_brox, name):
    """hm_brox_set_omega reaches k_sor and k_coarse: omega 1.0 and 1.5 give the oracle's flow at that omega (and not
    the flow at the default 1.99)"""
    c = bc.CASES_BY_NAME[name]
    F0, F1, ref199 = _reference(name)
    bf = _handle(c)
    for om in (1.0, 1.5):
        oracle_brox.set_omega(om)
        try:
            ref = [oracle_brox.calc(F0[i], F1[i], **bc.oracle_kw(c)) for i in range(c["n"])]
        finally:
            oracle_brox.set_omega(1.99)
        assert not all(np.array_equal(r[0], q[0]) for r, q in zip(ref, ref199)), (name, om)
        bf.set_omega(om)
        for cmax in (0, 32, 64):
            bf.tune("coarse_max", cmax)
            U, V = _flow(bf, c, F0, F1)
            _check(U, V, ref, (name, om, cmax))
    bf.set_omega(1.99)
    U, V = _flow(bf, c, F0, F1)
    _check(U, V, ref199, (name, 1.99))
    bf.close()


# ---- a pyramid level of one pixel: refused before anything runs ------------------------------------------------
@pytest.mark.parametrize("W,H,scale,level", [(1, 1, 0.8, 0), (64, 64, 0.01, 1)])
def test_one_pixel_level_is_refused(hm, tmp_path, W, H, scale, level):
    from hydra_mi import brox
    with pytest.raises(RuntimeError, match="level %d is 1x1" % level):
        brox.BroxOpticalFlow(W, H, scale_factor=scale)
    # the flow tool on such a video: a nonzero exit, no flow files
    vid = str(tmp_path / "video.npy")
    np.save(vid, np.random.default_rng(0).integers(0, 256, (3, H, W)).astype(np.uint8))
    prefix = str(tmp_path / "flow")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "optical_flow_ext.py"), vid, prefix, "0.197", "50",
                        str(scale)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "level %d is 1x1" % level in r.stderr, (r.returncode, r.stderr[-500:])
    assert not os.path.exists(prefix + "_000_x.mat")
