"""The smooth sub-pixel shift field of the stabiliser on the CPU: the restatement (tests/stabfield_ref.py) against hand-made
cases, hydra_mi.stabilize(mode="field") driven by the restatement's sums against the restatement bit for bit, and the
recovery on the planted video with a smooth sub-pixel residual motion, beside the patches.

The constants below were measured with this file's own test (it prints the whole table), seeds 0-5, B = 16, S = 3, one
pass, worst of the 12 cells, traces by roi_ref.extract(thr=0.47, alpha=1.0) as in tests/test_stab_cpu.py.  Columns: clean,
jittered, then for min_score at the default (0.57) and at 0: patch shifts, the field at whole pixels, the field with the
sub-pixel estimate.

  stabfield_ref.smooth_jittered_video (smooth, sub-pixel: what the tracker leaves)
  seed  clean   jittered  patch   field   field+sub   patch   field   field+sub
  0     0.9919  0.8465    0.9237  0.9804  0.9827      0.9523  0.9831  0.9895
  1     0.9900  0.8493    0.9494  0.9731  0.9758      0.9579  0.9855  0.9896
  2     0.9897  0.8221    0.9523  0.9790  0.9841      0.9460  0.9859  0.9886
  3     0.9888  0.8513    0.8194  0.9801  0.9827      0.9536  0.9808  0.9876
  4     0.9900  0.6631    0.9132  0.9717  0.9793      0.9116  0.9789  0.9878
  5     0.9923  0.8825    0.9486  0.9851  0.9860      0.9562  0.9876  0.9895

  stab_ref.jittered_video (whole pixels, constant per region, hard seams: where the patches are the right choice; nothing is
  asserted for the field here)
  0     0.9919  0.3403    0.9746  0.9610  0.9625      0.9796  0.9421  0.9428
  1     0.9900  0.3941    0.9492  0.9768  0.9771      0.9878  0.9665  0.9677
  2     0.9897  0.3288    0.9498  0.9817  0.9817      0.9746  0.9752  0.9762
  3     0.9888  0.4458    0.9825  0.9745  0.9749      0.9793  0.9169  0.9168
  4     0.9900  0.2879    0.9725  0.9722  0.9723      0.9854  0.8585  0.8592
  5     0.9923  0.4563    0.9543  0.9761  0.9762      0.9857  0.8755  0.8766
"""
import functools

import numpy as np
import pytest

import roi_ref
import stab_ref
import stabfield_ref as ref
from test_roi_cpu import THR

TRACE_BOUND = 0.9558      # the worst cell of the field with sub-pixel on the smooth video over the six seeds at the default
#                           min_score, 0.9758, minus 0.02 (DESIGN section 10's and 13's margin for a seed)
B, S = 16, 3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _box_video(seed, F=5, H=30, W=44, box=(3, 2, 37, 25)):
    """a random video and a rectangular map c0, r0, bw, bh"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    m = np.zeros((H, W), bool)
    c0, r0, bw, bh = box
    m[r0:r0 + bh, c0:c0 + bw] = True
    return v, m


def test_a_constant_whole_pixel_q_is_the_whole_pixel_gather():
    v, m = _box_video(0)
    m[10:13, 12:15] = False                                   # a hole in the map
    rng = np.random.default_rng(1)
    for Bp in (4, 7, 16):
        npatch = stab_ref.patch_grid(m, Bp)["npx"] * stab_ref.patch_grid(m, Bp)["npy"]
        sh = np.repeat(rng.integers(-3, 4, (v.shape[0], 1, 2)), npatch, 1).astype(np.int8)
        one = np.ones(sh.shape[:2], np.uint8)
        got = ref.warp(v, m, Bp, 16 * sh.astype(np.int16), one)
        assert np.array_equal(got, stab_ref.shift(v, m, Bp, sh)) and not got[:, ~m].any()
        assert np.array_equal(ref.field_sums(v, m, Bp, 16 * sh.astype(np.int16), one), stab_ref.frame_sums(v, m, Bp, sh))
    # whole-pixel shifts that differ between the patches: the same gather wherever the four patches a pixel sees agree
    sh = rng.integers(-2, 3, (v.shape[0], npatch, 2)).astype(np.int8)
    got, want = ref.warp(v, m, 16, 16 * sh.astype(np.int16), np.ones(sh.shape[:2], np.uint8)), stab_ref.shift(v, m, 16, sh)
    assert np.array_equal(got[:, 2:10, 3:11], want[:, 2:10, 3:11])           # the first half patch of both axes: one patch


def test_the_field_between_two_patches_is_linear_and_hits_each_q_at_its_centre():
    v, m = _box_video(2, box=(3, 2, 32, 10))                  # two patches of 16 in a row, one patch row
    q = np.array([[-32, 16], [64, 48]], np.int16)
    d = ref.field(m, 16, q, np.ones(2, np.uint8))
    assert d.shape == (10, 32, 2)
    assert (d == d[:1]).all()                                 # one patch row: constant along y
    x = np.arange(32)
    assert (d[0, :8] == q[0]).all() and (d[0, 24:] == q[1]).all()            # constant in the first and last half patch
    # the centres of the patches lie at x = 7.5 and 23.5: between them q0 + (q1 - q0)(2x + 1 - 16) / 32, rounded half up
    for c in range(2):
        want = np.floor((2 * (int(q[0, c]) * (32 - (2 * x[8:24] - 15)) + int(q[1, c]) * (2 * x[8:24] - 15)) + 32) / 64.0)
        assert np.array_equal(d[0, 8:24, c], want.astype(np.int64))
        assert (np.diff(d[0, 8:24, c], 2) == 0).all() or np.abs(np.diff(d[0, 8:24, c], 2)).max() <= 1   # linear up to rounding
    assert np.array_equal(d[0, 7], q[0]) and np.array_equal(d[0, 24], q[1])
    assert np.array_equal(d[0, 15] + d[0, 16], q[0].astype(np.int64) + q[1])  # symmetric about the seam


def test_an_invalid_patch_takes_its_neighbours_value_and_an_all_invalid_frame_is_unchanged():
    v, m = _box_video(3, box=(3, 2, 32, 10))
    q = np.array([[[-32, 16], [200, -200]], [[5, 5], [7, 7]]], np.int16)
    valid = np.array([[1, 0], [0, 0]], np.uint8)
    d = ref.field(m, 16, q[0], valid[0])
    assert (d[:, :24] == q[0, 0]).all()                       # the invalid patch does not pull the field to zero ...
    assert not d[:, 24:].any()                                # ... but past the centre of a border patch it is alone: den = 0
    assert not ref.field(m, 16, q[1], valid[1]).any()
    got = ref.warp(v[:2], m, 16, q, valid)
    assert np.array_equal(got[1], np.where(m, v[1], 0))
    const = ref.warp(v[:1], m, 16, np.repeat(q[:1, :1], 2, 1), np.ones((1, 2), np.uint8))[0]
    assert np.array_equal(got[0, :, :3 + 24], const[:, :3 + 24]) and np.array_equal(got[0, :, 3 + 24:], np.where(m, v[0], 0)[:, 3 + 24:])
    # an invalid patch between two valid ones: the field runs from one neighbour to the other across it
    v, m = _box_video(3, box=(3, 2, 40, 8))                   # five patches of 8
    q5 = np.array([[0, 0], [16, -16], [200, 200], [48, -48], [0, 0]], np.int16)
    d = ref.field(m, 8, q5, np.array([1, 1, 0, 1, 1], np.uint8))
    assert (d[0, 12:20] == q5[1]).all() and (d[0, 20:28] == q5[3]).all()      # either side of its centre: the neighbour alone


def test_a_single_patch_per_axis():
    for box, Bp, grid in (((3, 2, 32, 10), 16, (2, 1)), ((3, 2, 10, 25), 16, (1, 2)), ((3, 2, 11, 9), 64, (1, 1))):
        v, m = _box_video(4, box=box)
        g = stab_ref.patch_grid(m, Bp)
        assert (g["npx"], g["npy"]) == grid
        npatch = grid[0] * grid[1]
        q = np.arange(2 * npatch, dtype=np.int16).reshape(npatch, 2) * 9 - 5
        d = ref.field(m, Bp, q, np.ones(npatch, np.uint8))
        if grid[0] == 1:
            assert (d == d[:, :1]).all()                      # constant along x
        if grid[1] == 1:
            assert (d == d[:1]).all()
        if npatch == 1:
            assert (d == q[0]).all()
        else:
            assert np.array_equal(d[0, 0], q[0]) and np.array_equal(d[-1, -1], q[-1])


def test_negative_q_rounds_by_floor_and_the_sample_is_bilinear():
    v, m = _box_video(5, F=1, box=(3, 2, 32, 10))
    one = np.ones(2, np.uint8)
    # halfway between -1 and 0 at x = 15 | 16: (2 num + den) / (2 den) with num / den = -17/32 and -15/32 -> -1 and 0
    d = ref.field(m, 16, np.array([[-1, -1], [0, 0]], np.int16), one)
    assert d[0, 15, 0] == -1 and d[0, 16, 0] == 0
    d = ref.field(m, 16, np.array([[-3, 0], [-2, 0]], np.int16), one)       # -2.5 rounds up to -2 (floor of -2.5 + 0.5)
    assert d[0, 15, 0] == -3 and d[0, 16, 0] == -2 and (d[0, :, 0] >= -3).all() and (d[0, :, 0] <= -2).all()
    # a constant q of (-5, 19): x0 = x - 1, fx = 11, y0 = y + 1, fy = 3
    q = np.array([[[-5, 19], [-5, 19]]], np.int16)
    got = ref.warp(v, m, 16, q, np.ones((1, 2), np.uint8))[0]
    box = np.zeros((13, 34), np.int64)                        # the box with a margin of zeros (two rows below)
    box[1:11, 1:33] = v[0, 2:12, 3:35]
    for y, x in ((0, 0), (4, 17), (9, 31), (8, 0), (9, 5)):
        a, b_, c, e = box[y + 2, x], box[y + 2, x + 1], box[y + 3, x], box[y + 3, x + 1]
        assert got[2 + y, 3 + x] == (5 * 13 * a + 11 * 13 * b_ + 5 * 3 * c + 11 * 3 * e + 128) >> 8
    assert not got[~m].any()


def test_the_parabola_on_a_hand_made_score_table(hm):
    from hydra_mi import stabilize
    S1 = 2                                                    # 5 x 5 shifts, index (dy + 2) 5 + dx + 2
    inf = np.inf
    sc = np.full((1, 6, 25), 0.1)
    sh = np.zeros((1, 6, 2), np.int8)
    fb = np.zeros((1, 6), bool)
    # patch 0: winner (0, 0) 0.9, x neighbours 0.5 | 0.7, y neighbours 0.8 | 0.8
    sc[0, 0, 12], sc[0, 0, 11], sc[0, 0, 13], sc[0, 0, 7], sc[0, 0, 17] = 0.9, 0.5, 0.7, 0.8, 0.8
    # patch 1: winner (2, -1) at the border of the search along x; y neighbours 0.2 | 0.85
    sh[0, 1] = (2, -1)
    sc[0, 1, 9], sc[0, 1, 8], sc[0, 1, 4], sc[0, 1, 14] = 0.9, 0.89, 0.2, 0.85
    # patch 2: winner (-1, 1) with an invalid x neighbour; along y den >= 0 (a flat top: ties)
    sh[0, 2] = (-1, 1)
    sc[0, 2, 16], sc[0, 2, 15], sc[0, 2, 17], sc[0, 2, 11], sc[0, 2, 21] = 0.9, -inf, 0.5, 0.9, 0.9
    # patch 3: a fallback, whatever its scores
    fb[0, 3] = True
    sc[0, 3, 12], sc[0, 3, 11], sc[0, 3, 13] = 0.5, 0.1, 0.4
    # patch 4 (numbers exact in binary): along x a tie with the left neighbour, off = 0.5 / -1.0 = -0.5 exactly and
    # 16 off + 0.5 = -7.5 -> -8; along y a neighbour above the "winner" (no choice of the product's, but defined): off = -1.5,
    # clipped to -0.5
    sc[0, 4, 12], sc[0, 4, 11], sc[0, 4, 13], sc[0, 4, 7], sc[0, 4, 17] = 0.75, 0.75, 0.25, 1.0, 0.25
    # patch 5: negative winner shift with a negative offset: floor, not truncation
    sh[0, 5] = (-1, 0)
    sc[0, 5, 11], sc[0, 5, 10], sc[0, 5, 12] = 0.9, 0.8, 0.3
    # patch 0 x: den = 0.5 - 1.8 + 0.7 = -0.6, off = -0.2 / -1.2 = 0.167, floor(2.67 + 0.5) = 3; y: off = 0
    # patch 1 y: den = 0.2 - 1.8 + 0.85 = -0.75, off = -0.65 / -1.5 = 0.433, floor(6.93 + 0.5) = 7: -16 + 7
    # patch 5 x: den = 0.8 - 1.8 + 0.3 = -0.7, off = 0.5 / -1.4 = -0.357, floor(-5.71 + 0.5) = -6: -16 - 6
    want = np.array([[(3, 0), (32, -9), (-16, 16), (0, 0), (-8, -8), (-22, 0)]], np.int16)
    for fn in (ref.subpixel, stabilize.subpixel):
        got = fn(sc, sh, fb, S1)
        assert got.dtype == np.int16 and np.array_equal(got, want), fn.__module__
        assert not fn(sc[:, :1], sh[:, :1], fb[:, :1], 0).any()             # S = 0: nothing to refine with


@pytest.mark.parametrize("Bp, Sp, passes", [(4, 1, 1), (7, 1, 2), (16, 3, 2), (5, 2, 3)])
def test_estimate_field_equals_the_restatement(hm, Bp, Sp, passes):
    """hydra_mi.stabilize.estimate(mode="field") on the restatement's sums against the restatement's own estimate: q, valid,
    shifts, scores (bit for bit), fallbacks and templates, also in blocks; mode="patch" is as it was."""
    from hydra_mi import stabilize
    rng = np.random.default_rng(7)
    H, W = 28, 34
    base = rng.integers(0, 256, (H + 8, W + 8)).astype(np.float64)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4        # a little smooth
    v = np.empty((9, H, W), np.uint8)
    for k in range(9):                                        # sub-pixel moves of one texture, and noise
        fx, fy = (k % 4) / 4.0, (k % 3) / 3.0
        f = base[4:4 + H, 4:4 + W] * (1 - fx) * (1 - fy) + base[4:4 + H, 5:5 + W] * fx * (1 - fy) + \
            base[5:5 + H, 4:4 + W] * (1 - fx) * fy + base[5:5 + H, 5:5 + W] * fx * fy
        v[k] = np.clip(np.rint(f + rng.integers(-3, 4, (H, W))), 0, 255)
    m = np.zeros((H, W), bool)
    m[2:25, 3:31] = True
    m[2:6, 3:7] = False
    want = ref.estimate(v, m, Bp, Sp, 1, passes, 0.3, 3, mode="field")
    old = stabilize.MATCH_BYTES
    for budget in (old, 1):                                   # one block, and a frame per block
        stabilize.MATCH_BYTES = budget
        try:
            got = stabilize.estimate(ref.RefBody(v, m), Bp, Sp, 1, passes, 0.3, 3, mode="field")
        finally:
            stabilize.MATCH_BYTES = old
        assert got["mode"] == "field" and got["q"].dtype == np.int16 and got["valid"].dtype == np.uint8
        assert np.array_equal(got["q"], want["q"]) and np.array_equal(got["valid"], want["valid"])
        assert np.array_equal(got["shifts"], want["shifts"]) and np.array_equal(got["fallback"], want["fallback"])
        assert np.array_equal(_bits(got["score"]), _bits(want["score"])) and np.array_equal(got["n_core"], want["n_core"])
        assert len(got["templates"]) == passes and all(np.array_equal(a, c) for a, c in zip(got["templates"], want["templates"]))
    assert (got["q"] % 16).any() and got["valid"].any() and np.array_equal(got["valid"], ~got["fallback"])
    body = ref.RefBody(v, m)
    est = stabilize.stabilize(body, B=Bp, S=Sp, k_ref=1, passes=passes, min_score=0.3, n_min=3, mode="field")
    assert np.array_equal(est["q"], want["q"]) and np.array_equal(body.regs, ref.warp(v, m, Bp, want["q"], want["valid"]))
    # the default mode: today's keys, today's result, and apply gathers whole pixels
    body = ref.RefBody(v, m)
    patch = stabilize.stabilize(body, B=Bp, S=Sp, k_ref=1, passes=passes, min_score=0.3, n_min=3)
    old_way = stab_ref.estimate(v, m, Bp, Sp, 1, passes, 0.3, 3)
    assert sorted(patch) == ["B", "S", "fallback", "grid", "n_core", "score", "shifts", "templates"]
    assert np.array_equal(patch["shifts"], old_way["shifts"]) and np.array_equal(body.regs, stab_ref.shift(v, m, Bp, old_way["shifts"]))
    with pytest.raises(ValueError, match="mode 'smooth'"):
        stabilize.estimate(ref.RefBody(v, m), mode="smooth")


def test_the_smooth_jitter_is_what_it_says():
    jit, clean, cs, act, d = ref.smooth_jittered_video(0)
    F, H, W = clean.shape
    assert d.shape == (F, H, W, 2) and np.array_equal(jit[0], clean[0]) and not d[0].any()
    assert np.abs(d).max() <= ref.AMP and np.abs(d).max() > 1.0 and np.abs(np.diff(d, axis=0)).max() <= ref.STEP
    assert np.abs(np.diff(d, axis=2)).max() < 0.2 and np.abs(np.diff(d, axis=1)).max() < 0.2       # smooth: no seams
    nodes_x, nodes_y = np.linspace(0, W - 1, ref.GRID_X), np.linspace(0, H - 1, ref.GRID_Y)
    k, y, x = 40, 60, 50                                      # bilinear between the four nodes round it
    jx, jy = np.searchsorted(nodes_x, x) - 1, np.searchsorted(nodes_y, y) - 1
    tx, ty = (x - nodes_x[jx]) / (nodes_x[jx + 1] - nodes_x[jx]), (y - nodes_y[jy]) / (nodes_y[jy + 1] - nodes_y[jy])
    rng = np.random.default_rng((0, 77))
    steps = rng.uniform(-ref.STEP, ref.STEP, (F, ref.GRID_Y, ref.GRID_X, 2))
    walk = np.zeros_like(steps)
    for i in range(1, F):
        walk[i] = np.clip(walk[i - 1] + steps[i], -ref.AMP, ref.AMP)
    want = (walk[k, jy, jx] * (1 - tx) + walk[k, jy, jx + 1] * tx) * (1 - ty) + (walk[k, jy + 1, jx] * (1 - tx) + walk[k, jy + 1, jx + 1] * tx) * ty
    assert np.allclose(d[k, y, x], want, rtol=0, atol=1e-12)
    sx, sy = x - d[k, y, x, 0], y - d[k, y, x, 1]
    x0, y0 = int(np.floor(sx)), int(np.floor(sy))
    fx, fy = sx - x0, sy - y0
    c = clean[k].astype(np.float64)
    val = (c[y0, x0] * (1 - fx) + c[y0, x0 + 1] * fx) * (1 - fy) + (c[y0 + 1, x0] * (1 - fx) + c[y0 + 1, x0 + 1] * fx) * fy
    assert abs(int(jit[k, y, x]) - val) <= 0.5 + 1e-9


class _CachedBody(ref.RefBody):
    """the restatement's sums of one pass over one video, kept for the second min_score"""
    sums = None

    def body_rec_match(self, template, B, S, k0=0, n=None, want=("A", "V1", "V2")):
        key = (np.asarray(template).tobytes(), B, S, k0, n)
        if self.sums is None or self.sums[0] != key:
            self.sums = (key, super().body_rec_match(template, B, S, k0, n))
        return self.sums[1]


def _worst(v, m, cs, act):
    e = roi_ref.extract(v, m, cs, thr=THR, alpha=1.0)
    F_c = e["F_roi"] - e["F_np"]
    return min(np.corrcoef(F_c[:, s], act[s])[0, 1] for s in range(12))


@functools.lru_cache(maxsize=None)
def _row(video, seed):
    """-> (clean, jittered, then per min_score (default, 0): patch, field at whole pixels, field with sub-pixel)"""
    from hydra_mi import stabilize
    jit, clean, cs, act = (ref.smooth_jittered_video if video == "smooth" else stab_ref.jittered_video)(seed)[:4]
    m = roi_ref.planted_map()
    row = [_worst(clean, m, cs, act), _worst(jit, m, cs, act)]
    sums = None
    for min_score in (None, 0.0):
        body = _CachedBody(jit, m)
        body.sums = sums
        est = stabilize.estimate(body, B=B, S=S, min_score=min_score, mode="field")
        sums = body.sums
        one = stab_ref.estimate(jit[:3], m, B, S, min_score=stabilize.DEFAULT_MIN_SCORE if min_score is None else 0.0)
        assert np.array_equal(est["shifts"][:3], one["shifts"])             # the whole-pixel part is the patch mode's
        row += [_worst(stab_ref.shift(body.regs, m, B, est["shifts"]), m, cs, act),
                _worst(ref.warp(body.regs, m, B, 16 * est["shifts"].astype(np.int16), est["valid"]), m, cs, act),
                _worst(ref.warp(body.regs, m, B, est["q"], est["valid"]), m, cs, act)]
    return tuple(row)


@pytest.mark.parametrize("seed", range(6))
def test_the_field_cures_smooth_sub_pixel_jitter_better_than_the_patches(hm, seed):
    """The worst cell's trace against the planted activity on the smooth video, and (nothing asserted for the field) on
    stab_ref.jittered_video, whose regions move rigidly with hard seams: the table of DESIGN section 13."""
    from hydra_mi import stabilize
    assert stabilize.DEFAULT_MIN_SCORE == 0.57
    smooth, seams = _row("smooth", seed), _row("seams", seed)
    for name, row in (("smooth", smooth), ("seams", seams)):
        print("%s seed %d: clean %.4f, jittered %.4f; min_score 0.57: patch %.4f, field %.4f, field + sub-pixel %.4f; "
              "min_score 0: patch %.4f, field %.4f, field + sub-pixel %.4f" % ((name, seed) + row))
    assert smooth[4] >= TRACE_BOUND
    assert smooth[4] >= smooth[2] and smooth[7] >= smooth[5]  # a condition, not a measurement: no worse than the patches
