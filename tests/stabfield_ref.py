"""NumPy restatement of the smooth sub-pixel shift field of the stabiliser (include/hydra_mi.h: hm_body_rec_warp /
_field_sums; hydra_mi.stabilize mode="field"): the sub-pixel estimate from the score table, the field between the patch
centres, the bilinear sample, the estimate built on them, and the planted video with a smooth sub-pixel residual motion
that the recovery tests run on.  It imports stab_ref and changes nothing in it.

`q` is (F, patches, 2) int16 (dx, dy) in 1/16 px, `valid` (F, patches); everything after the score table is exact
integers (int64 here, floor division by //).
"""
import math

import numpy as np

import roi_ref
import stab_ref


# ---- the sub-pixel estimate ---------------------------------------------------------------------------------------------
def score_table(ms, St, Stt):
    """-> (n, patches, (2S+1)^2) float64: the normalised correlation of stab_ref.choose for every shift, -inf: invalid"""
    A, V1, V2, nc = (ms[k].astype(np.int64) for k in ("A", "V1", "V2", "n_core"))
    n, npatch, nsh = A.shape
    var_t = (nc * Stt - St * St).astype(np.float64)
    out = np.full((n, npatch, nsh), -np.inf)
    for s in range(nsh):
        cov = (nc[None] * A[:, :, s] - V1[:, :, s] * St[None]).astype(np.float64)
        var_v = (nc[None] * V2[:, :, s] - V1[:, :, s] * V1[:, :, s]).astype(np.float64)
        valid = (var_v > 0) & (var_t[None] > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, :, s] = np.where(valid, cov / np.sqrt(var_v * var_t[None]), -np.inf)
    return out


def subpixel(sc, shifts, fallback, S):
    """One (frame, patch, axis) at a time -> q (n, patches, 2) int16"""
    n1 = 2 * S + 1
    n, npatch, _ = sc.shape
    q = np.zeros((n, npatch, 2), np.int16)
    for k in range(n):
        for p in range(npatch):
            if fallback[k, p]:
                continue
            d = (int(shifts[k, p, 0]), int(shifts[k, p, 1]))
            idx = (d[1] + S) * n1 + d[0] + S
            s0 = float(sc[k, p, idx])
            for axis, step in ((0, 1), (1, n1)):
                off = 0.0
                if abs(d[axis]) < S:
                    lo, hi = float(sc[k, p, idx - step]), float(sc[k, p, idx + step])
                    if lo > -math.inf and hi > -math.inf:
                        den = (lo - 2.0 * s0) + hi
                        if den < 0.0:
                            off = (lo - hi) / (2.0 * den)
                            off = min(max(off, -0.5), 0.5)
                q[k, p, axis] = 16 * d[axis] + math.floor(16.0 * off + 0.5)
    return q


# ---- the field and the sample -------------------------------------------------------------------------------------------
def _axis(n_px, B, n_patch):
    """per box coordinate: (i, i1, w0, w1)"""
    x = np.arange(n_px, dtype=np.int64)
    u = 2 * x + 1 - B
    i = np.clip(u // (2 * B), 0, max(n_patch - 2, 0))
    w1 = np.clip(u - 2 * B * i, 0, 2 * B)
    return i, np.minimum(i + 1, n_patch - 1), 2 * B - w1, w1


def field(inmap, B, q, valid):
    """One frame: q (patches, 2), valid (patches,) -> (bh, bw, 2) int64, the shift (dx, dy) in 1/16 px of every box pixel"""
    g = stab_ref.patch_grid(inmap, B)
    npx, npy = g["npx"], g["npy"]
    ix, ix1, wx0, wx1 = _axis(g["bw"], B, npx)
    iy, iy1, wy0, wy1 = _axis(g["bh"], B, npy)
    qq = np.asarray(q).astype(np.int64).reshape(npy, npx, 2)
    vv = (np.asarray(valid).reshape(npy, npx) != 0).astype(np.int64)
    num = np.zeros((g["bh"], g["bw"], 2), np.int64)
    den = np.zeros((g["bh"], g["bw"]), np.int64)
    for jy, wy in ((iy, wy0), (iy1, wy1)):
        for jx, wx in ((ix, wx0), (ix1, wx1)):
            w = wy[:, None] * wx[None, :] * vv[jy[:, None], jx[None, :]]
            num += w[:, :, None] * qq[jy[:, None], jx[None, :]]
            den += w
    safe = np.maximum(den, 1)
    return np.where(den[:, :, None] > 0, (2 * num + den[:, :, None]) // (2 * safe[:, :, None]), 0)


def _tap(box, ys, xs):
    """box (bh, bw) int64 at integer (ys, xs), 0 off the box"""
    bh, bw = box.shape
    on = (ys >= 0) & (ys < bh) & (xs >= 0) & (xs < bw)
    return np.where(on, box[np.clip(ys, 0, bh - 1), np.clip(xs, 0, bw - 1)], 0)


def warp(regs, inmap, B, q, valid):
    """-> (F, H, W) uint8: every map pixel of every frame sampled bilinearly at its frame's field, 0 off the map"""
    m = np.asarray(inmap, bool)
    regs = np.asarray(regs)
    g = stab_ref.patch_grid(m, B)
    r0, c0, bh, bw = g["r0"], g["c0"], g["bh"], g["bw"]
    mb = m[r0:r0 + bh, c0:c0 + bw]
    yy, xx = np.mgrid[0:bh, 0:bw]
    out = np.zeros(regs.shape, np.uint8)
    for k in range(regs.shape[0]):
        box = np.where(mb, regs[k, r0:r0 + bh, c0:c0 + bw], 0).astype(np.int64)
        d = field(m, B, q[k], valid[k])
        X, Y = 16 * xx + d[:, :, 0], 16 * yy + d[:, :, 1]
        x0, y0, fx, fy = X >> 4, Y >> 4, X & 15, Y & 15
        v = ((16 - fx) * (16 - fy) * _tap(box, y0, x0) + fx * (16 - fy) * _tap(box, y0, x0 + 1) +
             (16 - fx) * fy * _tap(box, y0 + 1, x0) + fx * fy * _tap(box, y0 + 1, x0 + 1) + 128) >> 8
        out[k, r0:r0 + bh, c0:c0 + bw] = np.where(mb, v, 0)
    return out


def field_sums(regs, inmap, B, q, valid):
    """-> (H, W) uint32: the sum over the frames of warp"""
    s = warp(regs, inmap, B, q, valid).astype(np.int64).sum(0)
    assert s.max(initial=0) < 2 ** 32
    return s.astype(np.uint32)


# ---- the estimate -------------------------------------------------------------------------------------------------------
def estimate(regs, inmap, B=16, S=3, k_ref=0, passes=1, min_score=0.0, n_min=None, mode="patch"):
    """hydra_mi.stabilize.estimate(mode=...) on a registered video -> stab_ref.estimate's dict, in field mode with q and
    valid"""
    if mode == "patch":
        return stab_ref.estimate(regs, inmap, B, S, k_ref, passes, min_score, n_min)
    m = np.asarray(inmap, bool)
    regs = np.where(m[None], np.asarray(regs), 0).astype(np.uint8)
    F = regs.shape[0]
    n_min = B * B / 4 if n_min is None else n_min
    template = regs[k_ref]
    templates = []
    for p in range(passes):
        if p > 0:
            sums = field_sums(regs, m, B, out["q"], out["valid"]).astype(np.int64)
            template = ((2 * sums + F) // (2 * F)).astype(np.uint8)
        templates.append(template)
        ms = stab_ref.match(regs, m, B, S, template)
        St, Stt = stab_ref.template_sums(template, m, B, S)
        sh, sc, fb = stab_ref.choose(ms, St, Stt, S, min_score, n_min)
        q = subpixel(score_table(ms, St, Stt), sh, fb, S)
        out = dict(shifts=sh, score=sc, fallback=fb, n_core=ms["n_core"], templates=templates, q=q, valid=(~fb).astype(np.uint8))
    return out


class RefBody(stab_ref.RefBody):
    """stab_ref.RefBody that also answers the two calls of the field mode"""

    def body_rec_field_sums(self, q, valid, B, k0=0, n=None):
        n = self.regs.shape[0] - k0 if n is None else n
        return field_sums(self.regs[k0:k0 + n], self.inmap, B, q, valid)

    def body_rec_warp(self, q, valid, B):
        self.regs = warp(self.regs, self.inmap, B, q, valid)


# ---- the planted video with a smooth sub-pixel residual motion ------------------------------------------------------------
GRID_X, GRID_Y = 5, 4                  # the control grid: nodes spread evenly from the first to the last column and row
STEP, AMP = 0.7, 2.0                   # px


def smooth_motion(seed, F, H, W):
    """-> (F, H, W, 2) float64 (dx, dy): every node of the control grid walks on its own (steps uniform in +-STEP per
    axis and frame from one default_rng((seed, 77)), drawn as (F, GRID_Y, GRID_X, 2); clipped at +-AMP; frame 0 unshifted),
    bilinear between the nodes"""
    rng = np.random.default_rng((seed, 77))
    steps = rng.uniform(-STEP, STEP, (F, GRID_Y, GRID_X, 2))
    d = np.zeros((F, GRID_Y, GRID_X, 2))
    for k in range(1, F):
        d[k] = np.clip(d[k - 1] + steps[k], -AMP, AMP)
    gx = np.arange(W) * (GRID_X - 1) / (W - 1)
    gy = np.arange(H) * (GRID_Y - 1) / (H - 1)
    jx, jy = np.minimum(gx.astype(int), GRID_X - 2), np.minimum(gy.astype(int), GRID_Y - 2)
    tx, ty = (gx - jx)[None, None, :, None], (gy - jy)[None, :, None, None]
    top = d[:, jy][:, :, jx] * (1 - tx) + d[:, jy][:, :, jx + 1] * tx
    bot = d[:, jy + 1][:, :, jx] * (1 - tx) + d[:, jy + 1][:, :, jx + 1] * tx
    return top * (1 - ty) + bot * ty


def smooth_jittered_video(seed):
    """roi_ref.planted_video(seed) with a smooth sub-pixel jitter: a pixel p takes the clean frame at p - d(p), sampled
    bilinearly (coordinates clipped to the frame) and rounded
    -> (jittered video, clean video, centres, activity, motion (F, H, W, 2))"""
    v, cs, act, _ = roi_ref.planted_video(seed)
    F, H, W = v.shape
    d = smooth_motion(seed, F, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty_like(v)
    for k in range(F):
        sx = np.clip(xx - d[k, :, :, 0], 0, W - 1)
        sy = np.clip(yy - d[k, :, :, 1], 0, H - 1)
        x0, y0 = np.minimum(np.floor(sx).astype(int), W - 2), np.minimum(np.floor(sy).astype(int), H - 2)
        fx, fy = sx - x0, sy - y0
        f = v[k].astype(np.float64)
        val = (f[y0, x0] * (1 - fx) + f[y0, x0 + 1] * fx) * (1 - fy) + (f[y0 + 1, x0] * (1 - fx) + f[y0 + 1, x0 + 1] * fx) * fy
        out[k] = np.clip(np.rint(val), 0, 255)
    return out, v, cs, act, d


def smooth_jittered_scene(seed, uv):
    """smooth_jittered_video as the tracker sees it (stab_ref.jittered_scene's construction: roi_ref.planted_scene's two
    halves) -> (frames, states, centres, activity, the jittered video in body coordinates)"""
    j, _, cs, act, _ = smooth_jittered_video(seed)
    F = j.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = roi_ref.PLANTED_SHIFT
    frames = j.copy()
    frames[F // 2:] = np.roll(j[F // 2:], (dr, dc), axis=(1, 2))
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    states = np.array([rest if k < F // 2 else moved for k in range(F)])
    return frames, states, cs, act, j
