"""NumPy restatement of the patch sums, the sums at given shifts and the shift in place of the recorded registered video
(include/hydra_mi.h: hm_body_rec_match / _frame_sums / _shift), of the estimate built on them (hydra_mi.stabilize), and
the planted video with a planted residual motion that the recovery tests run on.

`regs` is the registered video (F, H, W) uint8, `inmap` the body map as a mask (tri_of >= 0).  A pixel outside the map
counts 0 whatever `regs` holds there, as in the record.  Shifts are (dx, dy) = (columns, rows); shift index
(dy + S)(2S + 1) + dx + S.  All sums are exact integers.
"""
import numpy as np

import roi_ref

# ---- the patch grid ---------------------------------------------------------------------------------------------------


def patch_grid(inmap, B):
    """The record's box (the bounding box of the map; one pixel at (0, 0) for an empty map) and the grid of B x B patches
    that tiles it from its top-left corner -> dict c0, r0, bw, bh, npx, npy, B"""
    m = np.asarray(inmap, bool)
    if not m.any():
        c0 = r0 = 0
        bw = bh = 1
    else:
        rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        c0, r0 = int(cols[0]), int(rows[0])
        bw, bh = int(cols[-1]) - c0 + 1, int(rows[-1]) - r0 + 1
    return dict(c0=c0, r0=r0, bw=bw, bh=bh, npx=-(-bw // B), npy=-(-bh // B), B=int(B))


def patch_index(inmap, B):
    """-> (H, W) int32: the patch of every pixel of the box (row-major), -1 outside the box"""
    m = np.asarray(inmap, bool)
    g = patch_grid(m, B)
    out = np.full(m.shape, -1, np.int32)
    yy, xx = np.mgrid[0:g["bh"], 0:g["bw"]]
    out[g["r0"]:g["r0"] + g["bh"], g["c0"]:g["c0"] + g["bw"]] = (yy // B) * g["npx"] + xx // B
    return out


def core_mask(inmap, S):
    """-> (H, W) bool: the pixels p for which every p + d, |dx| <= S and |dy| <= S, is on the frame and in the map"""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    out = m.copy()
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            sh = np.zeros((H, W), bool)
            sh[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = m[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
            out &= sh
    return out


def _per_patch(x, pp, npatch):
    """x (n, pixels) int64, pp the patch of every pixel -> (n, npatch) sums"""
    order = np.argsort(pp, kind="stable")
    cs = np.concatenate((np.zeros((x.shape[0], 1), np.int64), np.cumsum(x[:, order], 1)), 1)
    ends = np.searchsorted(pp[order], np.arange(npatch), side="right")
    starts = np.searchsorted(pp[order], np.arange(npatch), side="left")
    return cs[:, ends] - cs[:, starts]


def match(regs, inmap, B, S, template, k0=0, n=None):
    """-> dict: n_core (patches,) uint32; A, V1, V2 (n, patches, (2S+1)^2) uint32: the sums over every patch's core of
    v_k(p + d) t(p), v_k(p + d) and v_k(p + d)^2 for the frames k0 .. k0 + n - 1"""
    m = np.asarray(inmap, bool)
    regs = np.asarray(regs)
    H, W = m.shape
    n = regs.shape[0] - k0 if n is None else n
    g = patch_grid(m, B)
    c0, r0, bw, bh, npx, npy = (g[key] for key in ("c0", "r0", "bw", "bh", "npx", "npy"))
    n1 = 2 * S + 1
    v = np.zeros((n, H + 2 * S, W + 2 * S), np.int32)                # the frames with a margin of S zeros
    v[:, S:S + H, S:S + W] = np.where(m[None], regs[k0:k0 + n], 0)
    core = np.zeros((npy * B, npx * B), np.int32)                     # the box, filled up to whole patches
    core[:bh, :bw] = core_mask(m, S)[r0:r0 + bh, c0:c0 + bw]
    t = np.zeros((npy * B, npx * B), np.int32)
    t[:bh, :bw] = np.asarray(template)[r0:r0 + bh, c0:c0 + bw]
    t *= core

    def per_patch(x):
        return x.reshape(n, npy, B, npx, B).sum((2, 4), dtype=np.int64).reshape(n, npy * npx)

    out = dict(n_core=per_patch(np.broadcast_to(core, (n,) + core.shape))[0].astype(np.uint32) if n else
               core.reshape(npy, B, npx, B).sum((1, 3)).reshape(-1).astype(np.uint32))
    A, V1, V2 = (np.zeros((n, npy * npx, n1 * n1), np.int64) for _ in range(3))
    x = np.zeros((n, npy * B, npx * B), np.int32)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            s = (dy + S) * n1 + dx + S
            x[:, :bh, :bw] = v[:, S + r0 + dy:S + r0 + dy + bh, S + c0 + dx:S + c0 + dx + bw]
            xc = x * core
            A[:, :, s], V1[:, :, s], V2[:, :, s] = per_patch(x * t), per_patch(xc), per_patch(xc * x)
    assert max(A.max(initial=0), V2.max(initial=0)) < 2 ** 32
    out.update(A=A.astype(np.uint32), V1=V1.astype(np.uint32), V2=V2.astype(np.uint32))
    return out


def shift(regs, inmap, B, shifts):
    """shifts (F, patches, 2) (dx, dy) -> (F, H, W) uint8: v'_k(p) = v_k(p + d_k,patch(p)) where p and p + d are in the
    map (and so in the box), else 0"""
    m = np.asarray(inmap, bool)
    regs = np.asarray(regs)
    F, H, W = regs.shape
    sh = np.asarray(shifts).astype(np.int64)
    ys, xs = np.nonzero(m)
    pp = patch_index(m, B)[ys, xs]
    out = np.zeros((F, H, W), np.uint8)
    for k in range(F):
        sx, sy = xs + sh[k, pp, 0], ys + sh[k, pp, 1]
        on = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        sxc, syc = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
        out[k, ys, xs] = np.where(on & m[syc, sxc], regs[k, syc, sxc], 0)
    return out


def frame_sums(regs, inmap, B, shifts=None):
    """-> (H, W) uint32: the sum over the frames of every map pixel taken at its patch's shift of that frame"""
    m = np.asarray(inmap, bool)
    regs = np.asarray(regs)
    F = regs.shape[0]
    if shifts is None:
        shifts, B = np.zeros((F, 1, 2), np.int8), 2 ** 20
    s = shift(regs, m, B, shifts).astype(np.int64).sum(0)
    assert s.max(initial=0) < 2 ** 32
    return s.astype(np.uint32)


# ---- the estimate -----------------------------------------------------------------------------------------------------
def template_sums(template, inmap, B, S):
    """-> (St, Stt) (patches,) int64: the sums of t and t^2 over every patch's core"""
    m = np.asarray(inmap, bool)
    g = patch_grid(m, B)
    rows, cols = np.nonzero(core_mask(m, S))
    pp = patch_index(m, B)[rows, cols]
    t = np.asarray(template).astype(np.int64)[rows, cols]
    npatch = g["npx"] * g["npy"]
    return _per_patch(t[None], pp, npatch)[0], _per_patch((t * t)[None], pp, npatch)[0]


def choose(ms, St, Stt, S, min_score, n_min):
    """One frame-by-patch decision at a time, the shifts walked in index order: -> (shifts (n, patches, 2) int8, score
    (n, patches) float64, NaN without a valid shift; fallback (n, patches) bool)"""
    n1 = 2 * S + 1
    A, V1, V2, nc = ms["A"].astype(np.int64), ms["V1"].astype(np.int64), ms["V2"].astype(np.int64), ms["n_core"].astype(np.int64)
    n, npatch, _ = A.shape
    shifts = np.zeros((n, npatch, 2), np.int8)
    score = np.full((n, npatch), np.nan)
    fallback = np.zeros((n, npatch), bool)
    var_t = (nc * Stt - St * St).astype(np.float64)
    best = np.full((n, npatch), -np.inf)
    best_d2 = np.zeros((n, npatch), np.int64)
    found = np.zeros((n, npatch), bool)
    for s in range(n1 * n1):
        dy, dx = s // n1 - S, s % n1 - S
        cov = (nc[None] * A[:, :, s] - V1[:, :, s] * St[None]).astype(np.float64)
        var_v = (nc[None] * V2[:, :, s] - V1[:, :, s] * V1[:, :, s]).astype(np.float64)
        valid = (var_v > 0) & (var_t[None] > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            sc = cov / np.sqrt(var_v * var_t[None])
        d2 = dx * dx + dy * dy
        take = valid & (~found | (sc > best) | ((sc == best) & (d2 < best_d2)))
        best = np.where(take, sc, best)
        best_d2 = np.where(take, d2, best_d2)
        shifts[take] = (dx, dy)
        found |= take
    score[found] = best[found]
    fallback = (nc[None] < n_min) | ~found | (np.where(found, best, 0.0) < min_score)
    shifts[fallback] = 0
    return shifts, score, fallback


def estimate(regs, inmap, B=16, S=3, k_ref=0, passes=1, min_score=0.0, n_min=None):
    """hydra_mi.stabilize.estimate on a registered video -> dict shifts, score, fallback, n_core, templates"""
    m = np.asarray(inmap, bool)
    regs = np.where(m[None], np.asarray(regs), 0).astype(np.uint8)
    F = regs.shape[0]
    n_min = B * B / 4 if n_min is None else n_min
    template = regs[k_ref]
    templates = []
    for p in range(passes):
        if p > 0:
            sums = frame_sums(regs, m, B, out["shifts"]).astype(np.int64)
            template = ((2 * sums + F) // (2 * F)).astype(np.uint8)
        templates.append(template)
        ms = match(regs, m, B, S, template)
        St, Stt = template_sums(template, m, B, S)
        sh, sc, fb = choose(ms, St, Stt, S, min_score, n_min)
        out = dict(shifts=sh, score=sc, fallback=fb, n_core=ms["n_core"], templates=templates)
    return out


class RefBody:
    """What hydra_mi.stabilize asks of a BodyReadout(keep=True), answered by the restatement: the record is `regs` with 0
    outside the map."""

    def __init__(self, regs, inmap):
        self.keep = True
        self.r = self
        self.inmap = np.asarray(inmap, bool)
        self.tri_of_pixel = np.where(self.inmap, 0, -1).astype(np.int32)
        self.regs = np.where(self.inmap[None], np.asarray(regs), 0).astype(np.uint8)

    def body_rec_count(self):
        return self.regs.shape[0]

    def body_rec_fetch(self, k0=0, n=None):
        n = self.regs.shape[0] - k0 if n is None else n
        return self.regs[k0:k0 + n].copy()

    def body_rec_match(self, template, B, S, k0=0, n=None, want=("A", "V1", "V2")):
        return match(self.regs, self.inmap, B, S, template, k0, n)

    def body_rec_frame_sums(self, shifts=None, B=16, k0=0, n=None):
        n = self.regs.shape[0] - k0 if n is None else n
        return frame_sums(self.regs[k0:k0 + n], self.inmap, B, shifts)

    def body_rec_shift(self, shifts, B):
        self.regs = shift(self.regs, self.inmap, B, shifts)


# ---- the planted video with a planted residual motion ---------------------------------------------------------------
SEAMS_X = (34, 62, 90)                 # between the cells of roi_ref.planted_video's 4 x 3 grid
SEAMS_Y = (42, 78)


def region_index(H, W):
    """-> (H, W) int: the region (row-major, 4 x 3) of every pixel"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.searchsorted(SEAMS_Y, yy, side="right") * (len(SEAMS_X) + 1) + np.searchsorted(SEAMS_X, xx, side="right")


def jittered_video(seed, amp=2):
    """roi_ref.planted_video(seed) with a whole-pixel jitter: 4 x 3 regions with seams at x = 34, 62, 90 and y = 42, 78,
    each with its own random walk (steps -1, 0, 1 per axis from its own default_rng((seed, 1000 + region)), clipped at
    +-amp), frame 0 unshifted; a pixel p of region r takes v(p - d_r) (clipped to the frame)
    -> (jittered video, clean video, centres, activity, planted (F, 12, 2) int (dx, dy): the shift that undoes it)"""
    v, cs, act, _ = roi_ref.planted_video(seed)
    F, H, W = v.shape
    reg = region_index(H, W)
    nreg = (len(SEAMS_X) + 1) * (len(SEAMS_Y) + 1)
    d = np.zeros((F, nreg, 2), np.int64)
    for r in range(nreg):
        rng = np.random.default_rng((seed, 1000 + r))
        steps = rng.integers(-1, 2, (F, 2))
        for k in range(1, F):
            d[k, r] = np.clip(d[k - 1, r] + steps[k], -amp, amp)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty_like(v)
    for k in range(F):
        sx = np.clip(xx - d[k, reg, 0], 0, W - 1)
        sy = np.clip(yy - d[k, reg, 1], 0, H - 1)
        out[k] = v[k, sy, sx]
    return out, v, cs, act, d


def jittered_scene(seed, uv, amp=2):
    """jittered_video as the tracker sees it (roi_ref.planted_scene's two halves) -> (frames, states, centres, activity,
    planted shifts, the jittered video in body coordinates)"""
    j, _, cs, act, d = jittered_video(seed, amp)
    F = j.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = roi_ref.PLANTED_SHIFT
    frames = j.copy()
    frames[F // 2:] = np.roll(j[F // 2:], (dr, dc), axis=(1, 2))
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    states = np.array([rest if k < F // 2 else moved for k in range(F)])
    return frames, states, cs, act, d, j


def whole_patches(inmap, B):
    """-> (patches,) int: the region a patch lies wholly inside, -1 when it straddles a seam"""
    m = np.asarray(inmap, bool)
    pid = patch_index(m, B)
    reg = region_index(*m.shape)
    g = patch_grid(m, B)
    out = np.full(g["npx"] * g["npy"], -1)
    for p in range(len(out)):
        r = np.unique(reg[pid == p])
        if len(r) == 1:
            out[p] = r[0]
    return out
