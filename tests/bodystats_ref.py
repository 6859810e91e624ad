"""NumPy restatement of the statistics of the registered video (include/hydra_mi.h: hm_body_stats_*; hydra_mi.body).

Sums in int64, the images in float64 with every step one rounded operation in the library's order, the peaks by brute
force; and the planted video the recovery tests run on.  `inmap` is the body map as a mask (tri_of >= 0).
"""
import numpy as np

CAP = 65536
# forward neighbours whose cross sums a pixel stores (d = 0..3), as (d_col, d_row): right, down-right, down, down-left
FORWARD = ((1, 0), (1, 1), (0, 1), (-1, 1))
# the order the correlations are added in: E, SE, S, SW, W, NW, N, NE
EIGHT = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def _shifted(a, dc, dr, fill=0):
    """b[r, c] = a[r + dr, c + dc], `fill` where that is off the frame"""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    rs, rq = slice(max(0, -dr), H - max(0, dr)), slice(max(0, dr), H - max(0, -dr))
    cs, cq = slice(max(0, -dc), W - max(0, dc)), slice(max(0, dc), W - max(0, -dc))
    out[..., rs, cs] = a[..., rq, cq]
    return out


def accumulate(regs, inmap):
    """Registered frames (F, H, W) uint8 -> (s1, s2 (H, W), cross (4, H, W), vmax (H, W)) int64; zeros outside the map."""
    v = np.asarray(regs).astype(np.int64)
    m = np.asarray(inmap, bool)
    H, W = m.shape
    if v.shape[0] == 0:
        z = np.zeros((H, W), np.int64)
        return z, z.copy(), np.zeros((4, H, W), np.int64), z.copy()
    s1 = np.where(m, v.sum(0), 0)
    s2 = np.where(m, (v * v).sum(0), 0)
    vmax = np.where(m, v.max(0), 0)
    cross = np.zeros((4, H, W), np.int64)
    for d, (dc, dr) in enumerate(FORWARD):
        both = m & _shifted(m, dc, dr, False)
        cross[d] = np.where(both, (v * _shifted(v, dc, dr)).sum(0), 0)
    return s1, s2, cross, vmax


def images(s1, s2, cross, vmax, F, inmap):
    """-> (mean, std, corr (H, W) float64, NaN outside the map; max (H, W) uint8)"""
    m = np.asarray(inmap, bool)
    Ff = np.float64(F)
    a1 = np.asarray(s1).astype(np.float64)
    var = Ff * np.asarray(s2).astype(np.float64) - a1 * a1
    mean = a1 / Ff
    std = np.sqrt(var) / Ff
    x = np.asarray(cross).astype(np.float64)
    tot = np.zeros(m.shape)
    cnt = np.zeros(m.shape, np.int64)
    for k, (dc, dr) in enumerate(EIGHT):
        # the cross sum of (p, q): stored at p for the forward neighbours, at q for the backward ones
        xc = x[k] if k < 4 else _shifted(x[k - 4], dc, dr)
        vq, bq = _shifted(var, dc, dr), _shifted(a1, dc, dr)
        ok = m & _shifted(m, dc, dr, False) & (var > 0) & (vq > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = (Ff * xc - a1 * bq) / np.sqrt(var * vq)
        tot = np.where(ok, tot + np.where(ok, rho, 0.0), tot)
        cnt += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = np.where(cnt > 0, tot / np.maximum(cnt, 1).astype(np.float64), 0.0)
    nan = np.float64("nan")
    return (np.where(m, mean, nan), np.where(m, std, nan), np.where(m, corr, nan),
            np.where(m, np.asarray(vmax), 0).astype(np.uint8))


def score_image(which, mean, std, corr, vmax):
    """0 / "corr", 1 / "std", 2 / "range" = max - mean"""
    which = {"corr": 0, "std": 1, "range": 2}.get(which, which)
    return corr if which == 0 else std if which == 1 else np.asarray(vmax).astype(np.float64) - mean


def peaks(score, inmap, radius, min_score=-np.inf):
    """Brute force over every map pixel -> (raster indices int32, scores), score descending, index ascending."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    out = []
    for r in range(H):
        for c in range(W):
            if not m[r, c]:
                continue
            s = score[r, c]
            if not s >= min_score:
                continue
            best = True
            for rq in range(max(0, r - radius), min(H, r + radius + 1)):
                for cq in range(max(0, c - radius), min(W, c + radius + 1)):
                    if not m[rq, cq] or (rq == r and cq == c):
                        continue
                    t = score[rq, cq]
                    if t > s or (t == s and rq * W + cq < r * W + c):
                        best = False
                        break
                if not best:
                    break
            if best:
                out.append((s, r * W + c))
    out.sort(key=lambda e: (-e[0], e[1]))
    return np.array([e[1] for e in out], np.int32), np.array([e[0] for e in out], np.float64)


def peaks_fast(score, inmap, radius, min_score=-np.inf):
    """The same peaks from shifted comparisons (whole images at a time): for the larger frames of the GPU tests."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    s = np.where(m, score, np.nan)
    with np.errstate(invalid="ignore"):
        keep = m & (s >= min_score)
        for dr in range(-radius, radius + 1):
            for dc in range(-radius, radius + 1):
                if dr == 0 and dc == 0:
                    continue
                t = _shifted(s, dc, dr, np.nan)
                keep &= ~((t >= s) if (dr < 0 or (dr == 0 and dc < 0)) else (t > s))
    idx = np.flatnonzero(keep.reshape(-1))
    sc = s.reshape(-1)[idx]
    order = np.lexsort((idx, -sc))
    return idx[order].astype(np.int32), sc[order].astype(np.float64)


# ---- the planted video ---------------------------------------------------------------------------------------------
PLANTED = dict(H=128, W=128, F=200, K=12, amp=70.0, noise=8, sigma=2.0)


def planted_video(seed):
    """128 x 128, 200 frames: a static random texture 40..120, 12 Gaussian cells (sigma 2 px, amplitude 70 x activity) on
    a jittered 4 x 3 grid, centres (20 + 28 gx + j, 24 + 36 gy + j'), j, j' in -4..4, activity a <- 0.8 a + event clipped at
    1 with events Bernoulli(0.06), integer noise -8..8 -> (video (F, H, W) uint8, centres (12, 2) int (col, row) pixel
    indices, activity (12, F))."""
    H, W, F, K = PLANTED["H"], PLANTED["W"], PLANTED["F"], PLANTED["K"]
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 121, (H, W)).astype(np.float64)
    cs = []
    for gy in range(3):
        for gx in range(4):
            cs.append((20 + gx * 28 + rng.integers(-4, 5), 24 + gy * 36 + rng.integers(-4, 5)))
    cs = np.array(cs[:K])
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = [np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * PLANTED["sigma"] ** 2)) for cx, cy in cs]
    act = np.zeros((K, F))
    for i in range(K):
        s = rng.random(F) < 0.06
        a = 0.0
        for k in range(F):
            a = a * 0.8 + (1.0 if s[k] else 0.0)
            act[i, k] = min(a, 1.0)
    v = np.empty((F, H, W), np.uint8)
    for k in range(F):
        f = base + sum(PLANTED["amp"] * act[i, k] * blobs[i] for i in range(K)) + \
            rng.integers(-PLANTED["noise"], PLANTED["noise"] + 1, (H, W))
        v[k] = np.clip(np.rint(f), 0, 255)
    return v, cs, act


PLANTED_BOX = (6.0, 6.0, 122.0, 122.0, 14.0)        # mesh.box_mesh arguments: a margin of 6 px, the cells are >= 16 px in
PLANTED_SHIFT = (3, -2)                              # whole pixels (d_col, d_row) of the second half of the frames


def planted_scene(seed, uv):
    """The planted video as the tracker sees it: the first half of the frames with the mesh at rest (X = uv, the warp is
    the identity on the map), the second half with mesh and frame moved by PLANTED_SHIFT -> (frames (F, H, W) uint8,
    states (F, 4N), centres, activity).  The registered video is the planted one on the map either way."""
    v, cs, act = planted_video(seed)
    F = v.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = PLANTED_SHIFT
    frames = v.copy()
    frames[F // 2:] = np.roll(v[F // 2:], (dr, dc), axis=(1, 2))     # (what wraps round lands in the margin: never read)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    states = np.array([rest if k < F // 2 else moved for k in range(F)])
    return frames, states, cs, act


def disc_trace(video, point, radius):
    """mean of every frame over the pixels whose centre lies within `radius` of `point` (x, y)"""
    H, W = video.shape[1:]
    yy, xx = np.mgrid[0:H, 0:W]
    m = (xx + 0.5 - point[0]) ** 2 + (yy + 0.5 - point[1]) ** 2 <= radius * radius
    return video[:, m].astype(np.float64).mean(1)
