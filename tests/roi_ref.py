"""NumPy / Python-integer restatement of the reductions over the recorded registered video (include/hydra_mi.h:
hm_body_rec_*) and of the footprints, ROIs and traces built on them (hydra_mi.roi), and the planted video with neuropil
the recovery tests run on.

`regs` is the registered video (F, H, W) uint8, `inmap` the body map as a mask (tri_of >= 0), `seeds` (P, 2) integer
pixel indices (col, row) of map pixels.  Sums are exact integers (int64 / uint64 where they fit, Python integers where
they do not); every floating-point step is written out once.
"""
import numpy as np

# ---- the reductions ---------------------------------------------------------------------------------------------------


def label_sums(regs, inmap, labels, L):
    """-> (F, L) uint64: the sum of every frame over the map pixels of each label"""
    v = np.asarray(regs).astype(np.int64)
    lab = np.where(np.asarray(inmap, bool), np.asarray(labels), -1)
    out = np.zeros((v.shape[0], L), np.uint64)
    for i in range(L):
        out[:, i] = v[:, lab == i].sum(1)
    return out


def _d2(H, W, seed):
    """integer distance^2 of every pixel centre from the centre of pixel `seed` (col, row)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx - int(seed[0])) ** 2 + (yy - int(seed[1])) ** 2


def disc_and_ring(inmap, seed, r_disc, r_in, r_out):
    """-> (disc, ring) masks: map pixels with d2 <= r_disc^2, and with r_in^2 <= d2 <= r_out^2 (float64 comparisons of
    the whole number d2 with r * r, the rule of body.disc_labels)"""
    m = np.asarray(inmap, bool)
    d2 = _d2(m.shape[0], m.shape[1], seed).astype(np.float64)
    rd, ri, ro = float(r_disc), float(r_in), float(r_out)
    return m & (d2 <= rd * rd), m & (d2 >= ri * ri) & (d2 <= ro * ro)


def window(H, W, seed, R):
    """The (2R + 1)^2 window round `seed`: (rows, cols, on) -- pixel indices (clipped where off the frame) and whether the
    window pixel is on the frame; window index (dy + R) * (2R + 1) + dx + R."""
    d = np.arange(-R, R + 1)
    rr, cc = np.meshgrid(int(seed[1]) + d, int(seed[0]) + d, indexing="ij")
    on = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
    return np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1), on


def overflow_bound(F, n_T, n_G):
    """F (255 n_T n_G)^2 as a Python integer: the sums of U^2 are exact in int64 while it stays below 2^63"""
    return int(F) * (255 * int(n_T) * int(n_G)) ** 2


def seed_sums(regs, inmap, seeds, r_disc, r_in, r_out, R):
    """-> dict: n_T, n_G (P,) uint32; T, G (F, P) uint64; U (F, P) int64 = n_G T - n_T G; w1, w2 (P, 2R+1, 2R+1) uint64,
    c (P, 2R+1, 2R+1) int64 (0 off the frame and outside the map); u1, u2 (P,) int64"""
    v = np.asarray(regs).astype(np.int64)
    m = np.asarray(inmap, bool)
    F, H, W = v.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    P, S = seeds.shape[0], 2 * R + 1
    out = dict(n_T=np.zeros(P, np.uint32), n_G=np.zeros(P, np.uint32), T=np.zeros((F, P), np.uint64),
               G=np.zeros((F, P), np.uint64), U=np.zeros((F, P), np.int64), w1=np.zeros((P, S, S), np.uint64),
               w2=np.zeros((P, S, S), np.uint64), c=np.zeros((P, S, S), np.int64), u1=np.zeros(P, np.int64),
               u2=np.zeros(P, np.int64))
    for s, seed in enumerate(seeds):
        disc, ring = disc_and_ring(m, seed, r_disc, r_in, r_out)
        nT, nG = int(disc.sum()), int(ring.sum())
        if overflow_bound(F, nT, nG) >= 2 ** 63:
            raise OverflowError("seed %d: F (255 n_T n_G)^2 = %d (255 * %d * %d)^2 reaches 2^63" % (s, F, nT, nG))
        T, G = v[:, disc].sum(1), v[:, ring].sum(1)
        U = nG * T - nT * G
        rr, cc, on = window(H, W, seed, R)
        ok = on & m[rr, cc]
        x = np.where(ok[None], v[:, rr, cc], 0)                    # (F, S, S)
        out["n_T"][s], out["n_G"][s] = nT, nG
        out["T"][:, s], out["G"][:, s], out["U"][:, s] = T, G, U
        out["w1"][s], out["w2"][s] = x.sum(0), (x * x).sum(0)
        out["c"][s] = (x * U[:, None, None]).sum(0)
        out["u1"][s], out["u2"][s] = U.sum(), (U * U).sum()
    return out


def weighted_sums(regs, inmap, seeds, weights, R):
    """weights (P, 2R+1, 2R+1) uint16 round each seed -> (F, P) uint64: sum of weight x value over the window pixels on
    the frame and in the map"""
    v = np.asarray(regs).astype(np.int64)
    m = np.asarray(inmap, bool)
    F, H, W = v.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    out = np.zeros((F, seeds.shape[0]), np.uint64)
    for s, seed in enumerate(seeds):
        rr, cc, on = window(H, W, seed, R)
        a = np.where(on & m[rr, cc], np.asarray(weights[s]).astype(np.int64), 0)
        out[:, s] = (v[:, rr, cc] * a[None]).sum((1, 2))
    return out


# ---- footprints, ROIs, traces (host arithmetic on the exact sums) -----------------------------------------------------
def footprints(ss, F, inmap, seeds, R):
    """rho (P, 2R+1, 2R+1) float64: (F c - w1 u1) / sqrt((F w2 - w1^2)(F u2 - u1^2)), the three whole numbers formed as
    Python integers and rounded once each to binary64, then one product, one square root, one division; 0 where a
    variance is 0, NaN off the frame and outside the map."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    P, S = seeds.shape[0], 2 * R + 1
    rho = np.full((P, S, S), np.nan)
    F = int(F)
    for s, seed in enumerate(seeds):
        rr, cc, on = window(H, W, seed, R)
        u1, u2 = int(ss["u1"][s]), int(ss["u2"][s])
        vb = F * u2 - u1 * u1
        for i in range(S):
            for j in range(S):
                if not (on[i, j] and m[rr[i, j], cc[i, j]]):
                    continue
                w1, w2, c = int(ss["w1"][s, i, j]), int(ss["w2"][s, i, j]), int(ss["c"][s, i, j])
                va = F * w2 - w1 * w1
                if va == 0 or vb == 0:
                    rho[s, i, j] = 0.0
                    continue
                num = F * c - w1 * u1
                rho[s, i, j] = np.float64(float(num)) / np.sqrt(np.float64(float(va)) * np.float64(float(vb)))
    return rho


def grow(rho, thr):
    """One window (S, S) -> the mask of the pixels with rho >= thr that are 4-connected to the centre through such
    pixels (all False when the centre itself is below thr or NaN)"""
    S = rho.shape[0]
    R = S // 2
    with np.errstate(invalid="ignore"):
        ok = rho >= thr
    got = np.zeros((S, S), bool)
    if not ok[R, R]:
        return got
    got[R, R] = True
    todo = [(R, R)]
    while todo:
        i, j = todo.pop()
        for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            if 0 <= a < S and 0 <= b < S and ok[a, b] and not got[a, b]:
                got[a, b] = True
                todo.append((a, b))
    return got


def rois(rho, thr, inmap, seeds, R, r_disc):
    """-> (labels (H, W) int32, -1: none; counts (P,) int64; fallback (P,) bool).  Every seed claims its grown pixels, or
    its disc when its own pixel is below thr (fallback); a pixel claimed by several seeds goes to the one whose centre
    is nearer (integer distance^2), then to the lower index."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    P = seeds.shape[0]
    labels = np.full((H, W), -1, np.int32)
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    fallback = np.zeros(P, bool)
    for s, seed in enumerate(seeds):
        claim = np.zeros((H, W), bool)
        g = grow(rho[s], thr)
        if g.any():
            rr, cc, on = window(H, W, seed, R)
            claim[rr[g & on], cc[g & on]] = True
            claim &= m
        else:
            fallback[s] = True
            claim = disc_and_ring(m, seed, r_disc, 0.0, 0.0)[0]
        d2 = _d2(H, W, seed)
        take = claim & (d2 < best)                                  # (strictly nearer: a tie keeps the lower index)
        best[take] = d2[take]
        labels[take] = s
    counts = np.array([(labels == s).sum() for s in range(P)], np.int64)
    return labels, counts, fallback


def ring_weights(labels, inmap, seeds, r_in, r_out):
    """-> (weights (P, 2Rg+1, 2Rg+1) uint16 of 0 / 1, Rg = floor(r_out); counts (P,)): the ring pixels of every seed
    that belong to no ROI"""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    Rg = int(np.floor(float(r_out)))
    w = np.zeros((seeds.shape[0], 2 * Rg + 1, 2 * Rg + 1), np.uint16)
    free = m & (np.asarray(labels) < 0)
    for s, seed in enumerate(seeds):
        ring = disc_and_ring(m, seed, 0.0, r_in, r_out)[1] & free
        rr, cc, on = window(H, W, seed, Rg)
        w[s] = on & ring[rr, cc]
    return w, w.reshape(w.shape[0], -1).sum(1).astype(np.int64), Rg


def baseline(x, q, half):
    """The running q-th percentile of x over the frames k - half .. k + half, clipped at the ends (np.percentile's
    linear rule)"""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    return np.array([np.percentile(x[max(0, k - half):min(F, k + half + 1)], q) for k in range(F)], np.float64)


def _mean(sums, count):
    s = np.asarray(sums).astype(np.float64)
    return s / np.float64(count) if count > 0 else np.full(s.shape, np.nan)


def extract(regs, inmap, seeds, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=0.3, alpha=0.7, q=10.0, half=100):
    """The whole of hydra_mi.roi.extract on a registered video -> the same dict"""
    regs = np.asarray(regs)
    m = np.asarray(inmap, bool)
    F = regs.shape[0]
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    P = seeds.shape[0]
    ss = seed_sums(regs, m, seeds, r_disc, r_in, r_out, R)
    rho = footprints(ss, F, m, seeds, R)
    labels, counts, fallback = rois(rho, thr, m, seeds, R, r_disc)
    lsum = label_sums(regs, m, labels, P)
    w, ring_counts, Rg = ring_weights(labels, m, seeds, r_in, r_out)
    gsum = weighted_sums(regs, m, seeds, w, Rg)
    F_roi = np.stack([_mean(lsum[:, s], counts[s]) for s in range(P)], 1).reshape(F, P)
    F_np = np.stack([_mean(gsum[:, s], ring_counts[s]) if ring_counts[s] > 0 else np.zeros(F) for s in range(P)],
                    1).reshape(F, P)
    F_c = F_roi - np.float64(alpha) * F_np
    dff = np.empty((F, P))
    for s in range(P):
        with np.errstate(invalid="ignore", divide="ignore"):
            dff[:, s] = (F_c[:, s] - baseline(F_c[:, s], q, half)) / baseline(F_roi[:, s], q, half)
    return dict(footprints=rho, roi_labels=labels, roi_counts=counts, ring_counts=ring_counts, F_roi=F_roi, F_np=F_np,
                dff=dff, seed_fallback=fallback)


# ---- the planted video with neuropil ----------------------------------------------------------------------------------
PLANTED = dict(H=128, W=128, F=300, K=12, amp=50.0, noise=8, sigma_lo=1.5, sigma_hi=2.5, neuropil=30.0, ar=0.95)
PLANTED_BOX = (6.0, 6.0, 122.0, 122.0, 14.0)        # mesh.box_mesh arguments (bodystats_ref.PLANTED_BOX)
PLANTED_SHIFT = (3, -2)                              # whole pixels (d_col, d_row) of the second half of the frames


def planted_video(seed):
    """128 x 128, 300 frames: the grid and the activity model of bodystats_ref.planted_video (12 cells on a jittered 4 x 3
    grid, a <- 0.8 a + event clipped at 1, events Bernoulli(0.06)) with elliptical Gaussian cells (sigmas 1.5..2.5 px along
    axes at a random angle, amplitude 50 x activity), a static texture 40..120, integer noise -8..8, and neuropil: one
    AR(1) signal (coefficient 0.95, Gaussian steps) scaled to 0..30 and added to every pixel
    -> (video (F, H, W) uint8, centres (12, 2) int (col, row), activity (12, F), neuropil (F,))."""
    H, W, F, K = PLANTED["H"], PLANTED["W"], PLANTED["F"], PLANTED["K"]
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 121, (H, W)).astype(np.float64)
    cs = []
    for gy in range(3):
        for gx in range(4):
            cs.append((20 + gx * 28 + rng.integers(-4, 5), 24 + gy * 36 + rng.integers(-4, 5)))
    cs = np.array(cs[:K])
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = []
    for cx, cy in cs:
        sa, sb = rng.uniform(PLANTED["sigma_lo"], PLANTED["sigma_hi"], 2)
        th = rng.uniform(0.0, np.pi)
        a = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        b = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        blobs.append(np.exp(-(a * a / (2 * sa * sa) + b * b / (2 * sb * sb))))
    act = np.zeros((K, F))
    for i in range(K):
        s = rng.random(F) < 0.06
        a = 0.0
        for k in range(F):
            a = a * 0.8 + (1.0 if s[k] else 0.0)
            act[i, k] = min(a, 1.0)
    npil = np.zeros(F)
    x = 0.0
    for k in range(F):
        x = PLANTED["ar"] * x + rng.normal()
        npil[k] = x
    npil = PLANTED["neuropil"] * (npil - npil.min()) / (npil.max() - npil.min())
    v = np.empty((F, H, W), np.uint8)
    for k in range(F):
        f = base + npil[k] + sum(PLANTED["amp"] * act[i, k] * blobs[i] for i in range(K)) + \
            rng.integers(-PLANTED["noise"], PLANTED["noise"] + 1, (H, W))
        v[k] = np.clip(np.rint(f), 0, 255)
    return v, cs, act, npil


def planted_scene(seed, uv):
    """The planted video as the tracker sees it (bodystats_ref.planted_scene): the first half of the frames with the mesh
    at rest, the second half with mesh and frame moved by PLANTED_SHIFT -> (frames, states (F, 4N), centres, activity)"""
    v, cs, act, _ = planted_video(seed)
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


def planted_map():
    """The body map of mesh.box_mesh(*PLANTED_BOX) as a mask, restated: the pixels whose centres lie in the box (the CPU
    tests have no device to ask)"""
    H, W = PLANTED["H"], PLANTED["W"]
    x0, y0, x1, y1, _ = PLANTED_BOX
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx + 0.5 >= x0) & (xx + 0.5 < x1) & (yy + 0.5 >= y0) & (yy + 0.5 < y1)
