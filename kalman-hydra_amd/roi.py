"""Cell footprints, ROIs and neuropil-corrected dF/F traces from the registered video kept on the device.

The device gives exact integer sums over the recorded frames (hm_body_rec_* in include/hydra_mi.h, csrc/roi_kernels.h);
everything here is host arithmetic on those sums, of the size seeds x window pixels:

  seed trace   U_k = n_G T_k - n_T G_k: the sum over the seed's disc minus the sum over a ring round it, scaled to whole
               numbers -- what the seed's pixels share with a frame-wide background (neuropil) cancels.
  footprint    rho_s(p): the correlation over time of every pixel of the (2R + 1)^2 window with U.
  ROI          the pixels with rho >= thr that are 4-connected to the seed pixel; a pixel claimed by several seeds goes
               to the nearer centre, then the lower index.  A seed whose own pixel is below thr keeps its disc.
  traces       F_roi (mean over the ROI), F_np (mean over the ring pixels that belong to no ROI),
               F_c = F_roi - alpha F_np, dF/F = (F_c - F0) / F0_raw with running-percentile baselines.

    body = BodyReadout(kf, keep=True, stats=True)
    ... track: body.frame(...) per frame, or FlowEKFPipeline.run(body=body) ...
    points, _ = body.find_points(12)
    res = roi.extract(body, points)

tests/roi_ref.py restates every step in NumPy and Python integers; the two agree bit for bit.
"""
import numpy as np

from .body import BodyReadout

#: halfway between the lowest footprint value within 2 px of a planted centre (0.542) and the highest on ring pixels
#: (0.401) of the planted video with neuropil (tests/roi_ref.py, six seeds; tests/test_roi_cpu.py measures both)
DEFAULT_THR = 0.47


def seeds_of(points):
    """Points (P, 2) in body coordinates -> the pixels (column, row) that hold them, int32 (find_points gives pixel
    centres: c + 0.5 -> c)."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    if not np.isfinite(p).all():
        raise ValueError("roi: a point is not finite")
    return np.floor(p).astype(np.int32)


def _window(H, W, seed, R):
    d = np.arange(-R, R + 1)
    rr, cc = np.meshgrid(int(seed[1]) + d, int(seed[0]) + d, indexing="ij")
    on = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
    return np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1), on


def _ints(a):
    """an integer array as an object array of Python integers (their products pass 2^64)"""
    a = np.asarray(a)
    return np.array(a.tolist(), dtype=object).reshape(a.shape)


def footprints(ss, F, inmap, seeds, R):
    """rho (P, 2R+1, 2R+1) float64 from the sums of body_rec_seed_sums:
    (F c - w1 u1) / sqrt((F w2 - w1^2)(F u2 - u1^2)).  The three whole numbers are formed in Python integers and rounded
    once each to binary64; then one product, one square root, one division.  0 where a variance is 0, NaN off the frame
    and outside the map."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    P, S = len(seeds), 2 * R + 1
    F = int(F)
    w1, w2, c = _ints(ss["w1"]), _ints(ss["w2"]), _ints(ss["c"])
    u1, u2 = _ints(ss["u1"]).reshape(P, 1, 1), _ints(ss["u2"]).reshape(P, 1, 1)
    num = (F * c - w1 * u1).astype(np.float64)
    va = (F * w2 - w1 * w1).astype(np.float64)
    vb = np.broadcast_to((F * u2 - u1 * u1).astype(np.float64), va.shape)
    flat = (va == 0.0) | (vb == 0.0)                 # (whole numbers: the rounded value is 0 only when the integer is)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(flat, 0.0, num / np.sqrt(va * vb))
    for s in range(P):
        rr, cc, on = _window(H, W, seeds[s], R)
        rho[s][~(on & m[rr, cc])] = np.nan
    return rho.reshape(P, S, S)


def grow(rho, thr):
    """One window (S, S) -> mask of the pixels with rho >= thr that are 4-connected to the centre through such pixels
    (none when the centre itself is below thr or NaN)."""
    S = rho.shape[0]
    R = S // 2
    with np.errstate(invalid="ignore"):
        ok = rho >= thr
    got = np.zeros((S, S), bool)
    if not ok[R, R]:
        return got
    got[R, R] = True
    while True:                                       # dilate by the 4-neighbourhood within `ok` until nothing is added
        nxt = got.copy()
        nxt[1:, :] |= got[:-1, :]
        nxt[:-1, :] |= got[1:, :]
        nxt[:, 1:] |= got[:, :-1]
        nxt[:, :-1] |= got[:, 1:]
        nxt &= ok
        if (nxt == got).all():
            return got
        got = nxt


def assign(rho, thr, inmap, seeds, R, r_disc):
    """-> (labels (H, W) int32, -1: none; counts (P,) int64; fallback (P,) bool).  Every seed claims the pixels grown from
    it, or the map pixels of its disc when its own pixel is below thr (fallback); a pixel claimed by several seeds goes to
    the one whose centre is nearer (integer distance^2), then to the lower index.  Nothing grows again after that."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    P = len(seeds)
    labels = np.full((H, W), -1, np.int32)
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    fallback = np.zeros(P, bool)
    Rd = int(np.floor(float(r_disc)))
    r2 = float(r_disc) * float(r_disc)
    for s in range(P):
        g = grow(rho[s], thr)
        Rw = R
        if not g.any():
            fallback[s] = True
            Rw = Rd
            d = np.arange(-Rd, Rd + 1)
            g = (d[None, :] ** 2 + d[:, None] ** 2).astype(np.float64) <= r2
        rr, cc, on = _window(H, W, seeds[s], Rw)
        d = np.arange(-Rw, Rw + 1, dtype=np.int64)
        d2 = d[None, :] ** 2 + d[:, None] ** 2
        take = g & on & m[rr, cc] & (d2 < best[rr, cc])       # (strictly nearer: a tie keeps the lower index)
        best[rr[take], cc[take]] = d2[take]
        labels[rr[take], cc[take]] = s
    counts = np.bincount(labels[labels >= 0], minlength=P).astype(np.int64)
    return labels, counts, fallback


def ring_weights(labels, inmap, seeds, r_in, r_out):
    """-> (weights (P, 2Rg+1, 2Rg+1) uint16 of 0 / 1, counts (P,) int64, Rg = floor(r_out)): every seed's ring pixels
    (map pixels with r_in^2 <= d2 <= r_out^2) that belong to no ROI."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    Rg = int(np.floor(float(r_out)))
    d = np.arange(-Rg, Rg + 1)
    d2 = (d[None, :] ** 2 + d[:, None] ** 2).astype(np.float64)
    ring = (d2 >= float(r_in) * float(r_in)) & (d2 <= float(r_out) * float(r_out))
    free = m & (np.asarray(labels) < 0)
    w = np.zeros((len(seeds), 2 * Rg + 1, 2 * Rg + 1), np.uint16)
    for s in range(len(seeds)):
        rr, cc, on = _window(H, W, seeds[s], Rg)
        w[s] = ring & on & free[rr, cc]
    return w, w.reshape(len(seeds), -1).sum(1).astype(np.int64), Rg


def baseline(x, q, half):
    """The running q-th percentile of x over the frames k - half .. k + half, the window clipped at the ends
    (np.percentile's linear rule)."""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    return np.array([np.percentile(x[max(0, k - half):min(F, k + half + 1)], q) for k in range(F)], np.float64)


def _means(sums, counts, empty):
    F, P = sums.shape
    out = np.empty((F, P))
    for s in range(P):
        out[:, s] = sums[:, s].astype(np.float64) / np.float64(counts[s]) if counts[s] > 0 else empty
    return out


def extract(body, points, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=None, alpha=0.7, q=10.0, half=100):
    """Footprints, ROIs and traces of the cells at `points` ((P, 2) in body coordinates, inside the mesh) from the frames a
    BodyReadout(keep=True) has recorded.  -> dict:
      footprints (P, 2R+1, 2R+1) float64   correlation of every window pixel with the ring-corrected seed trace
      roi_labels (H, W) int32, roi_counts (P,), seed_fallback (P,) bool (the seed kept its disc of r_disc)
      ring_counts (P,)                     ring pixels left after every ROI pixel is taken out (0: F_np is 0)
      F_roi, F_np (F, P) float64           mean over the ROI, mean over the ring
      dff (F, P) float64                   (F_c - F0) / F0_raw, F_c = F_roi - alpha F_np
    F0 is the running q-th percentile of F_c over 2 half + 1 frames; F0_raw is the same percentile of F_roi, not of F_c: the
    corrected baseline is near zero when alpha takes the whole background away, and dividing by it would blow the ratio
    up.  thr None: DEFAULT_THR."""
    r = BodyReadout.record(body, "roi.extract")
    F = r.body_rec_count()
    if F < 1:
        raise RuntimeError("roi.extract: no frame recorded")
    thr = DEFAULT_THR if thr is None else float(thr)
    m = body.tri_of_pixel >= 0
    seeds = seeds_of(points)
    P = seeds.shape[0]
    ss = r.body_rec_seed_sums(seeds, r_disc, r_in, r_out, R)
    rho = footprints(ss, F, m, seeds, R)
    labels, counts, fallback = assign(rho, thr, m, seeds, R, r_disc)
    lsum = r.body_rec_label_sums(labels, P)
    w, ring_counts, Rg = ring_weights(labels, m, seeds, r_in, r_out)
    gsum = r.body_rec_weighted_sums(seeds, w, Rg)
    F_roi = _means(lsum, counts, np.nan)
    F_np = _means(gsum, ring_counts, 0.0)
    F_c = F_roi - np.float64(alpha) * F_np
    dff = np.empty((F, P))
    for s in range(P):
        with np.errstate(invalid="ignore", divide="ignore"):
            dff[:, s] = (F_c[:, s] - baseline(F_c[:, s], q, half)) / baseline(F_roi[:, s], q, half)
    return dict(footprints=rho, roi_labels=labels, roi_counts=counts, ring_counts=ring_counts, F_roi=F_roi, F_np=F_np,
                dff=dff, seed_fallback=fallback, seed_sums=ss, seeds=seeds, ring_radii=np.array([r_in, r_out], np.float64))
