"""NumPy restatement of the running baseline per pixel of the kept registered video (include/hydra_mi.h:
hm_body_rec_planes / hm_body_rec_stats_add; hydra_mi.detrend), in exact integers, and the drifting planted video the
seed recovery is measured on.  `inmap` is the body map as a mask (tri_of >= 0)."""
import numpy as np

import roi_ref

KINDS = {"recorded": 0, "baseline": 1, "excess": 2, "dff": 3}


def rank(q, n):
    """0-based rank of the baseline among n window values, in integers"""
    return (int(q) * (int(n) - 1)) // 100


def planes(regs, inmap, what, half, q, floor=1, gain=1, k0=0, n=None):
    """Registered frames (F, H, W) uint8 -> the planes of kind `what` (0 / "recorded", 1 / "baseline", 2 / "excess",
    3 / "dff") of the frames k0 .. k0 + n - 1 (default: all from k0), (n, H, W) uint8; 0 outside the map.  The windows
    reach over all F frames.  np.partition per frame."""
    what = KINDS.get(what, what)
    v = np.where(np.asarray(inmap, bool)[None], np.asarray(regs, np.uint8), 0).astype(np.uint8)
    F = v.shape[0]
    n = F - k0 if n is None else n
    if what == 0:
        return v[k0:k0 + n]
    out = np.empty_like(v)
    for k in range(k0, k0 + n):
        a, b = max(0, k - int(half)), min(F - 1, k + int(half))
        r = rank(q, b - a + 1)
        B = np.partition(v[a:b + 1], r, axis=0)[r].astype(np.int64)
        E = np.maximum(v[k].astype(np.int64) - B, 0)
        if what == 1:
            out[k] = B
        elif what == 2:
            out[k] = E
        else:
            out[k] = np.minimum(255, (int(gain) * E) // np.maximum(B, int(floor)))
    return out[k0:k0 + n]


DRIFT = dict(bleach=600.0, patches=6, sigma=14.0, lo=20.0, hi=108.0, amp=40.0, T_lo=150.0, T_hi=400.0)


def drifting_video(seed):
    """roi_ref.planted_video(seed) with a drift added: a bleaching factor exp(-k / 600) and six Gaussian patches (sigma
    14 px, centres uniform in 20..108, amplitude 40), each scaled by 0.5 + 0.5 sin(2 pi k / T + phi) with T uniform in
    150..400 frames; generator np.random.default_rng(100 + seed); rounded to uint8, 0 off roi_ref.planted_map()
    -> (video (F, H, W) uint8, centres (12, 2) int (col, row), clean video (F, H, W) uint8)."""
    v, cs = roi_ref.planted_video(seed)[:2]
    F, H, W = v.shape
    rng = np.random.default_rng(100 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    k = np.arange(F, dtype=np.float64)
    add = np.zeros((F, H, W))
    for _ in range(DRIFT["patches"]):
        cx, cy = rng.uniform(DRIFT["lo"], DRIFT["hi"], 2)
        T = rng.uniform(DRIFT["T_lo"], DRIFT["T_hi"])
        phi = rng.uniform(0.0, 2.0 * np.pi)
        blob = DRIFT["amp"] * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * DRIFT["sigma"] ** 2))
        add += (0.5 + 0.5 * np.sin(2.0 * np.pi * k / T + phi))[:, None, None] * blob[None]
    f = v.astype(np.float64) * np.exp(-k / DRIFT["bleach"])[:, None, None] + add
    m = roi_ref.planted_map()
    out = np.where(m[None], np.clip(np.rint(f), 0, 255), 0).astype(np.uint8)
    return out, cs, np.where(m[None], v, 0).astype(np.uint8)


def drifting_scene(seed, uv):
    """The drifting video as the tracker sees it (roi_ref.planted_scene: the second half of the frames with mesh and
    frame moved by roi_ref.PLANTED_SHIFT) -> (frames (F, H, W) uint8, states (F, 4N), centres, the drifting video).  The
    registered video is the drifting one on the map either way."""
    v, cs, _ = drifting_video(seed)
    F = v.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = roi_ref.PLANTED_SHIFT
    frames = v.copy()
    frames[F // 2:] = np.roll(v[F // 2:], (dr, dc), axis=(1, 2))     # (what wraps round lands in the margin: never read)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    return frames, np.array([rest if k < F // 2 else moved for k in range(F)]), cs, v


def seeds_found(peaks_idx, W, centres, tol=2):
    """how many of the centres (col, row) have one of the peaks (raster indices) within `tol` px"""
    rr, cc = np.divmod(np.asarray(peaks_idx, np.int64), W)
    return int(sum(bool(((cc - cx) ** 2 + (rr - cy) ** 2 <= tol * tol).any()) for cx, cy in centres))
