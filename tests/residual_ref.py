"""NumPy restatement of the residual video of the demixed model (include/hydra_mi.h: hm_body_rec_residual_planes /
hm_body_rec_residual_stats_add; hydra_mi.residual), in exact integers: the rule one frame and one layer at a time in
int64, and model, blank_discs and find_more over the restatements of roi_ref, demix_ref and bodystats_ref."""
import functools
import math

import numpy as np

import bodystats_ref as bs
import demix_ref
import roi_ref

TBITS = 24


def planes(regs, inmap, labels, weights, traces, blank=None, offset=64):
    """regs (F, H, W) uint8 the record, inmap (H, W), labels (n_layers, H, W) int32 (-1: none), weights the same shape
    uint16 or None (65535 everywhere), traces (F, L) int32, blank (H, W) or None -> (R (F, H, W) uint8, clipped)."""
    regs = np.asarray(regs)
    m = np.asarray(inmap, bool)
    lab = np.asarray(labels, np.int64)
    lab = lab[None] if lab.ndim == 2 else lab
    w = np.full(lab.shape, 65535, np.int64) if weights is None else np.asarray(weights).astype(np.int64).reshape(lab.shape)
    tr = np.asarray(traces).astype(np.int64)
    live = m if blank is None else m & (np.asarray(blank) == 0)
    out = np.zeros(regs.shape, np.uint8)
    clipped = 0
    for k in range(regs.shape[0]):
        acc = np.zeros(m.shape, np.int64)
        for j in range(lab.shape[0]):
            has = lab[j] >= 0
            acc += np.where(has, w[j] * tr[k][np.where(has, lab[j], 0)], 0)
        mod = (acc + (1 << 23)) >> 24                                  # (NumPy's >> on int64 is arithmetic: floor)
        r = offset + regs[k].astype(np.int64) - mod
        clipped += int((live & ((r < 0) | (r > 255))).sum())
        out[k] = np.where(live, np.clip(r, 0, 255), 0)
    return out, clipped


def layers(shapes_q, seeds, R, shape, n_layers):
    """cellview.layers_from_shapes pixel by pixel: per body pixel the cells with a window value > 0 there in ascending
    index, the first n_layers kept -> (labels, weights, dropped)"""
    H, W = shape
    lab = np.full((n_layers, H, W), -1, np.int32)
    wt = np.zeros((n_layers, H, W), np.uint16)
    depth = np.zeros((H, W), np.int64)
    dropped = 0
    for s, (c, r) in enumerate(np.asarray(seeds).reshape(-1, 2).tolist()):
        for i in range(2 * R + 1):
            for j in range(2 * R + 1):
                y, x, a = r - R + i, c - R + j, int(shapes_q[s][i][j])
                if a <= 0 or not (0 <= y < H and 0 <= x < W):
                    continue
                if depth[y, x] < n_layers:
                    lab[depth[y, x], y, x], wt[depth[y, x], y, x] = s, a
                else:
                    dropped += 1
                depth[y, x] += 1
    return lab, wt, dropped


def model(e, seeds, shape, n_layers=4):
    """hydra_mi.residual.model: the dict of demix_ref.demix and its seeds (P, 2) (column, row) -> (labels, weights, traces
    (F, P) int32, dropped)"""
    a_q = np.asarray(e["shapes_q"])
    C = np.asarray(e["C"], np.float64)
    F, P = C.shape
    lab, wt, dropped = layers(a_q, seeds, a_q.shape[1] // 2, shape, n_layers)
    tr = np.zeros((F, P), np.int32)
    for s in range(P):
        vals = [int(v) for v in a_q[s].ravel().tolist()]
        sa, g = sum(vals), sum(v * v for v in vals)
        if g == 0:
            continue
        scale = float(sa) / float(g)
        c = [float(C[k, s]) * scale for k in range(F)]
        mean = math.fsum(c) / F
        for k in range(F):
            t = float(np.rint((c[k] - mean) * 16777216.0))
            assert abs(t) < 2.0 ** 31
            tr[k, s] = int(t)
    return lab, wt, tr, dropped


def blank_discs(seeds, radius, shape):
    H, W = shape
    out = np.zeros((H, W), np.uint8)
    for c, r in np.asarray(seeds).reshape(-1, 2).tolist():
        for y in range(max(0, r - radius), min(H, r + radius + 1)):
            for x in range(max(0, c - radius), min(W, c + radius + 1)):
                if (x - c) ** 2 + (y - r) ** 2 <= radius * radius:
                    out[y, x] = 1
    return out


def first_pass(regs, inmap, radius=6, min_score=0.8):
    """the corr peaks of the record itself -> (seeds (P, 2) (column, row), scores of all peaks descending)"""
    m = np.asarray(inmap, bool)
    F, H, W = np.asarray(regs).shape
    img = bs.images(*bs.accumulate(regs, m), F, m)
    idx, sc = bs.peaks_fast(img[2], m, radius)
    keep = sc >= min_score
    rr, cc = np.divmod(idx[keep].astype(np.int64), W)
    return np.stack((cc, rr), 1), sc


def rois_ok(regs, inmap, seeds, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=0.47):
    ss = roi_ref.seed_sums(regs, inmap, seeds, r_disc, r_in, r_out, R)
    rho = roi_ref.footprints(ss, np.asarray(regs).shape[0], inmap, seeds, R)
    return bool((roi_ref.rois(rho, thr, inmap, seeds, R, r_disc)[1] >= 1).all())


def find_more(regs, inmap, seeds, min_score, rounds=3, radius=6, blank=2, offset=64, all_scores=False, **demix_args):
    """hydra_mi.residual.find_more on a registered video, seeds (P, 2) (column, row) whole pixels -> dict: seeds (all of
    them), round, scores (per round; with all_scores also "top": the best scores of every round without a threshold),
    accepted, refused [(round, (column, row), score, reason)], clipped, dropped, ended, e."""
    regs = np.asarray(regs)
    m = np.asarray(inmap, bool)
    F, H, W = regs.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    roi_args = {k: demix_args[k] for k in ("r_disc", "r_in", "r_out", "R", "thr") if k in demix_args}
    out = dict(round=[0] * len(seeds), scores=[], top=[], accepted=[], refused=[], clipped=[], dropped=0, ended="rounds")
    e = demix_ref.demix(regs, m, seeds, **demix_args)
    for rnd in range(1, rounds + 1):
        lab, wt, tr, out["dropped"] = model(e, seeds, (H, W))
        bl = None if blank is None else blank_discs(seeds, blank, (H, W))
        res, clipped = planes(regs, m, lab, wt, tr, bl, offset)
        out["clipped"].append(clipped)
        img = bs.images(*bs.accumulate(res, m), F, m)
        idx, sc = bs.peaks_fast(img[2], m, radius, min_score)
        out["scores"].append(sc)
        if all_scores:
            out["top"].append(bs.peaks_fast(img[2], m, radius)[1][:len(sc) + 3])
        taken = 0
        for i, v in zip(idx.tolist(), sc.tolist()):
            cand = np.array([i % W, i // W], np.int64)
            if (seeds == cand).all(1).any():
                out["refused"].append((rnd, cand, v, "seeded"))
                continue
            trial = np.vstack((seeds, cand))
            if not rois_ok(regs, m, trial, **roi_args):
                out["refused"].append((rnd, cand, v, "roi"))
                continue
            seeds = trial
            out["round"].append(rnd)
            taken += 1
        out["accepted"].append(taken)
        if taken == 0:
            out["ended"] = "none accepted"
            break
        e = demix_ref.demix(regs, m, seeds, **demix_args)
    out.update(seeds=seeds, round=np.array(out["round"], np.int32), e=e)
    return out


def matched(seeds, centres, tol=2.0):
    """every seed within tol px of a different planted centre, and every centre taken"""
    seeds, centres = np.asarray(seeds, np.float64), np.asarray(centres, np.float64)
    if len(seeds) != len(centres):
        return False
    d = np.sqrt(((seeds[:, None, :] - centres[None, :, :]) ** 2).sum(2))
    near = d.argmin(1)
    return bool((d[np.arange(len(seeds)), near] <= tol).all() and len(set(near.tolist())) == len(centres))


def found(seeds, centres, tol=2.0):
    """how many planted centres have a seed within tol px"""
    seeds, centres = np.asarray(seeds, np.float64), np.asarray(centres, np.float64)
    d = np.sqrt(((seeds[:, None, :] - centres[None, :, :]) ** 2).sum(2))
    return int((d.min(0) <= tol).sum())


@functools.lru_cache(maxsize=None)
def paired_more(seed, sep, min_score=0.8):
    """demix_ref.paired_video(seed, sep), its first pass and find_more from it (the product's defaults, alpha = 1 as
    demix_ref.paired_run), computed once for all the tests that look at it; nothing of it is to be changed
    -> (video, centres, activity, first seeds, first scores, dict of find_more)"""
    v, cs, act, _ = demix_ref.paired_video(seed, sep)
    m = roi_ref.planted_map()
    s0, sc0 = first_pass(v, m, 6, min_score)
    return v, cs, act, s0, sc0, find_more(v, m, s0, min_score, all_scores=True, alpha=1.0)
