"""Restatement of the trace maps over the recorded video (include/hydra_mi.h: hm_body_rec_trace_maps) and of hydra_mi.network
in loops, Python integers and a union-find, and the planted video with ensembles the recovery tests run on.

`regs` is the registered video (F, H, W) uint8, `inmap` the body map as a mask, `q` whole-number traces (F, L) as the
device takes them (frame-major), `x` traces (K, F) float64.  Every floating-point step is written out once.
"""
import numpy as np

import roi_ref

QMAX = 32767


# ---- the reduction ----------------------------------------------------------------------------------------------------
def trace_maps(regs, inmap, q):
    """-> (c (L, H, W) int64, w1, w2 (H, W) uint64): sum_k v_k(p) q[k, s], sum_k v_k(p), sum_k v_k(p)^2 over the map
    pixels, 0 elsewhere"""
    v = np.where(np.asarray(inmap, bool)[None], np.asarray(regs), 0).astype(np.int64)
    q = np.asarray(q).astype(np.int64)
    assert np.abs(q).max(initial=0) <= QMAX and v.shape[0] == q.shape[0]
    assert v.shape[0] ** 2 * 255 * QMAX < 2 ** 63
    c = np.zeros((q.shape[1],) + v.shape[1:], np.int64)
    for s in range(q.shape[1]):
        for k in range(v.shape[0]):
            c[s] += v[k] * q[k, s]
    return c, v.sum(0).astype(np.uint64), (v * v).sum(0).astype(np.uint64)


def quantise(x):
    """(K, F) float64 -> int32: rint((32767 x) / max|x|) per cell, 0 for an all-zero trace"""
    x = np.asarray(x, np.float64)
    if not np.isfinite(x).all():
        raise ValueError("a trace is not finite")
    q = np.zeros(x.shape, np.int32)
    for k in range(x.shape[0]):
        top = max((abs(float(v)) for v in x[k]), default=0.0)
        for f in range(x.shape[1]):
            if top > 0.0:
                q[k, f] = int(np.rint((np.float64(32767.0) * x[k, f]) / np.float64(top)))
    return q


def rho(c, w1, w2, q, inmap):
    """(K, H, W) float64 from the sums and the traces q (K, F) in Python integers: (F c - w1 u1) / sqrt((F w2 - w1^2)
    (F u2 - u1^2)), the three whole numbers rounded once each; 0 where a variance is 0, NaN outside the map"""
    m = np.asarray(inmap, bool)
    K, F = np.shape(q)
    H, W = m.shape
    out = np.full((K, H, W), np.nan)
    for s in range(K):
        qs = [int(v) for v in np.asarray(q)[s]]
        u1, u2 = sum(qs), sum(v * v for v in qs)
        vb = F * u2 - u1 * u1
        for y in range(H):
            for x in range(W):
                if not m[y, x]:
                    continue
                a1, a2, cc = int(w1[y, x]), int(w2[y, x]), int(c[s, y, x])
                va = F * a2 - a1 * a1
                if va == 0 or vb == 0:
                    out[s, y, x] = 0.0
                    continue
                num = F * cc - a1 * u1
                out[s, y, x] = np.float64(float(num)) / np.sqrt(np.float64(float(va)) * np.float64(float(vb)))
    return out


def maps(regs, inmap, x):
    """hydra_mi.network.maps on a registered video -> rho (K, H, W)"""
    q = quantise(x)
    c, w1, w2 = trace_maps(regs, inmap, q.T)
    return rho(c, w1, w2, q, inmap)


# ---- the host functions -----------------------------------------------------------------------------------------------
def pearson(a, b):
    """Pearson's r of two pieces of the same length: each centred on sum / n, then sum(a b) / sqrt(sum(a a) sum(b b));
    NaN for an empty or constant piece"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    n = len(a)
    if n < 1 or (a == a[0]).all() or (b == b[0]).all():
        return np.nan
    ac, bc = a - a.sum() / np.float64(n), b - b.sum() / np.float64(n)
    saa, sbb = (ac * ac).sum(), (bc * bc).sum()
    if not (saa > 0.0 and sbb > 0.0):
        return np.nan
    return (ac * bc).sum() / np.sqrt(saa * sbb)


def coactivity(x, max_lag=0):
    """-> r[i, j, max_lag + l], l in -max_lag..max_lag: x_i[:F - l] against x_j[l:] for l >= 0, x_i[-l:] against
    x_j[:F + l] for l < 0"""
    x = np.asarray(x, np.float64)
    K, F = x.shape
    r = np.full((K, K, 2 * max_lag + 1), np.nan)
    for i in range(K):
        for j in range(K):
            for l in range(-max_lag, max_lag + 1):
                if abs(l) >= F:
                    continue
                r[i, j, max_lag + l] = pearson(x[i, :F - l], x[j, l:]) if l >= 0 else pearson(x[i, -l:], x[j, :F + l])
    return r


def ensembles(r0, thr):
    """labels (K,) int32 by a union-find over the pairs with r0[i, j] >= thr, i != j"""
    K = len(r0)
    parent = list(range(K))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in range(K):
        for j in range(K):
            if i != j and r0[i][j] >= thr:             # (NaN: False)
                parent[find(i)] = find(j)
    groups = {}
    for i in range(K):
        groups.setdefault(find(i), []).append(i)
    big = sorted((g for g in groups.values() if len(g) > 1), key=lambda g: (-len(g), min(g)))
    labels = np.full(K, -1, np.int32)
    for e, g in enumerate(big):
        for i in g:
            labels[i] = e
    return labels


def ensemble_traces(x, labels):
    x = np.asarray(x, np.float64)
    E = max([int(l) for l in labels], default=-1) + 1
    out = np.zeros((E, x.shape[1]))
    for e in range(E):
        members = [i for i, l in enumerate(labels) if l == e]
        for f in range(x.shape[1]):
            acc = np.float64(0.0)
            for i in members:
                acc = acc + x[i, f]
            out[e, f] = acc / np.float64(len(members))
    return out


def lead_lag(ens, max_lag):
    r = coactivity(ens, max_lag)
    E = r.shape[0]
    lag, peak = np.zeros((E, E), np.int32), np.full((E, E), np.nan)
    for a in range(E):
        for b in range(E):
            best = None                                 # (r, -|lag|, lag): the largest wins
            for l in range(-max_lag, max_lag + 1):
                v = r[a, b, max_lag + l]
                if np.isnan(v):
                    continue
                key = (v, -abs(l), l)
                if best is None or key > best:
                    best = key
            if best is not None:
                lag[a, b], peak[a, b] = best[2], best[0]
    return lag, peak


def ensemble_map(rho_ens, thr):
    E, H, W = np.shape(rho_ens)
    out = np.full((H, W), -1, np.int16)
    for y in range(H):
        for x in range(W):
            top = None
            for e in range(E):
                v = rho_ens[e][y][x]
                if not np.isnan(v) and (top is None or v > top):
                    top, out[y, x] = v, e
            if top is None or not top >= thr:
                out[y, x] = -1
    return out


def strain_coupling(ens, J):
    ens, J = np.asarray(ens, np.float64), np.asarray(J, np.float64)
    out = np.full((ens.shape[0], J.shape[1]), np.nan)
    for e in range(ens.shape[0]):
        for t in range(J.shape[1]):
            if np.isfinite(J[:, t]).all() and np.isfinite(ens[e]).all():
                out[e, t] = pearson(ens[e], J[:, t])
    return out


# ---- the planted video with ensembles ---------------------------------------------------------------------------------
ENSEMBLES = dict(E=3, p_ens=0.05, p_drop=0.05, p_own=0.005, follow=(2, 0, 8))     # ensemble 2 is ensemble 0, 8 frames later


def planted_ensemble(i):
    """cell i of the 4 x 3 grid -> its ensemble: neighbours on the grid are in different ones"""
    return i % ENSEMBLES["E"]


def planted_video(seed):
    """The model of roi_ref.planted_video (128 x 128, 300 frames, 12 elliptical Gaussian cells on a jittered 4 x 3 grid,
    a <- 0.8 a + event clipped at 1, static texture, integer noise, an AR(1) neuropil on every pixel) with the events of
    ensembles: three ensembles of four cells (cell i in ensemble i mod 3); an ensemble has Bernoulli(0.05) events, those of
    ensemble 2 being ensemble 0's 8 frames later; a member takes each of them with probability 0.95 and has
    Bernoulli(0.005) events of its own -> (video (F, H, W) uint8, centres (12, 2) int (col, row), activity (12, F))."""
    P = roi_ref.PLANTED
    H, W, F, K = P["H"], P["W"], P["F"], P["K"]
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 121, (H, W)).astype(np.float64)
    cs = np.array([(20 + gx * 28 + rng.integers(-4, 5), 24 + gy * 36 + rng.integers(-4, 5)) for gy in range(3) for gx in range(4)])
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = []
    for cx, cy in cs:
        sa, sb = rng.uniform(P["sigma_lo"], P["sigma_hi"], 2)
        th = rng.uniform(0.0, np.pi)
        a = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        b = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        blobs.append(np.exp(-(a * a / (2 * sa * sa) + b * b / (2 * sb * sb))))
    ev = [rng.random(F) < ENSEMBLES["p_ens"] for _ in range(ENSEMBLES["E"])]
    late, early, d = ENSEMBLES["follow"]
    ev[late] = np.concatenate((np.zeros(d, bool), ev[early][:F - d]))
    act = np.zeros((K, F))
    for i in range(K):
        s = (ev[planted_ensemble(i)] & (rng.random(F) >= ENSEMBLES["p_drop"])) | (rng.random(F) < ENSEMBLES["p_own"])
        a = 0.0
        for k in range(F):
            a = a * 0.8 + (1.0 if s[k] else 0.0)
            act[i, k] = min(a, 1.0)
    npil = np.zeros(F)
    x = 0.0
    for k in range(F):
        x = P["ar"] * x + rng.normal()
        npil[k] = x
    npil = P["neuropil"] * (npil - npil.min()) / (npil.max() - npil.min())
    v = np.empty((F, H, W), np.uint8)
    for k in range(F):
        f = base + npil[k] + sum(P["amp"] * act[i, k] * blobs[i] for i in range(K)) + rng.integers(-P["noise"], P["noise"] + 1, (H, W))
        v[k] = np.clip(np.rint(f), 0, 255)
    return v, cs, act


def planted_scene(seed, uv):
    """The planted video as the tracker sees it (roi_ref.planted_scene): the first half of the frames with the mesh at
    rest, the second half with mesh and frame moved by roi_ref.PLANTED_SHIFT -> (frames, states (F, 4N), centres)"""
    v, cs, _ = planted_video(seed)
    F = v.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = roi_ref.PLANTED_SHIFT
    frames = v.copy()
    frames[F // 2:] = np.roll(v[F // 2:], (dr, dc), axis=(1, 2))     # (what wraps round lands in the margin: never read)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    return frames, np.array([rest if k < F // 2 else moved for k in range(F)]), cs


def planted_labels():
    """the labels hydra_mi.network.ensembles gives the planted cells: equal sizes, so numbered by lowest member"""
    return np.array([planted_ensemble(i) for i in range(roi_ref.PLANTED["K"])], np.int32)


def figures(dff, max_lag=10):
    """The two figures of the planted video from dF/F (F, 12): (the lowest lag-0 correlation within an ensemble, the
    highest between two ensembles), and the ensemble 0 -> 2 lead: (lag of the largest r, that r, r at lag 0)"""
    x = np.asarray(dff, np.float64).T
    r0 = coactivity(x)[:, :, 0]
    lab = planted_labels()
    same = lab[:, None] == lab[None, :]
    off = ~np.eye(len(lab), dtype=bool)
    ens = ensemble_traces(x, lab)
    lag, peak = lead_lag(ens, max_lag)
    return r0[same & off].min(), r0[~same].max(), (int(lag[0, 2]), peak[0, 2], pearson(ens[0], ens[2]))
