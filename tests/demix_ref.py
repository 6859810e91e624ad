"""Restatement of the trace products over the recorded video (hm_body_rec_trace_products) and of the whole of
hydra_mi.demix.extract, on a registered video in host memory: whole numbers as int64 / Python integers, shapes as
full-frame images, every floating-point step in Python floats one pixel and one frame at a time (the product works on
windows and whole columns; the two agree bit for bit).  And the paired video the recovery tests run on.

`regs` (F, H, W) uint8, `inmap` the body map as a mask, `seeds` (P, 2) integer (col, row) map pixels, as in roi_ref.
"""
import functools
import math

import numpy as np

import roi_ref

QBITS = 20
AMAX = 65535


def trace_products(regs, inmap, seeds, q, R):
    """q (F, P) int32 -> (P, 2R+1, 2R+1) int64: sum_k v_k(p) q[k, s] for every window pixel on the frame and in the map,
    0 elsewhere"""
    v = np.asarray(regs).astype(np.int64)
    m = np.asarray(inmap, bool)
    F, H, W = v.shape
    assert F * 255 * 2 ** 31 < 2 ** 63
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    q = np.asarray(q)
    assert q.dtype == np.int32 and q.shape == (F, seeds.shape[0])
    S = 2 * R + 1
    out = np.zeros((seeds.shape[0], S, S), np.int64)
    for s, seed in enumerate(seeds):
        rr, cc, on = roi_ref.window(H, W, seed, R)
        x = np.where((on & m[rr, cc])[None], v[:, rr, cc], 0)
        out[s] = (x * q[:, s].astype(np.int64)[:, None, None]).sum(0)
    return out


def quantise(col):
    """one trace (F,) -> (list of F integers, its largest centred magnitude)"""
    x = [float(t) for t in col]
    mean = math.fsum(x) / len(x)
    ch = [t - mean for t in x]
    mag = max(abs(t) for t in ch)
    if not mag > 0.0:
        return [0] * len(x), 0.0
    return [int(round(t * 1048576.0 / mag)) for t in ch], mag


def cholesky(G):
    """list of lists of floats -> L (lower), or the index of the pivot that is not positive"""
    P = len(G)
    L = [[0.0] * P for _ in range(P)]
    for j in range(P):
        acc = G[j][j]
        for k in range(j):
            acc = acc - L[j][k] * L[j][k]
        if not acc > 0.0:
            return j
        L[j][j] = math.sqrt(acc)
        for i in range(j + 1, P):
            acc = G[i][j]
            for k in range(j):
                acc = acc - L[i][k] * L[j][k]
            L[i][j] = acc / L[j][j]
    return L


def chol_solve(L, d):
    """one right-hand side (list of P floats) -> the solution of L L^T x = d"""
    P = len(L)
    z = [0.0] * P
    for i in range(P):
        acc = d[i]
        for k in range(i):
            acc = acc - L[i][k] * z[k]
        z[i] = acc / L[i][i]
    x = [0.0] * P
    for i in range(P - 1, -1, -1):
        acc = z[i]
        for k in range(i + 1, P):
            acc = acc - L[k][i] * x[k]
        x[i] = acc / L[i][i]
    return x


def demix(regs, inmap, seeds, iters=6, keep=0.25, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=0.47, alpha=0.7, q=10.0,
          half=100):
    """The whole of hydra_mi.demix.extract -> the dict of roi_ref.extract and shapes, shapes_q, C, dff_demixed,
    demix_change, demix_kept, demix_D, demix_M, demix_G, and C_rounds: C after every round."""
    regs = np.asarray(regs)
    m = np.asarray(inmap, bool)
    F, H, W = regs.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    P, S = seeds.shape[0], 2 * R + 1
    e = roi_ref.extract(regs, m, seeds, r_disc=r_disc, r_in=r_in, r_out=r_out, R=R, thr=thr, alpha=alpha, q=q, half=half)
    labels = e["roi_labels"]
    assert (e["roi_counts"] >= 1).all()
    w, n_G, Rg = roi_ref.ring_weights(labels, m, seeds, r_in, r_out)
    gsum = roi_ref.weighted_sums(regs, m, seeds, w, Rg).tolist()       # [k][s] Python integers
    ng = [max(int(n), 1) for n in n_G]
    wins = [roi_ref.window(H, W, seed, R) for seed in seeds]
    ok = [on & m[rr, cc] for rr, cc, on in wins]
    # shapes as full-frame images: whole numbers 0..65535 (A) and, inside a round, floats in the traces' units (B)
    A = np.zeros((P, H, W), np.int64)
    for s in range(P):
        A[s][labels == s] = AMAX
        rr, cc, on = wins[s]
        inwin = np.zeros((H, W), bool)
        inwin[rr[ok[s]], cc[ok[s]]] = True
        A[s][~inwin] = 0
    C = (e["F_roi"] - e["F_np"]).tolist()                               # [k][s]
    unit = [1.0] * P
    change, kept, rounds = [], [], []
    for it in range(iters):
        Q, mag = [], []
        for s in range(P):
            qs, ms = quantise([C[k][s] for k in range(F)])
            Q.append(qs)
            mag.append(ms)
        Qa = np.array(Q, np.int32).T.copy()                             # (F, P)
        M = [[sum(Q[s][k] * Q[t][k] for k in range(F)) for t in range(P)] for s in range(P)]
        D = trace_products(regs, m, seeds, Qa, R)
        B = np.zeros((P, H, W))
        y = []
        for s in range(P):
            B[s] = (A[s].astype(np.float64) / 65535.0) * ((unit[s] * mag[s]) / 1048576.0)
            rq = sum(gsum[k][s] * Q[s][k] for k in range(F))
            y.append([[float(ng[s] * int(D[s, i, j]) - rq) / float(ng[s]) for j in range(S)] for i in range(S)])
        for sweep in range(2):
            for s in range(P):
                if M[s][s] == 0:
                    continue
                rr, cc, on = wins[s]
                new = np.zeros((H, W))
                for i in range(S):
                    for j in range(S):
                        if not ok[s][i, j]:
                            continue
                        r_, c_ = rr[i, j], cc[i, j]
                        acc = 0.0
                        for t in range(P):
                            if t != s:
                                acc = acc + float(M[s][t]) * float(B[t, r_, c_])
                        x = (y[s][i][j] - acc) / float(M[s][s])
                        new[r_, c_] = x if x > 0.0 else 0.0
                B[s] = new
        empty = []
        for s in range(P):
            rr, cc, on = wins[s]
            win = np.where(ok[s], B[s][rr, cc], 0.0)
            top = float(win.max())
            g = roi_ref.grow(win, keep * top) if (M[s][s] != 0 and top > 0.0) else np.zeros((S, S), bool)
            empty.append(not g.any())
            if empty[s]:
                continue
            A[s] = 0
            for i in range(S):
                for j in range(S):
                    if g[i, j] and ok[s][i, j]:
                        A[s][rr[i, j], cc[i, j]] = int(round(65535.0 * float(win[i, j]) / top))
        kept.append(empty)
        G = [[int((A[s] * A[t]).sum()) for t in range(P)] for s in range(P)]
        sa = [int(A[s].sum()) for s in range(P)]
        aq = np.zeros((P, S, S), np.uint16)
        for s in range(P):
            rr, cc, on = wins[s]
            aq[s] = np.where(ok[s], A[s][rr, cc], 0)
        ws = roi_ref.weighted_sums(regs, m, seeds, aq, R).tolist()
        L = cholesky([[float(G[s][t]) for t in range(P)] for s in range(P)])
        if isinstance(L, int):
            raise np.linalg.LinAlgError("pivot %d" % L)
        Cn = []
        for k in range(F):
            d = [float(ng[s] * ws[k][s] - sa[s] * gsum[k][s]) / float(ng[s]) for s in range(P)]
            c = chol_solve(L, d)
            Cn.append([c[s] * (float(G[s][s]) / float(sa[s])) for s in range(P)])
        for s in range(P):
            unit[s] = (65535.0 * float(sa[s])) / float(G[s][s])
        num = math.fsum((Cn[k][s] - C[k][s]) * (Cn[k][s] - C[k][s]) for k in range(F) for s in range(P))
        den = math.fsum(C[k][s] * C[k][s] for k in range(F) for s in range(P))
        change.append(math.sqrt(num) / math.sqrt(den) if den > 0.0 else np.inf)
        C = Cn
        rounds.append(np.array(C, np.float64).reshape(F, P))
    C = np.array(C, np.float64).reshape(F, P)
    dff = np.empty((F, P))
    for s in range(P):
        with np.errstate(invalid="ignore", divide="ignore"):
            dff[:, s] = (C[:, s] - roi_ref.baseline(C[:, s], q, half)) / roi_ref.baseline(e["F_roi"][:, s], q, half)
    e.update(shapes=aq.astype(np.float64) / 65535.0, shapes_q=aq, C=C, dff_demixed=dff, demix_change=np.array(change),
             demix_kept=np.array(kept, bool).reshape(iters, P), demix_D=D, demix_M=np.array(M, np.int64),
             demix_G=np.array(G, np.int64), C_rounds=rounds)
    return e


def worst_cell(traces, act):
    """the lowest correlation of a cell's trace (F, K) with its planted activity (K, F)"""
    return min(np.corrcoef(traces[:, s], act[s])[0, 1] for s in range(act.shape[0]))


# ---- the paired video ---------------------------------------------------------------------------------------------------
def paired_video(seed, sep):
    """roi_ref.planted_video's model (texture 40..120, elliptical Gaussian cells of sigma 1.5..2.5 px and amplitude 50 x
    activity, neuropil 0..30, noise -8..8, 300 frames of 128 x 128) with the twelve cells as six pairs: pair centres on a
    2 x 3 grid at (30 + 56 gx +- 4, 24 + 36 gy +- 4), the partner `sep` px away in a random direction, rounded to whole
    pixels.  Cells 2i and 2i + 1 are pair i -> (video, centres (12, 2) (col, row), activity (12, F), neuropil (F,))."""
    PL = roi_ref.PLANTED
    H, W, F, K = PL["H"], PL["W"], PL["F"], PL["K"]
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 121, (H, W)).astype(np.float64)
    cs = []
    for gy in range(3):
        for gx in range(2):
            cx, cy = 30 + 56 * gx + rng.integers(-4, 5), 24 + 36 * gy + rng.integers(-4, 5)
            th = rng.uniform(0.0, 2.0 * np.pi)
            cs.append((cx, cy))
            cs.append((cx + int(np.rint(sep * np.cos(th))), cy + int(np.rint(sep * np.sin(th)))))
    cs = np.array(cs[:K])
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = []
    for cx, cy in cs:
        sa, sb = rng.uniform(PL["sigma_lo"], PL["sigma_hi"], 2)
        th = rng.uniform(0.0, np.pi)
        a = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        b = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        blobs.append(np.exp(-(a * a / (2 * sa * sa) + b * b / (2 * sb * sb))))
    act = np.zeros((K, F))
    for i in range(K):
        ev = rng.random(F) < 0.06
        a = 0.0
        for k in range(F):
            a = a * 0.8 + (1.0 if ev[k] else 0.0)
            act[i, k] = min(a, 1.0)
    npil = np.zeros(F)
    x = 0.0
    for k in range(F):
        x = PL["ar"] * x + rng.normal()
        npil[k] = x
    npil = PL["neuropil"] * (npil - npil.min()) / (npil.max() - npil.min())
    v = np.empty((F, H, W), np.uint8)
    for k in range(F):
        f = base + npil[k] + sum(PL["amp"] * act[i, k] * blobs[i] for i in range(K)) + \
            rng.integers(-PL["noise"], PL["noise"] + 1, (H, W))
        v[k] = np.clip(np.rint(f), 0, 255)
    return v, cs, act, npil


def paired_scene(seed, sep, uv):
    """The paired video as the tracker sees it (roi_ref.planted_scene's pattern): the first half of the frames with the
    mesh at rest, the second half with mesh and frame moved by roi_ref.PLANTED_SHIFT
    -> (frames, states (F, 4N), centres, activity)"""
    v, cs, act, _ = paired_video(seed, sep)
    F = v.shape[0]
    p = np.asarray(uv, np.float32).astype(np.float64)
    N = p.shape[0]
    dc, dr = roi_ref.PLANTED_SHIFT
    frames = v.copy()
    frames[F // 2:] = np.roll(v[F // 2:], (dr, dc), axis=(1, 2))
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * N)))
    moved = np.concatenate(((p + np.array([dc, dr], np.float64)).reshape(-1), np.zeros(2 * N)))
    states = np.array([rest if k < F // 2 else moved for k in range(F)])
    return frames, states, cs, act


@functools.lru_cache(maxsize=None)
def paired_run(seed, sep, iters=6, keep=0.25):
    """paired_video and its restated demixing (defaults of the product, thr = its default, alpha = 1), computed once for
    all the tests that look at it; nothing of it is to be changed -> (video, centres, activity, dict of demix)"""
    v, cs, act, _ = paired_video(seed, sep)
    return v, cs, act, demix(v, roi_ref.planted_map(), cs, iters=iters, keep=keep, alpha=1.0)
