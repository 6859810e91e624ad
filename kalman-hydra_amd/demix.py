"""Demixing of overlapping cells: footprints ("shapes") and traces fitted together to the registered video kept on the
device.

hydra_mi.roi gives a contested pixel to the nearer centre, and the trace of an ROI carries whatever a neighbour's blob
adds to its pixels.  Here the video round the seeds is modelled as

    v_k(p) = static(p) + neuropil_k + sum_s a_s(p) c_s(k),    a_s >= 0, a_s one 4-connected patch round seed s,

and a_s and c_s are fitted in turn, starting from the ROIs and their corrected traces:

  shapes given traces   the traces are centred and quantised to int32, q; the device gives D_s(p) = sum_k v_k(p) q_s(k)
                        (hm_body_rec_trace_products), the host M = Q^T Q and the ring term, all whole numbers; two
                        sweeps of HALS over the seeds, then the support rule: values below keep x the largest go, and of
                        the rest the part 4-connected to the seed pixel stays (roi.grow's rule).
  traces given shapes   the shapes are quantised to uint16, a_q; the device gives sum_p a_q,s(p) v_k(p)
                        (hm_body_rec_weighted_sums), the host G = A_q^T A_q and the ring term; G c_k = d_k is solved by a
                        Cholesky factorisation written out here, index by index in a fixed order.

Every whole number is formed in integers and every floating-point step is written once, in a fixed order:
tests/demix_ref.py restates all of it and the two agree bit for bit.

    body = BodyReadout(kf, keep=True)
    ... track ...
    res = demix.extract(body, points)
"""
import math

import numpy as np

from . import roi

QBITS = 20              # traces are quantised to +-2^20
AMAX = 65535            # shapes are quantised to 0..65535


def _overlap(S, dr, dc):
    """Windows of S x S round seeds s and t, t's centre (dr, dc) rows and columns from s's -> the slices (rows of s,
    columns of s, rows of t, columns of t) of the pixels they share, or None."""
    if abs(dr) >= S or abs(dc) >= S:
        return None
    r0, r1 = max(0, dr), min(S, S + dr)
    c0, c1 = max(0, dc), min(S, S + dc)
    return slice(r0, r1), slice(c0, c1), slice(r0 - dr, r1 - dr), slice(c0 - dc, c1 - dc)


def _pairs(seeds, S):
    P = len(seeds)
    out = {}
    for s in range(P):
        for t in range(P):
            if t != s:
                o = _overlap(S, int(seeds[t][1]) - int(seeds[s][1]), int(seeds[t][0]) - int(seeds[s][0]))
                if o is not None:
                    out[s, t] = o
    return out


def quantise_traces(c):
    """(F, P) float64 -> (q (F, P) int32, m (P,) float64): every column centred over time (the mean is the exactly rounded
    sum over F) and scaled so that its largest magnitude m becomes 2^20: q = rint(c^ 2^20 / m); 0 for a flat column."""
    c = np.asarray(c, np.float64)
    F, P = c.shape
    q = np.zeros((F, P), np.int32)
    m = np.zeros(P)
    for s in range(P):
        col = np.ascontiguousarray(c[:, s])
        ch = col - np.float64(math.fsum(col.tolist()) / F)
        m[s] = np.abs(ch).max()
        if m[s] > 0.0:
            q[:, s] = np.rint(ch * np.float64(2.0 ** QBITS) / m[s]).astype(np.int32)
    return q, m


def cholesky(G):
    """G (P, P) float64 symmetric -> L lower triangular with L L^T = G, column by column, every sum subtracted in
    ascending index order; None and the failing index when a pivot is not positive."""
    P = G.shape[0]
    L = np.zeros((P, P))
    for j in range(P):
        acc = G[j, j]
        for k in range(j):
            acc = acc - L[j, k] * L[j, k]
        if not acc > 0.0:
            return None, j
        L[j, j] = np.sqrt(acc)
        for i in range(j + 1, P):
            acc = G[i, j]
            for k in range(j):
                acc = acc - L[i, k] * L[j, k]
            L[i, j] = acc / L[j, j]
    return L, -1


def solve(L, d):
    """L from cholesky, d (F, P) -> x (F, P) with L L^T x_k = d_k: forward and back substitution, loops over the P indices
    (sums subtracted in ascending index order), every frame at once."""
    F, P = d.shape
    z = np.empty((P, F))
    for i in range(P):
        acc = np.array(d[:, i], np.float64)
        for k in range(i):
            acc = acc - L[i, k] * z[k]
        z[i] = acc / L[i, i]
    x = np.empty((P, F))
    for i in range(P - 1, -1, -1):
        acc = z[i].copy()
        for k in range(i + 1, P):
            acc = acc - L[k, i] * x[k]
        x[i] = acc / L[i, i]
    return np.ascontiguousarray(x.T)


def solve_traces(G, A, ws, gsum, ngs):
    """Traces given shapes, from whole numbers: G (P, P) int64 = A_q^T A_q, A (P, S, S) int64 the quantised shapes, ws and
    gsum (F, P) Python integers -- the sums over the shapes and over the rings of every frame --, ngs (P,) the ring counts
    (0 counted as 1).  d = (n_G ws - sum a_q gsum) / n_G, G c = d by cholesky and solve, C = c sum a_q^2 / sum a_q.
    -> (C (F, P) float64, sa (P,) the sums of the shapes, -1), or (None, sa, the index whose pivot is not positive).
    (hydra_mi.deeptrace runs the same step on the sums of the 16-bit frames.)"""
    P = G.shape[0]
    F = ws.shape[0]
    sa = [int(A[s].sum()) for s in range(P)]
    d = np.empty((F, P))
    for s in range(P):
        d[:, s] = (ngs[s] * ws[:, s] - sa[s] * gsum[:, s]).astype(np.float64) / np.float64(ngs[s])
    L, bad = cholesky(G.astype(np.float64))
    if L is None:
        return None, sa, bad
    c = solve(L, d)
    Cn = np.empty((F, P))
    for s in range(P):
        Cn[:, s] = c[:, s] * (np.float64(int(G[s, s])) / np.float64(sa[s]))
    return Cn, sa, -1


def _worst_pair(G):
    P = G.shape[0]
    best, pair = -1.0, (0, 0)
    for s in range(P):
        for t in range(s + 1, P):
            if G[s, s] > 0 and G[t, t] > 0:
                o = float(G[s, t]) / math.sqrt(float(G[s, s]) * float(G[t, t]))
                if o > best:
                    best, pair = o, (s, t)
    return pair, best


def shape_step(D, M, rq, n_G, valid, b, pairs, keep):
    """One update of the shapes in the units of the quantised traces.  D (P, S, S) int64 trace products, M (P, P) int64,
    rq (P,) Python integers sum_k gsum_s(k) q_s(k), n_G (P,) ring counts (0 counted as 1: its ring sums are 0), valid
    (P, S, S) window pixels on the frame and in the map, b (P, S, S) float64 the start (changed in place)
    -> (b, empty (P,) bool): after two HALS sweeps in index order and the support rule; an empty seed's b is undefined."""
    P, S = D.shape[0], D.shape[1]
    Mf = M.astype(np.float64)
    y = np.empty((P, S, S))
    for s in range(P):
        ng = max(int(n_G[s]), 1)
        y[s] = (ng * roi._ints(D[s]) - rq[s]).astype(np.float64) / np.float64(ng)
    for sweep in range(2):
        for s in range(P):
            if M[s, s] == 0:
                continue
            acc = np.zeros((S, S))
            for t in range(P):
                if (s, t) in pairs:
                    rs, cs, rt, ct = pairs[s, t]
                    acc[rs, cs] = acc[rs, cs] + Mf[s, t] * b[t][rt, ct]
            x = (y[s] - acc) / Mf[s, s]
            b[s] = np.where(valid[s] & (x > 0.0), x, 0.0)
    empty = np.zeros(P, bool)
    for s in range(P):
        top = b[s].max()
        if M[s, s] == 0 or not top > 0.0:
            empty[s] = True
            continue
        g = roi.grow(b[s], np.float64(keep) * top)
        if not g.any():
            empty[s] = True
            continue
        b[s] = np.where(g, b[s], 0.0)
    return b, empty


def extract(body, points, iters=6, keep=0.25, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=None, alpha=0.7, q=10.0, half=100):
    """roi.extract, then `iters` rounds of shapes given traces and traces given shapes -> its dict and
      shapes (P, 2R+1, 2R+1) float64   the footprints, largest value 1 (shapes_q / 65535)
      shapes_q (same) uint16           as they went to the device
      C (F, P) float64                 the demixed traces in grey levels per footprint pixel: the solution of G c = d
                                       for the shapes shapes_q, times sum a_q^2 / sum a_q
      dff_demixed (F, P) float64       (C - baseline(C)) / baseline(F_roi)
      demix_change (iters,) float64    |C - C_before| / |C_before| (Frobenius) of every round
      demix_kept (iters, P) bool       the seed's shape came out empty in that round and kept its previous one
      demix_D, demix_M, demix_G        the whole numbers of the last round: trace products (P, 2R+1, 2R+1) int64,
                                       Q^T Q and A_q^T A_q (P, P) int64
    keep 0 switches the support rule off."""
    iters = int(iters)
    if iters < 1:
        raise ValueError("demix.extract: iters %d" % iters)
    if not 0.0 <= float(keep) < 1.0:
        raise ValueError("demix.extract: keep %g outside 0 <= keep < 1" % keep)
    e = roi.extract(body, points, r_disc=r_disc, r_in=r_in, r_out=r_out, R=R, thr=thr, alpha=alpha, q=q, half=half)
    r = body.r
    F = r.body_rec_count()
    if F >= 1 << 22:
        raise OverflowError("demix.extract: %d frames: Q^T Q could pass 2^63" % F)
    m = body.tri_of_pixel >= 0
    H, W = m.shape
    seeds = roi.seeds_of(points)
    P, S = seeds.shape[0], 2 * int(R) + 1
    labels = e["roi_labels"]
    if (e["roi_counts"] < 1).any():
        raise ValueError("demix.extract: seed %d has no ROI pixel of its own" % int(np.flatnonzero(e["roi_counts"] < 1)[0]))
    w, n_G, Rg = roi.ring_weights(labels, m, seeds, r_in, r_out)      # the ring: fixed for the whole run
    gsum = roi._ints(r.body_rec_weighted_sums(seeds, w, Rg))          # (F, P) Python integers
    ngs = [max(int(n), 1) for n in n_G]
    valid = np.zeros((P, S, S), bool)
    a_q = np.zeros((P, S, S), np.uint16)
    for s in range(P):
        rr, cc, on = roi._window(H, W, seeds[s], R)
        valid[s] = on & m[rr, cc]
        a_q[s] = np.where(valid[s] & (labels[rr, cc] == s), AMAX, 0)
        if not a_q[s].any():
            raise ValueError("demix.extract: seed %d has no ROI pixel in its window of radius %d" % (s, R))
    pairs = _pairs(seeds, S)
    C = e["F_roi"] - e["F_np"]
    unit = np.ones(P)                                                  # v ~ sum_s (a_q,s / 65535) unit_s C_s
    change = np.zeros(iters)
    kept = np.zeros((iters, P), bool)
    for it in range(iters):
        # shapes, given traces
        Q, mag = quantise_traces(C)
        Q64 = Q.astype(np.int64)
        M = Q64.T @ Q64
        D = r.body_rec_trace_products(seeds, Q, R)
        Qo = roi._ints(Q)
        rq = [sum((gsum[:, s] * Qo[:, s]).tolist()) for s in range(P)]
        b = np.empty((P, S, S))
        for s in range(P):
            b[s] = (a_q[s].astype(np.float64) / np.float64(AMAX)) * ((unit[s] * mag[s]) / np.float64(2.0 ** QBITS))
        b, empty = shape_step(D, M, rq, n_G, valid, b, pairs, keep)
        kept[it] = empty
        for s in range(P):
            if not empty[s]:
                a_q[s] = np.rint((np.float64(AMAX) * b[s]) / b[s].max()).astype(np.uint16)
        # traces, given shapes
        A = a_q.astype(np.int64)
        G = np.zeros((P, P), np.int64)
        for s in range(P):
            G[s, s] = (A[s] * A[s]).sum()
            for t in range(P):
                if (s, t) in pairs:
                    rs, cs, rt, ct = pairs[s, t]
                    G[s, t] = (A[s][rs, cs] * A[t][rt, ct]).sum()
        ws = roi._ints(r.body_rec_weighted_sums(seeds, a_q, R))
        Cn, sa, bad = solve_traces(G, A, ws, gsum, ngs)
        if Cn is None:
            (s, t), o = _worst_pair(G)
            raise np.linalg.LinAlgError("demix.extract: round %d: the shapes' overlap matrix does not factor at seed %d; seeds "
                                        "%d and %d overlap most (%.6f of the geometric mean of their own sums of squares)"
                                        % (it, bad, s, t, o))
        for s in range(P):
            unit[s] = (np.float64(AMAX) * np.float64(sa[s])) / np.float64(int(G[s, s]))
        diff = Cn - C
        den = math.sqrt(math.fsum((C * C).ravel().tolist()))
        change[it] = math.sqrt(math.fsum((diff * diff).ravel().tolist())) / den if den > 0.0 else np.inf
        C = Cn
    dff = np.empty((F, P))
    for s in range(P):
        with np.errstate(invalid="ignore", divide="ignore"):
            dff[:, s] = (C[:, s] - roi.baseline(C[:, s], q, half)) / roi.baseline(e["F_roi"][:, s], q, half)
    e.update(shapes=a_q.astype(np.float64) / np.float64(AMAX), shapes_q=a_q, C=C, dff_demixed=dff, demix_change=change,
             demix_kept=kept, demix_D=D, demix_M=M, demix_G=G)
    return e
