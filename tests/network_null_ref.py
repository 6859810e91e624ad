"""Restatement of the significance of co-activity maps against circularly shifted traces (include/hydra_mi.h:
hm_body_rec_trace_null; hydra_mi.network shifts, surrogates, map_null, coactivity_null) in loops and
Python integers.

`regs` is the registered video (F, H, W) uint8, `inmap` the body map as a mask, `q` whole-number columns (F, L) as the
device takes them (column 0 the observed trace, the others its surrogates), `vb` (L,) the host's F u2 - u1^2 per column
as binary64.  Every floating-point step is written out once.  trace_null is the rule in Python integers, pixel by pixel;
trace_null_np the same numbers in vectorised int64 NumPy for videos too large for that (the two are compared in
tests/test_network_null_cpu.py).
"""
import numpy as np

import network_ref

QMAX = 32767
MIN_SHIFTS = 19


def shifts(F, n, guard, seed=0):
    cand = []
    for s in range(1, F):
        if min(s, F - s) > guard:
            cand.append(s)
    if len(cand) < MIN_SHIFTS:
        raise ValueError("%d candidates" % len(cand))
    if len(cand) <= n:
        return np.array(cand, np.int64)
    return np.sort(np.random.default_rng(seed).choice(np.array(cand, np.int64), size=n, replace=False))


def surrogates(q_row, sh):
    """(F, 1 + S) int32: column 0 the trace, column j the trace moved forward by sh[j - 1] frames, circularly"""
    F = len(q_row)
    out = np.zeros((F, 1 + len(sh)), np.int32)
    for k in range(F):
        out[k, 0] = q_row[k]
        for j, s in enumerate(sh):
            out[(k + int(s)) % F, 1 + j] = q_row[k]
    return out


def vb_of(q_col):
    """F u2 - u1^2 of a column in Python integers, rounded once"""
    qs = [int(v) for v in q_col]
    return float(len(qs) * sum(v * v for v in qs) - sum(qs) ** 2)


def rho_one(num, va, vb):
    """one conversion each, one product, one square root, one division; 0 where a variance is 0"""
    if va == 0 or vb == 0.0:
        return 0.0
    return float(np.float64(float(num)) / np.sqrt(np.float64(float(va)) * np.float64(vb)))


def trace_null(regs, inmap, q, vb):
    """hm_body_rec_trace_null in Python integers -> dict tmax, tmin (L,) float64, ge, le (H, W) uint32"""
    regs, m, q = np.asarray(regs), np.asarray(inmap, bool), np.asarray(q)
    F, L = q.shape
    H, W = m.shape
    assert regs.shape == (F, H, W) and 2 <= L <= 4096 and F * F * 255 * QMAX < 2 ** 63
    cols = [[int(v) for v in q[:, s]] for s in range(L)]
    assert all(abs(v) <= QMAX for col in cols for v in col)
    u1 = [sum(col) for col in cols]
    tmax, tmin = [None] * L, [None] * L
    ge, le = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    for y in range(H):
        for x in range(W):
            if not m[y, x]:
                continue
            v = [int(t) for t in regs[:, y, x]]
            w1, w2 = sum(v), sum(t * t for t in v)
            va = F * w2 - w1 * w1
            num0 = None
            for s in range(L):
                num = F * sum(a * b for a, b in zip(v, cols[s])) - w1 * u1[s]
                if s == 0:
                    num0 = num
                else:
                    ge[y, x] += num >= num0
                    le[y, x] += num <= num0
                r = rho_one(num, va, vb[s])
                tmax[s] = r if tmax[s] is None or r > tmax[s] else tmax[s]
                tmin[s] = r if tmin[s] is None or r < tmin[s] else tmin[s]
    return dict(tmax=np.array(tmax, np.float64), tmin=np.array(tmin, np.float64), ge=ge, le=le)


def trace_null_np(regs, inmap, q, vb):
    """The same in vectorised int64 NumPy.  The products c are made by a binary64 matrix product, exact because every
    partial sum is a whole number below 2^53 (asserted)."""
    regs, m = np.asarray(regs), np.asarray(inmap, bool)
    q = np.asarray(q).astype(np.int64)
    F, L = q.shape
    assert F * 255 * QMAX < 2 ** 53 and F * F * 255 * QMAX < 2 ** 63 and np.abs(q).max(initial=0) <= QMAX
    v = regs[:, m].astype(np.int64)                                   # (F, P)
    c = (v.T.astype(np.float64) @ q.astype(np.float64)).astype(np.int64)       # (P, L)
    w1, w2, u1 = v.sum(0), (v * v).sum(0), q.sum(0)
    num = F * c - w1[:, None] * u1[None, :]
    va = (F * w2 - w1 * w1).astype(np.float64)
    vb = np.asarray(vb, np.float64)
    flat = (va == 0.0)[:, None] | (vb == 0.0)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(flat, 0.0, num.astype(np.float64) / np.sqrt(va[:, None] * vb[None, :]))
    ge, le = np.zeros(m.shape, np.uint32), np.zeros(m.shape, np.uint32)
    ge[m] = (num[:, 1:] >= num[:, :1]).sum(1)
    le[m] = (num[:, 1:] <= num[:, :1]).sum(1)
    return dict(tmax=rho.max(0), tmin=rho.min(0), ge=ge, le=le)


def p_from_null(null, obs):
    """(1 + #{s: null[s] >= obs}) / (S + 1) per value of obs: the count is a whole number, then one division; NaN stays"""
    null, obs = np.asarray(null, np.float64).reshape(-1), np.asarray(obs, np.float64)
    S = len(null)
    out = np.full(obs.shape, np.nan)
    flat, res = obs.reshape(-1), out.reshape(-1)
    for i0 in range(0, len(flat), 4096):
        o = flat[i0:i0 + 4096]
        with np.errstate(invalid="ignore"):
            count = (null[None, :] >= o[:, None]).sum(1)
        res[i0:i0 + 4096] = np.where(np.isnan(o), np.nan, (1 + count).astype(np.float64) / np.float64(S + 1))
    return out


def map_null(regs, inmap, x, n=1000, guard=10, seed=0, alpha=0.05, reduce=trace_null_np):
    """hydra_mi.network.map_null on a registered video"""
    m = np.asarray(inmap, bool)
    rho = network_ref.maps(regs, m, x)
    q = network_ref.quantise(x)
    K, F = q.shape
    sh = shifts(F, n, guard, seed)
    S = len(sh)
    out = dict(rho=rho, shifts=sh, rho_max=np.zeros((K, S)), rho_min=np.zeros((K, S)), p_map=np.zeros(rho.shape),
               p_pix=np.zeros(rho.shape), sig=np.zeros(rho.shape, bool))
    for k in range(K):
        Q = surrogates(q[k], sh)
        o = reduce(regs, m, Q, np.array([vb_of(Q[:, s]) for s in range(S + 1)]))
        assert o["tmax"][0] == np.nanmax(rho[k]) and o["tmin"][0] == np.nanmin(rho[k])
        out["rho_max"][k], out["rho_min"][k] = o["tmax"][1:], o["tmin"][1:]
        out["p_map"][k] = p_from_null(o["tmax"][1:], rho[k])
        out["p_pix"][k] = np.where(m, (1 + o["ge"].astype(np.int64)) / np.float64(S + 1), np.nan)
        out["sig"][k] = np.where(np.isnan(out["p_map"][k]), 2.0, out["p_map"][k]) <= alpha
    return out


def coactivity_null(x, sh):
    """p_r (K, K): per ordered pair i != j, (1 + #{s: F sum q_i roll(q_j, s) - u1_i u1_j >= the same unrolled}) / (S + 1),
    Python integers; NaN on the diagonal and for a trace that is not finite"""
    x = np.asarray(x, np.float64)
    K, F = x.shape
    S = len(sh)
    q = [None] * K
    for i in range(K):
        if np.isfinite(x[i]).all():
            q[i] = [int(t) for t in network_ref.quantise(x[i:i + 1])[0]]
    p = np.full((K, K), np.nan)
    for i in range(K):
        for j in range(K):
            if i == j or q[i] is None or q[j] is None:
                continue
            u = sum(q[i]) * sum(q[j])
            obs = F * sum(a * b for a, b in zip(q[i], q[j])) - u
            qi, qj = np.array(q[i], np.int64), np.array(q[j], np.int64)          # (|sum| <= F x 32767^2 < 2^63)
            count = 0
            for s in sh:
                moved = np.concatenate((qj[F - int(s):], qj[:F - int(s)]))       # q_j, int(s) frames later
                count += F * int((qi * moved).sum()) - u >= obs
            p[i, j] = np.float64(1 + count) / np.float64(S + 1)
    return p


def map_sig(emap, sig):
    """`emap` with -1 where the winning ensemble's pixel is not significant"""
    out = np.array(emap, np.int16)
    H, W = out.shape
    for y in range(H):
        for x in range(W):
            if out[y, x] >= 0 and not sig[out[y, x], y, x]:
                out[y, x] = -1
    return out
