"""Co-active cells: which pixels of the animal go with a cell, which cells fire together, which group leads which.

The traces are the dF/F of hydra_mi.roi or hydra_mi.demix as they are, (cells, frames).  The spatial half runs over the
registered video kept on the device (hm_body_rec_trace_maps in include/hydra_mi.h, csrc/network_kernels.h: every trace
against every pixel of the record, exact integer sums); everything else is host arithmetic in NumPy on cells x cells x
lags numbers.  Exact whole numbers come first, then one rounding each, the rule of roi.footprints.

  quantise        a trace as whole numbers -32767..32767, what the device multiplies into the record
  maps            rho_s(p): the correlation over time of every pixel of the body map with every trace
  coactivity      Pearson's r of every pair of traces at every lag -max_lag..max_lag
  ensembles       the connected components of the graph r(lag 0) >= thr: the cells that fire together
  ensemble_traces, lead_lag, ensemble_map, strain_coupling, colour_map; extract does all of it in turn
  shifts, surrogates, map_null, coactivity_null   significance against circularly shifted traces: the null of a map is the
                  largest rho over all its pixels per surrogate, reduced on the device (hm_body_rec_trace_null,
                  csrc/network_null_kernels.h)

    body = BodyReadout(kf, keep=True, stats=True)
    ... track ...
    e = roi.extract(body, points)
    r = network.coactivity(e["dff"].T, max_lag=10)
    labels = network.ensembles(r[:, :, 10])
    ens = network.ensemble_traces(e["dff"].T, labels)
    lag, peak = network.lead_lag(ens, 10)
    which = network.ensemble_map(network.maps(body, ens), 0.3)

tests/network_ref.py and tests/network_null_ref.py restate every step in loops and Python integers; the two agree bit
for bit.
"""
import numpy as np

from . import cellview, videoio
from .body import BodyReadout

QMAX = 32767                          # the largest |q| hm_body_rec_trace_maps takes
LMAX = 1024                           # the most traces of one call
NULL_LMAX = 4096                      # the most columns hm_body_rec_trace_null takes: the trace and 4095 surrogates
MIN_SHIFTS = 19                       # fewer surrogates cannot reach p = 0.05: (1 + 0) / (19 + 1)

#: halfway between the lowest correlation of dF/F within a planted ensemble (0.682) and the highest between two
#: ensembles (0.424) of the planted video with ensembles (tests/network_ref.py, seeds 0..4; tests/test_network_cpu.py
#: measures both)
DEFAULT_THR = 0.55
#: halfway between the lowest map value of its own ensemble at a planted centre (0.812) and the highest elsewhere: another
#: ensemble's map at a centre, or any map more than 8 px from every cell (0.428); same video and seeds
DEFAULT_MAP_THR = 0.62
DEFAULT_LAG = 10


def quantise(traces):
    """Traces (K, F) -> int32 (K, F): rint(32767 x / max|x|) per cell, the product first, then the division, then the
    rounding.  An all-zero trace stays zero; a value that is not finite raises."""
    x = np.asarray(traces, np.float64)
    if x.ndim != 2:
        raise ValueError("network: traces of shape %r (need cells x frames)" % (x.shape,))
    if not np.isfinite(x).all():
        k, f = np.argwhere(~np.isfinite(x))[0]
        raise ValueError("network: trace %d is not finite in frame %d" % (k, f))
    q = np.zeros(x.shape, np.int32)
    for k in range(x.shape[0]):
        top = np.abs(x[k]).max() if x.shape[1] else 0.0
        if top > 0.0:
            q[k] = np.rint(np.float64(QMAX) * x[k] / top).astype(np.int32)
    return q


def rho_from_sums(c, w1, w2, q, inmap):
    """rho (K, H, W) float64 from the sums of body_rec_trace_maps for the quantised traces q (K, F):
    (F c - w1 u1) / sqrt((F w2 - w1^2)(F u2 - u1^2)), u1 = sum q, u2 = sum q^2.  The first two whole numbers and the
    numerator are formed in int64 (exact: hm_body_rec_trace_maps refuses what could pass 2^63), F u2 - u1^2 in Python
    integers (it may pass 2^63 beyond 92681 frames); each is rounded once to binary64, then one product, one square root,
    one division.  0 where a variance is 0, NaN outside the map."""
    q = np.asarray(q, np.int64)
    K, F = q.shape
    m = np.asarray(inmap, bool)
    c = np.asarray(c).astype(np.int64).reshape((K,) + m.shape)
    w1, w2 = np.asarray(w1).astype(np.int64), np.asarray(w2).astype(np.int64)
    u1 = q.sum(1)
    va = (F * w2 - w1 * w1).astype(np.float64)
    rho = np.empty(c.shape, np.float64)
    for s in range(K):
        qs = [int(v) for v in q[s]]
        vb = np.float64(float(F * sum(v * v for v in qs) - sum(qs) ** 2))
        num = (F * c[s] - w1 * u1[s]).astype(np.float64)
        flat = (va == 0.0) | (vb == 0.0)              # (whole numbers: the rounded value is 0 only when the integer is)
        with np.errstate(invalid="ignore", divide="ignore"):
            rho[s] = np.where(flat, 0.0, num / np.sqrt(va * vb))
        rho[s][~m] = np.nan
    return rho


def maps(body, traces):
    """rho (K, H, W) float64: the correlation over the frames a BodyReadout(keep=True) has recorded of every pixel of the
    body map with every trace (K, F), the traces quantised (`quantise`).  0 where the pixel or the trace is constant, NaN
    outside the map.  The sums are made on the device, LMAX traces per call."""
    r = BodyReadout.record(body, "network.maps")
    F = r.body_rec_count()
    if F < 1:
        raise RuntimeError("network.maps: no frame recorded")
    q = quantise(traces)
    if q.shape[1] != F:
        raise ValueError("network.maps: traces of %d frames for a record of %d" % (q.shape[1], F))
    m = body.tri_of_pixel >= 0
    rho = np.empty((q.shape[0],) + m.shape, np.float64)
    w = r.body_rec_trace_maps(np.zeros((F, 1), np.int32), want=("w1", "w2"))
    for k0 in range(0, q.shape[0], LMAX):
        qk = q[k0:k0 + LMAX]
        c = r.body_rec_trace_maps(np.ascontiguousarray(qk.T), want=("c",))["c"]
        rho[k0:k0 + LMAX] = rho_from_sums(c, w["w1"], w["w2"], qk, m)
    return rho


def _pearson_rows(a, B):
    """Pearson's r of the row a (n,) with every row of B (J, n): each centred on sum / n, then
    sum(a b) / sqrt(sum(a a) sum(b b)); NaN where either is constant."""
    n = a.shape[0]
    out = np.full(B.shape[0], np.nan)
    if n < 1:
        return out
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):       # (a value that is not finite: NaN)
        ac = a - a.sum() / np.float64(n)
        Bc = B - (B.sum(1) / np.float64(n))[:, None]
        saa, sbb, sab = (ac * ac).sum(), (Bc * Bc).sum(1), (ac[None, :] * Bc).sum(1)
        ok = (sbb > 0.0) & (saa > 0.0) & ~(a == a[0]).all() & ~(B == B[:, :1]).all(1)
        out[ok] = (sab / np.sqrt(saa * sbb))[ok]
    return out


def coactivity(traces, max_lag=0):
    """Traces (K, F) -> r (K, K, 2 max_lag + 1) float64: r[i, j, max_lag + l] is Pearson's r of x_i[:F - l] with
    x_j[l:] for l >= 0 (cell j follows cell i by l frames), and r[i, j, max_lag - l] = r[j, i, max_lag + l].  NaN where a
    piece is constant (or empty: max_lag >= F)."""
    x = np.ascontiguousarray(traces, np.float64)
    if x.ndim != 2:
        raise ValueError("network: traces of shape %r (need cells x frames)" % (x.shape,))
    max_lag = int(max_lag)
    if max_lag < 0:
        raise ValueError("network: max_lag %d is negative" % max_lag)
    K, F = x.shape
    r = np.full((K, K, 2 * max_lag + 1), np.nan)
    for l in range(min(max_lag, F - 1) + 1):
        A, B = np.ascontiguousarray(x[:, :F - l]), np.ascontiguousarray(x[:, l:])
        for i in range(K):
            r[i, :, max_lag + l] = _pearson_rows(A[i], B)
        r[:, :, max_lag - l] = r[:, :, max_lag + l].T
    return r


def ensembles(r0, thr=None, p=None, alpha=0.05):
    """The lag-0 correlations (K, K) -> a label per cell (K,) int32: the connected components of the graph with an edge
    where r0[i, j] >= thr or r0[j, i] >= thr, i != j, numbered by decreasing size, then by lowest member; a cell alone
    gets -1.  NaN is no edge.  thr None: DEFAULT_THR.  With p (K, K), the p-values of coactivity_null, an edge also needs
    p[i, j] <= alpha or p[j, i] <= alpha."""
    thr = DEFAULT_THR if thr is None else float(thr)
    r0 = np.asarray(r0, np.float64)
    K = r0.shape[0]
    with np.errstate(invalid="ignore"):
        adj = r0 >= thr
    adj = (adj | adj.T) & ~np.eye(K, dtype=bool)
    if p is not None:
        with np.errstate(invalid="ignore"):
            low = np.asarray(p, np.float64) <= float(alpha)
        adj &= low | low.T
    comp = np.full(K, -1, np.int64)
    groups = []
    for i in range(K):
        if comp[i] >= 0:
            continue
        reach = np.zeros(K, bool)
        reach[i] = True
        while True:                                   # (grow by the neighbours until nothing is added)
            nxt = reach | adj[reach].any(0)
            if (nxt == reach).all():
                break
            reach = nxt
        comp[reach] = len(groups)
        groups.append(np.flatnonzero(reach))
    big = sorted((g for g in groups if len(g) > 1), key=lambda g: (-len(g), g[0]))
    labels = np.full(K, -1, np.int32)
    for e, g in enumerate(big):
        labels[g] = e
    return labels


def ensemble_traces(traces, labels):
    """-> (E, F) float64: the mean dF/F of every ensemble's members, added in ascending index, then one division."""
    x = np.asarray(traces, np.float64)
    labels = np.asarray(labels)
    E = int(labels.max()) + 1 if labels.size else 0
    out = np.zeros((max(E, 0), x.shape[1]))
    for e in range(E):
        members = np.flatnonzero(labels == e)
        for i in members:
            out[e] = out[e] + x[i]
        out[e] = out[e] / np.float64(len(members))
    return out


def lead_lag(ens, max_lag):
    """Ensemble traces (E, F) -> (lag (E, E) int32, r (E, E) float64): per ordered pair (a, b) the lag l in
    -max_lag..max_lag with the largest r of coactivity(ens, max_lag)[a, b] (b follows a by l frames) and that r.  Ties go
    to the smaller |lag|, then to the positive lag; NaN never wins (all NaN: lag 0, r NaN)."""
    max_lag = int(max_lag)
    r = coactivity(ens, max_lag)
    E = r.shape[0]
    lags = np.arange(-max_lag, max_lag + 1)
    order = sorted(range(len(lags)), key=lambda i: (abs(int(lags[i])), -int(lags[i])))       # the ties' order
    lag, peak = np.zeros((E, E), np.int32), np.full((E, E), np.nan)
    for a in range(E):
        for b in range(E):
            for i in order:
                v = r[a, b, i]
                if not np.isnan(v) and (np.isnan(peak[a, b]) or v > peak[a, b]):
                    lag[a, b], peak[a, b] = lags[i], v
    return lag, peak


def ensemble_map(rho_ens, thr):
    """The ensembles' maps (E, H, W) -> (H, W) int16: per pixel the ensemble with the largest rho if that is >= thr, else
    -1.  Ties go to the lower index; NaN counts as below (outside the map: -1)."""
    rho = np.asarray(rho_ens, np.float64)
    if rho.ndim != 3 or rho.shape[0] > 32767:
        raise ValueError("network: maps of shape %r (need ensembles x H x W, at most 32767 of them)" % (rho.shape,))
    if rho.shape[0] == 0:
        return np.full(rho.shape[1:], -1, np.int16)
    x = np.where(np.isnan(rho), -np.inf, rho)
    best = x.argmax(0)                                # (the first of equal values)
    top = np.take_along_axis(x, best[None], 0)[0]
    return np.where(top >= float(thr), best, -1).astype(np.int16)


def strain_coupling(ens, J):
    """Ensemble traces (E, F) and the area ratio of every triangle (F, T) (strain.triangles: J) -> (E, T) float64:
    Pearson's r between each ensemble trace and each triangle's area ratio; NaN for a triangle with a NaN frame or a
    constant one, and for a constant trace."""
    x = np.ascontiguousarray(ens, np.float64)
    Jt = np.ascontiguousarray(np.asarray(J, np.float64).T)
    if x.ndim != 2 or Jt.ndim != 2 or x.shape[1] != Jt.shape[1]:
        raise ValueError("network: traces %r and area ratios %r (need E x F and F x T)" % (x.shape, np.shape(J)))
    out = np.full((x.shape[0], Jt.shape[0]), np.nan)
    ok = np.isfinite(Jt).all(1)
    for e in range(x.shape[0]):
        if np.isfinite(x[e]).all():
            out[e, ok] = _pearson_rows(x[e], Jt[ok])
    return out


def colour_map(ensemble_map, gray, path=None):
    """(H, W) ensemble per pixel (-1: none) over a gray image (H, W) uint8 -> (H, W, 3) uint8 B G R: the gray value where
    there is none, else (gray + colour + 1) >> 1 with ensemble e in cellview.palette's colour e.  With `path` the image is
    also written as PNG (videoio.write_png)."""
    em = np.asarray(ensemble_map)
    g = np.asarray(gray)
    if g.dtype != np.uint8 or g.shape != em.shape or em.ndim != 2:
        raise ValueError("network: a map of shape %r over a %s image of shape %r (need uint8, the same shape)" %
                         (em.shape, g.dtype, g.shape))
    out = np.repeat(g[:, :, None], 3, axis=2)
    on = em >= 0
    if on.any():
        pal = cellview.palette(int(em.max()) + 1).astype(np.uint16)
        out[on] = ((g[on].astype(np.uint16)[:, None] + pal[em[on]] + 1) >> 1).astype(np.uint8)
    if path is not None:
        videoio.write_png(path, out)
    return out


def shifts(F, n, guard, seed=0):
    """The circular shifts a null is made of -> sorted int64: the candidates are s in 1..F-1 with min(s, F - s) > guard
    (a shift nearer to 0 leaves the surrogate correlated with the trace itself through its autocorrelation); all of them
    if there are no more than n, else n drawn without replacement by np.random.default_rng(seed).choice and sorted.
    Fewer than MIN_SHIFTS candidates raises: p = 0.05 cannot be reached."""
    F, n, guard = int(F), int(n), int(guard)
    cand = np.array([s for s in range(1, F) if min(s, F - s) > guard], np.int64)
    if len(cand) < MIN_SHIFTS:
        raise ValueError("network: %d circular shifts of %d frames beyond a guard of %d (need at least %d)" %
                         (len(cand), F, guard, MIN_SHIFTS))
    if len(cand) <= n:
        return cand
    return np.sort(np.random.default_rng(seed).choice(cand, size=n, replace=False))


def surrogates(q_row, shifts):
    """A quantised trace (F,) and S shifts -> (F, 1 + S) int32 as the device takes it: column 0 the trace, column j
    np.roll(trace, shifts[j - 1])."""
    q = np.asarray(q_row, np.int32).reshape(-1)
    out = np.empty((q.shape[0], 1 + len(shifts)), np.int32)
    out[:, 0] = q
    for j, s in enumerate(shifts):
        out[:, 1 + j] = np.roll(q, int(s))
    return out


def p_from_null(null, obs):
    """(1 + #{s: null[s] >= obs}) / (S + 1) for every value of obs, float64: the count is of whole numbers, then one
    division.  NaN where obs is NaN."""
    null = np.sort(np.asarray(null, np.float64).reshape(-1))
    obs = np.asarray(obs, np.float64)
    S = null.shape[0]
    count = S - np.searchsorted(null, np.where(np.isnan(obs), 0.0, obs), side="left")
    return np.where(np.isnan(obs), np.nan, (1 + count).astype(np.float64) / np.float64(S + 1))


def map_null(body, traces, n=1000, guard=DEFAULT_LAG, seed=0, alpha=0.05, rho=None):
    """The significance of maps(body, traces) against circularly shifted traces -> dict:
      rho (K, H, W)                 maps(body, traces)
      shifts (S,) int64             shifts(F, n, guard, seed), the same for every trace
      rho_max, rho_min (K, S)       per surrogate the largest and smallest rho over all pixels of the map
      p_map (K, H, W) float64       (1 + #{s: rho_max[s] >= rho(p)}) / (S + 1): the family-wise p-value of a pixel, the
                                    maximum over the whole map being the statistic; NaN outside the map
      p_pix (K, H, W) float64       (1 + #{s: num_s(p) >= num_0(p)}) / (S + 1): the pixel against its own surrogates alone
                                    (uncorrected; whole numbers compared); NaN outside the map
      sig (K, H, W) bool            p_map <= alpha
    Per trace one call of the device (hm_body_rec_trace_null): F x (S + 1) whole numbers go in, two planes of counts and
    2 (S + 1) doubles come out.  The observed column's maximum must be the largest rho of `maps`, bit for bit.  `rho`: what
    maps(body, traces) gave, for a caller that has it already."""
    BodyReadout.record(body, "network.map_null")
    rho = maps(body, traces) if rho is None else np.asarray(rho, np.float64)
    q = quantise(traces)
    K, F = q.shape
    sh = shifts(F, n, guard, seed)
    S = len(sh)
    if S + 1 > NULL_LMAX:
        raise ValueError("network.map_null: %d surrogates (at most %d a call)" % (S, NULL_LMAX - 1))
    m = body.tri_of_pixel >= 0
    out = dict(rho=rho, shifts=sh, rho_max=np.empty((K, S)), rho_min=np.empty((K, S)), p_map=np.empty(rho.shape),
               p_pix=np.empty(rho.shape), sig=np.empty(rho.shape, bool))
    for k in range(K):
        qs = [int(v) for v in q[k]]
        vb = float(F * sum(v * v for v in qs) - sum(qs) ** 2)          # (a roll keeps both sums: every column's)
        o = body.r.body_rec_trace_null(surrogates(q[k], sh), np.full(S + 1, vb))
        assert o["tmax"][0] == np.nanmax(rho[k]) and o["tmin"][0] == np.nanmin(rho[k])
        out["rho_max"][k], out["rho_min"][k] = o["tmax"][1:], o["tmin"][1:]
        out["p_map"][k] = p_from_null(o["tmax"][1:], rho[k])
        out["p_pix"][k] = np.where(m, (1 + o["ge"].astype(np.int64)).astype(np.float64) / np.float64(S + 1), np.nan)
        with np.errstate(invalid="ignore"):
            out["sig"][k] = out["p_map"][k] <= float(alpha)
    return out


def coactivity_null(traces, shifts):
    """Traces (K, F) and S circular shifts -> p_r (K, K) float64: for every ordered pair i != j the observed
    F sum(q_i q_j) - u1_i u1_j of the quantised traces (int64, exact: F below 92682) against the same with q_j rolled by
    every shift: (1 + #{s: surrogate >= observed}) / (S + 1).  NaN on the diagonal and for a trace with a value that is
    not finite."""
    x = np.asarray(traces, np.float64)
    if x.ndim != 2:
        raise ValueError("network: traces of shape %r (need cells x frames)" % (x.shape,))
    K, F = x.shape
    if F * F * QMAX * QMAX >= 2 ** 63:
        raise ValueError("network.coactivity_null: %d frames (F x F x 32767^2 could pass 2^63)" % F)
    ok = np.isfinite(x).all(1)
    q = np.zeros((K, F), np.int64)
    q[ok] = quantise(x[ok])
    u1 = q.sum(1)
    S = len(shifts)
    p = np.full((K, K), np.nan)
    for j in np.flatnonzero(ok):
        rolled = np.array([np.roll(q[j], int(s)) for s in shifts], np.int64).reshape(S, F)
        for i in np.flatnonzero(ok):
            if i == j:
                continue
            obs = F * (q[i] * q[j]).sum() - u1[i] * u1[j]
            sur = F * (rolled * q[i][None, :]).sum(1) - u1[i] * u1[j]
            p[i, j] = np.float64(1 + int((sur >= obs).sum())) / np.float64(S + 1)
    return p


def extract(body, traces, thr=None, max_lag=DEFAULT_LAG, map_thr=None, null=0, guard=DEFAULT_LAG, seed=0, alpha=0.05):
    """The whole readout of the traces (K, F) of the cells of a BodyReadout(keep=True) -> dict:
      r (K, K, 2 max_lag + 1) float64      coactivity; a trace with a value that is not finite correlates with nothing
      labels (K,) int32, ens_traces (E, F) ensembles(r at lag 0, thr) and their mean traces
      lead_lag (E, E) int32, lead_r (E, E)  lead_lag(ens_traces, max_lag)
      rho (E, H, W) float64                 maps(body, ens_traces)
      map (H, W) int16                      ensemble_map(rho, map_thr)
      gray (H, W) uint8                     the mean recorded frame, rint(w1 / F): what colour_map paints the map on
    thr None: DEFAULT_THR; map_thr None: DEFAULT_MAP_THR.  With null > 0 also, against `null` circular shifts
    (shifts(F, null, guard, seed)):
      p_r (K, K)                            coactivity_null of the cells' traces
      p_map (E, H, W), rho_max (E, S), sig (E, H, W) bool, shifts (S,)     map_null of the ensembles' traces at alpha
      map_sig (H, W) int16                  `map` with -1 where the winning ensemble's pixel is not significant"""
    x = np.asarray(traces, np.float64)
    max_lag = int(max_lag)
    r = coactivity(x, max_lag)
    labels = ensembles(r[:, :, max_lag], thr)
    ens = ensemble_traces(x, labels)
    lag, peak = lead_lag(ens, max_lag)
    rho = maps(body, ens)
    F = body.r.body_rec_count()
    w1 = body.r.body_rec_trace_maps(np.zeros((F, 1), np.int32), want=("w1",))["w1"]
    gray = np.rint(w1.astype(np.float64) / np.float64(F)).astype(np.uint8)
    out = dict(r=r, labels=labels, ens_traces=ens, lead_lag=lag, lead_r=peak, rho=rho,
               map=ensemble_map(rho, DEFAULT_MAP_THR if map_thr is None else map_thr), gray=gray)
    if null > 0:
        sh = shifts(F, null, guard, seed)
        out.update(p_r=coactivity_null(x, sh), shifts=sh)
        if len(ens):
            mn = map_null(body, ens, null, guard, seed, alpha, rho=rho)
            out.update(p_map=mn["p_map"], rho_max=mn["rho_max"], sig=mn["sig"])
        else:
            out.update(p_map=np.empty(rho.shape), rho_max=np.empty((0, len(sh))), sig=np.empty(rho.shape, bool))
        won = np.take_along_axis(out["sig"], np.maximum(out["map"], 0).astype(np.int64)[None], 0)[0] if len(ens) else False
        out["map_sig"] = np.where((out["map"] >= 0) & won, out["map"], -1).astype(np.int16)
    return out
