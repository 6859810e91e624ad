"""Activity waves: where on the animal an event starts and how it travels, from the kept registered video.

Around every trigger frame (the onsets of an ensemble's trace) each map pixel's binned plane is followed from a baseline
window to its maximum; the latency is the sub-frame time at which it crosses half of that rise, in 1/256 frame relative to
the trigger.  The device works all of it out in exact integers (hm_body_rec_waves: the rule is stated word for word in
include/hydra_mi.h and DESIGN.md section 27; csrc/waves_kernels.h; tests/waves_ref.py restates it in NumPy and Python
integers): the latency per event and pixel, its count and sums over the events, and per event the nine sums of a plane
fit of the latency round every node of a grid.  The host turns the sums into a mean latency map, its gradient (frames
per pixel) and the velocity (pixels per frame), in binary64, one operation at a time.

    body = BodyReadout(kf, keep=True)
    for each frame: kf.compute(...); body.registered(kf.state.X, raw_frame)
    trig = waves.triggers(ens_traces, pre=8, lead=8, post=24, F=frames)      # a list: one int32 array per ensemble
    w = waves.latency(body, trig[0])                       # lat_mean, lat_sd, cnt, n_bin, nodes, fit
    g, v = waves.velocity(w["fit"], n_min=20)              # per event and node
    c, r = waves.origin(w["lat_mean"], w["cnt"], min_cnt=3)
"""
import warnings

import numpy as np

from . import detrend, events, videoio
from .body import BodyReadout

DEFAULT_PRE, DEFAULT_LEAD, DEFAULT_POST = 8, 8, 24
DEFAULT_BIN = 2                    # bins of 5 x 5 pixels
DEFAULT_MIN_RISE = 8               # grey levels of the plane, per pixel of the bin
DEFAULT_STEP, DEFAULT_FIT = 8, 6   # a node every 8 pixels, fitted over the pixels within 6
DEFAULT_REFRACTORY = 16            # frames between two onsets of a trace
LAT_NONE = np.iinfo(np.int32).min  # the latency where there is none (why >= 2)
B_MAX, PRE_MAX, LEAD_MAX, POST_MAX, E_MAX, STEP_MAX, RF_MAX = 8, 64, 64, 256, 65536, 64, 16
WHY = {0: "valid", 1: "valid, still rising at the window's end", 2: "rise too small", 3: "at half height when the search starts",
       255: "off the map"}


def _check(who, b, pre, lead, post, min_rise, step, Rf):
    for name, v, lo, hi in (("b", b, 0, B_MAX), ("pre", pre, 1, PRE_MAX), ("lead", lead, 0, LEAD_MAX), ("post", post, 1, POST_MAX),
                            ("min_rise", min_rise, 1, 255), ("step", step, 1, STEP_MAX), ("Rf", Rf, 1, RF_MAX)):
        if not lo <= int(v) <= hi:
            raise ValueError("%s: %s %r outside %d..%d" % (who, name, v, lo, hi))


def admissible(t, pre, lead, post, F):
    """bool per trigger frame: its baseline and search windows lie inside a record of F frames"""
    t = np.asarray(t, np.int64)
    return (t - int(lead) - int(pre) >= 0) & (t + int(post) <= int(F) - 1)


def onsets(binary, refractory):
    """A row of bool per frame -> int32: the first frame of every run of events that lies at least `refractory` frames
    after the onset kept before it."""
    ev = np.asarray(binary, bool).reshape(-1)
    first = np.flatnonzero(ev & ~np.concatenate(([False], ev[:-1])))
    out, last = [], None
    for k in first:
        if last is None or k - last >= int(refractory):
            out.append(int(k))
            last = int(k)
    return np.array(out, np.int32)


def triggers(ens_traces, g=None, lam=None, s_min=None, refractory=DEFAULT_REFRACTORY, pre=DEFAULT_PRE, lead=DEFAULT_LEAD,
             post=DEFAULT_POST, F=None):
    """The onsets of every trace (E, F) -> a list of int32 arrays, one per trace.  A trace is deconvolved as hydra_mi.events
    does it (g None: estimate_g; lam None: default_lam(g, noise); s_min None: default_smin(noise); each a scalar or one
    per trace), binarised, and the first frame of every run of events at least `refractory` frames after the previous onset
    is kept (onsets).  Onsets whose windows t - lead - pre .. t + post leave the record of F frames (None: the traces'
    length) are dropped."""
    x = np.asarray(ens_traces, np.float64)
    x = x[None] if x.ndim == 1 else x
    if x.ndim != 2:
        raise ValueError("waves.triggers: traces of shape %r (need (E, F))" % (x.shape,))
    if int(refractory) < 1:
        raise ValueError("waves.triggers: refractory %r (need >= 1)" % (refractory,))
    F = x.shape[1] if F is None else int(F)
    per = lambda v, i: None if v is None else float(np.broadcast_to(np.asarray(v, np.float64), x.shape[:1])[i])
    out = []
    for i, y in enumerate(x):
        if not np.isfinite(y).all():
            out.append(np.zeros(0, np.int32))
            continue
        sigma = events.noise(y)
        gi = events.estimate_g(y) if g is None else per(g, i)
        li = events.default_lam(gi, sigma) if lam is None else per(lam, i)
        si = events.default_smin(sigma) if s_min is None else per(s_min, i)
        _, s = events.deconvolve(y, gi, li)
        t = onsets(events.binarise(s, si), refractory)
        out.append(t[admissible(t, pre, lead, post, F)].astype(np.int32))
    return out


def node_grid(r, step):
    """The fit's nodes on the renderer r's record -> ((N, 2) int32: column and row in the frame, row-major; (ny, nx))"""
    nx, ny, c0, r0 = r.body_rec_wave_nodes(step)
    jj, ii = np.divmod(np.arange(nx * ny), nx)
    return np.stack((c0 + ii * int(step), r0 + jj * int(step)), 1).astype(np.int32), (ny, nx)


def latency(body, trig, what="dff", half=detrend.DEFAULT_HALF, q=detrend.DEFAULT_Q, floor=detrend.DEFAULT_FLOOR,
            gain=detrend.DEFAULT_GAIN, b=DEFAULT_BIN, pre=DEFAULT_PRE, lead=DEFAULT_LEAD, post=DEFAULT_POST, min_rise=DEFAULT_MIN_RISE,
            step=DEFAULT_STEP, Rf=DEFAULT_FIT, keep=False):
    """The latency maps of the events at the trigger frames `trig` (int32) of a BodyReadout(keep=True) -> dict:
      lat_mean (H, W) float32   frames after the trigger: (sum_lat / cnt) / 256 in binary64, then rounded; NaN where cnt is 0
      lat_sd (H, W) float32     sqrt(max(sum_lat2 / cnt - (sum_lat / cnt)^2, 0)) / 256, likewise
      cnt (H, W) uint32         the events in which the pixel is valid;  n_bin (H, W) uint16: the map pixels of its bin
      nodes (N, 2) int32        column and row of the fit's nodes, row-major;  nodes_shape (ny, nx)
      fit (E, N, 9) int64       the nine sums of hm_body_rec_waves per event and node (velocity reads them)
    and with `keep` the planes per event: lat, rise (E, H, W) int32, why (E, H, W) uint8.  No trigger: no call; cnt and n_bin 0."""
    detrend._check("waves.latency", what, half, q, floor, gain)
    _check("waves.latency", b, pre, lead, post, min_rise, step, Rf)
    r = BodyReadout.record(body, "waves.latency")
    t = np.ascontiguousarray(trig, np.int32).reshape(-1)
    nodes, (ny, nx) = node_grid(r, step)
    H, W = r.ny, r.nx
    if t.size == 0:
        o = dict(n_bin=np.zeros((H, W), np.uint16), cnt=np.zeros((H, W), np.uint32), sum_lat=np.zeros((H, W), np.int64), sum_lat2=np.zeros((H, W), np.int64),
                 fit=np.zeros((0, nx * ny, 9), np.int64), lat=np.zeros((0, H, W), np.int32), rise=np.zeros((0, H, W), np.int32),
                 why=np.zeros((0, H, W), np.uint8))
    else:
        want = r.WAVE_OUTPUTS if keep else ("n_bin", "cnt", "sum_lat", "sum_lat2", "fit")
        o = r.body_rec_waves(t, what, half, q, floor, gain, b, pre, lead, post, min_rise, step, Rf, want=want)
    mean, sd = mean_sd(o["cnt"], o["sum_lat"], o["sum_lat2"])
    out = dict(lat_mean=mean, lat_sd=sd, cnt=o["cnt"], n_bin=o["n_bin"], nodes=nodes, nodes_shape=(ny, nx), fit=o["fit"])
    if keep:
        out.update(lat=o["lat"], rise=o["rise"], why=o["why"])
    return out


def mean_sd(cnt, sum_lat, sum_lat2):
    """The sums of hm_body_rec_waves -> (lat_mean, lat_sd) float32 in frames, NaN where cnt is 0.  In binary64:
    m = sum_lat / cnt; lat_mean = m / 256; v = sum_lat2 / cnt - m m; lat_sd = sqrt(max(v, 0)) / 256."""
    c = np.asarray(cnt).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.asarray(sum_lat).astype(np.float64) / c
        v = np.asarray(sum_lat2).astype(np.float64) / c - m * m
        mean, sd = m / 256.0, np.sqrt(np.maximum(v, 0.0)) / 256.0
    none = np.asarray(cnt) == 0
    return np.where(none, np.nan, mean).astype(np.float32), np.where(none, np.nan, sd).astype(np.float32)


def _solve(n, a11, a12, a22, b1, b2, ok, scale):
    """The closed 2 x 2 form of velocity, from float64 arrays of A's and bvec's entries"""
    with np.errstate(divide="ignore", invalid="ignore"):
        det = a11 * a22 - a12 * a12
        gx = ((a22 * b1 - a12 * b2) / det) / scale
        gy = ((a11 * b2 - a12 * b1) / det) / scale
        s = gx * gx + gy * gy
        vx, vy = gx / s, gy / s
    bad = ~(ok & (det > 0.0) & (s > 0.0))
    g, v = np.stack((gx, gy), -1), np.stack((vx, vy), -1)
    g[bad] = np.nan
    v[bad] = np.nan
    return g, v


def velocity(fit, n_min):
    """The nine sums (..., 9) int64 of hm_body_rec_waves (n, Sx, Sy, Sxx, Sxy, Syy, SL, SxL, SyL over the valid pixels round a
    node, L in 1/256 frame) -> (g (..., 2) float64 frames per pixel, v (..., 2) float64 pixels per frame), (x, y) each.
    In int64 (every product stays below 2^41):
      a11 = n Sxx - Sx Sx; a12 = n Sxy - Sx Sy; a22 = n Syy - Sy Sy; b1 = n SxL - Sx SL; b2 = n SyL - Sy SL.
    Then converted to binary64 (all exact), one operation at a time in this order:
      det = a11 a22 - a12 a12;
      gx = ((a22 b1 - a12 b2) / det) / 256; gy = ((a11 b2 - a12 b1) / det) / 256;
      s = gx gx + gy gy; vx = gx / s; vy = gy / s.
    NaN where n < n_min, det <= 0 (fewer than three valid pixels off one line) or s == 0 (a flat latency: no direction)."""
    f = np.asarray(fit)
    if f.dtype != np.int64 or f.shape[-1:] != (9,):
        raise ValueError("waves.velocity: sums of %s and shape %r (need int64, (..., 9))" % (f.dtype, f.shape))
    n, sx, sy, sxx, sxy, syy, sl, sxl, syl = (f[..., i] for i in range(9))
    a11, a12, a22 = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    b1, b2 = n * sxl - sx * sl, n * syl - sy * sl
    as64 = lambda a: a.astype(np.float64)
    return _solve(n, as64(a11), as64(a12), as64(a22), as64(b1), as64(b2), n >= int(n_min), 256.0)


def mean_fit(lat_mean, cnt, nodes, Rf, min_cnt):
    """The nine sums of the fit on the mean map -> (N, 9) float64: as hm_body_rec_waves forms them per event, with
    lat_mean (frames) as the latency and a pixel valid where cnt >= min_cnt; in binary64, the window's pixels added row by
    row."""
    lm, c = np.asarray(lat_mean, np.float64), np.asarray(cnt)
    nodes = np.asarray(nodes, np.int64).reshape(-1, 2)
    H, W = lm.shape
    valid = (c >= int(min_cnt)) & np.isfinite(lm)
    out = np.zeros((len(nodes), 9), np.float64)
    for dy in range(-int(Rf), int(Rf) + 1):
        for dx in range(-int(Rf), int(Rf) + 1):
            x, y = nodes[:, 0] + dx, nodes[:, 1] + dy
            on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            on[on] = valid[y[on], x[on]]
            L = np.where(on, lm[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)
            geo = np.array([1.0, dx, dy, dx * dx, dx * dy, dy * dy], np.float64)
            out[:, :6] += on[:, None] * geo[None]
            out[:, 6:] += np.stack((L, dx * L, dy * L), 1)          # (L is 0 where the pixel is not valid)
    return out


def mean_velocity(lat_mean, cnt, nodes, Rf, min_cnt, n_min=3):
    """velocity's fit on the mean latency map: the same nodes and windows, a pixel valid where cnt >= min_cnt -> (g, v) as
    velocity gives them ((N, 2) float64 each), from mean_fit's sums, all in binary64."""
    f = mean_fit(lat_mean, cnt, nodes, Rf, min_cnt)
    n, sx, sy, sxx, sxy, syy, sl, sxl, syl = (f[:, i] for i in range(9))
    return _solve(n, n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy, n * sxl - sx * sl, n * syl - sy * sl,
                  n >= int(n_min), 1.0)


def origin(lat_mean, cnt, min_cnt):
    """Where the wave starts: (column, row) of the pixel of least mean latency among those with cnt >= min_cnt (and at
    least 1); ties go to the lower raster index.  None if there is no such pixel."""
    lm, c = np.asarray(lat_mean, np.float64), np.asarray(cnt)
    ok = (c >= max(int(min_cnt), 1)) & np.isfinite(lm)
    if not ok.any():
        return None
    i = int(np.argmin(np.where(ok, lm, np.inf)))          # (the first of equal values)
    return i % lm.shape[1], i // lm.shape[1]


def lut():
    """256 colours B G R from early (blue) through green to late (red)"""
    i = np.arange(256)
    return np.stack((255 - i, 255 - np.abs(2 * i - 255), i), 1).astype(np.uint8)


def colour_map(lat_mean, gray, path=None):
    """(H, W) mean latency (NaN: none) over a gray image (H, W) uint8 -> (H, W, 3) uint8 B G R: the gray value where there
    is none, else (gray + colour + 1) >> 1 with the colour lut()[floor(255 (v - lo) / (hi - lo))] between the least and the
    largest latency of the map (one latency alone: entry 0).  With `path` the image is also written as PNG
    (videoio.write_png), as network.colour_map writes its own."""
    lm, g = np.asarray(lat_mean, np.float64), np.asarray(gray)
    if g.dtype != np.uint8 or g.shape != lm.shape or lm.ndim != 2:
        raise ValueError("waves: a map of shape %r over a %s image of shape %r (need uint8, the same shape)" % (lm.shape, g.dtype, g.shape))
    out = np.repeat(g[:, :, None], 3, axis=2)
    on = np.isfinite(lm)
    if on.any():
        lo, hi = lm[on].min(), lm[on].max()
        idx = np.floor(255.0 * (lm[on] - lo) / (hi - lo)).astype(np.int64) if hi > lo else np.zeros(int(on.sum()), np.int64)
        out[on] = ((g[on].astype(np.uint16)[:, None] + lut()[idx].astype(np.uint16) + 1) >> 1).astype(np.uint8)
    if path is not None:
        videoio.write_png(path, out)
    return out


def extract(body, ens_traces=None, trig=None, n_min=None, min_cnt=1, refractory=DEFAULT_REFRACTORY, **params):
    """The whole readout, one hm_body_rec_waves call per ensemble.  `trig`: a list of trigger arrays, one per ensemble; None:
    triggers(ens_traces, ...) over the record's frames.  params: latency's (what .. Rf, keep).  -> dict:
      triggers (sum E,) int32, trigger_ens (sum E,) int32     every trigger used and its ensemble
      lat_mean, lat_sd (K, H, W) float32, count (K, H, W) uint32, n_bin (H, W) uint16
      nodes (N, 2) int32, velocity (K, N, 2) float32           per node the median over the events of velocity(fit, n_min)
      speed (K,) float64                                       the median |velocity| over the nodes where it is finite (NaN: none)
      origin (K, 2) int32                                      origin(lat_mean, count, min_cnt), (-1, -1) where there is none
      valid (K,) float64                                       the share of (event, map pixel) that is valid
      gray (H, W) uint8                                        the mean recorded frame, as network.extract forms it
    and with keep=True lat, rise (sum E, H, W) int32, why (sum E, H, W) uint8, fit (sum E, N, 9) int64.  n_min None: a
    quarter of the fit window's pixels."""
    r = BodyReadout.record(body, "waves.extract")
    F = r.body_rec_count()
    win = {k: params.get(k, d) for k, d in (("pre", DEFAULT_PRE), ("lead", DEFAULT_LEAD), ("post", DEFAULT_POST))}
    if trig is None:
        trig = triggers(ens_traces, refractory=refractory, F=F, **win)
    trig = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in trig]
    keep = bool(params.get("keep", False))
    Rf = int(params.get("Rf", DEFAULT_FIT))
    n_min = (2 * Rf + 1) ** 2 // 4 if n_min is None else int(n_min)
    H, W, K = r.ny, r.nx, len(trig)
    kept = {k: [] for k in ("lat", "rise", "why", "fit")}
    nodes = node_grid(r, int(params.get("step", DEFAULT_STEP)))[0]
    out = dict(triggers=np.concatenate(trig + [np.zeros(0, np.int32)]).astype(np.int32),
               trigger_ens=np.concatenate([np.full(len(t), k, np.int32) for k, t in enumerate(trig)] + [np.zeros(0, np.int32)]),
               lat_mean=np.full((K, H, W), np.nan, np.float32), lat_sd=np.full((K, H, W), np.nan, np.float32),
               count=np.zeros((K, H, W), np.uint32), speed=np.full(K, np.nan), origin=np.full((K, 2), -1, np.int32),
               valid=np.zeros(K), n_bin=np.zeros((H, W), np.uint16), nodes=nodes, velocity=np.full((K, len(nodes), 2), np.nan, np.float32))
    for k, t in enumerate(trig):
        w = latency(body, t, **params)
        out["lat_mean"][k], out["lat_sd"][k], out["count"][k] = w["lat_mean"], w["lat_sd"], w["cnt"]
        if len(t):
            out["n_bin"] = w["n_bin"]                 # (the same for every ensemble that has a trigger; 0 without one)
            _, v = velocity(w["fit"], n_min)
            with warnings.catch_warnings():          # (a node that is NaN in every event stays NaN, without a word)
                warnings.simplefilter("ignore", RuntimeWarning)
                vm = np.nanmedian(v, axis=0)
            out["velocity"][k] = vm
            sp = np.sqrt(vm[:, 0] * vm[:, 0] + vm[:, 1] * vm[:, 1])
            if np.isfinite(sp).any():
                out["speed"][k] = float(np.median(sp[np.isfinite(sp)]))
            on_map = int((w["n_bin"] > 0).sum())
            out["valid"][k] = float(w["cnt"].sum()) / float(max(1, on_map * len(t)))
        o = origin(w["lat_mean"], w["cnt"], min_cnt)
        if o is not None:
            out["origin"][k] = o
        if keep:
            for key in kept:
                kept[key].append(w[key])
    if keep:
        N = len(nodes)
        empty = dict(lat=np.zeros((0, H, W), np.int32), rise=np.zeros((0, H, W), np.int32), why=np.zeros((0, H, W), np.uint8),
                     fit=np.zeros((0, N, 9), np.int64))
        out.update({key: np.concatenate(kept[key] + [empty[key]]) for key in kept})
    w1 = r.body_rec_trace_maps(np.zeros((F, 1), np.int32), want=("w1",))["w1"]
    out["gray"] = np.rint(w1.astype(np.float64) / np.float64(F)).astype(np.uint8)
    return out
