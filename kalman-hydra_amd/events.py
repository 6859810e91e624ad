"""Events from calcium traces: AR(1) deconvolution of cell traces on the host and of every pixel of the kept registered
video on the device.

An indicator's decay smears one event over several frames; that inflates every correlation between traces.  Here a trace
y is explained as c_k = g c_{k-1} + s_k with s_k >= 0, minimising 1/2 sum (c_k - y_k)^2 + lam sum s_k (AR(1) OASIS:
Friedrich, Zhou, Paninski 2017) on a stack of pools.  The rule is stated word for word in include/hydra_mi.h
(hm_body_rec_event_*) and DESIGN.md section 19; tests/events_ref.py restates it in Python floats.  `deconvolve` is that
rule in binary64 for a handful of cell traces; the device runs the same rule on every box pixel of every kept frame
(csrc/events_kernels.h), and on a trace of integers 0..255 the two agree bit for bit.

    body = BodyReadout(kf, keep=True)
    for each frame: kf.compute(...); body.registered(kf.state.X, raw_frame)
    g = events.estimate_g(trace); lam = events.default_lam(g, events.noise(trace))
    c, s = events.deconvolve(traces, g, lam)                     # cells x F
    count, total = events.count_image(body, g, lam_px, s_min)    # per pixel: events, and their summed size
    points, scores = events.find_points(body, 12, g, lam_px)     # seeds of the event video
    events.event_video(body, "events.avi", g, lam_px)
"""
import numpy as np

from . import detrend
from .body import BodyReadout

G_MIN, G_MAX = 0.05, 0.98          # estimate_g keeps inside these
LAM_Z = 2.0                        # default_lam: noise of this many sigma leaves no event in a long pool
SMIN_Z = 2.0                       # default_smin: events of at least this many sigma
VIDEO_BYTES = 512 << 20            # host memory a block of event_video's planes takes at most


def powers(g, F):
    """(pw, pw2): pw[l] = g^l by repeated multiplication and pw2[l] = pw[l] pw[l], l = 0 .. F, float64"""
    pw = np.empty(int(F) + 1, np.float64)
    pw[0] = 1.0
    g = np.float64(g)
    for l in range(1, int(F) + 1):
        pw[l] = pw[l - 1] * g
    return pw, pw * pw


def _check(who, g, lam):
    if not (np.isfinite(g) and 0.0 < g < 1.0):
        raise ValueError("%s: g %r outside 0 < g < 1" % (who, g))
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError("%s: lam %r negative or not finite" % (who, lam))


def _one(y, g, lam, pw, pw2):
    F = y.shape[0]
    v, w = np.empty(F, np.float64), np.empty(F, np.float64)      # the stack: pool i in slot i
    t, l = np.empty(F, np.int64), np.empty(F, np.int64)
    mu, n = lam * (1.0 - g), 0
    for k in range(F):
        v[n], w[n], t[n], l[n] = y[k] - (lam if k == F - 1 else mu), 1.0, k, 1
        n += 1
        while n > 1 and v[n - 1] < pw[l[n - 2]] * v[n - 2]:
            a, b = n - 2, n - 1
            num = w[a] * v[a] + (pw[l[a]] * w[b]) * v[b]
            den = w[a] + pw2[l[a]] * w[b]
            v[a], w[a] = num / den, den
            l[a] += l[b]
            n -= 1
    c, s = np.zeros(F, np.float64), np.zeros(F, np.float64)
    vp = np.where(v[:n] > 0.0, v[:n], 0.0)
    for i in range(n):
        c[t[i]:t[i] + l[i]] = vp[i] * pw[:l[i]]
        if i > 0:
            x = vp[i] - g * (vp[i - 1] * pw[l[i - 1] - 1])
            s[t[i]] = x if x > 0.0 else 0.0
    return c, s


def deconvolve(y, g, lam):
    """y (F,) or (cells, F); g, lam scalars or one per cell -> (c, s) float64 of y's shape: the calcium c_k = g c_{k-1} + s_k
    and the events s >= 0 (s_0 = 0) of the rule, in binary64 in the rule's order."""
    y = np.asarray(y, np.float64)
    flat = y.reshape(-1, y.shape[-1]) if y.ndim else y.reshape(1, 1)
    if y.ndim not in (1, 2):
        raise ValueError("events.deconvolve: traces of shape %r (need (F,) or (cells, F))" % (y.shape,))
    gs, lams = np.broadcast_to(np.asarray(g, np.float64), flat.shape[:1]), np.broadcast_to(np.asarray(lam, np.float64), flat.shape[:1])
    c, s = np.empty_like(flat), np.empty_like(flat)
    for i in range(flat.shape[0]):
        _check("events.deconvolve", gs[i], lams[i])
        pw, pw2 = powers(gs[i], flat.shape[1])
        c[i], s[i] = _one(flat[i], np.float64(gs[i]), np.float64(lams[i]), pw, pw2)
    return c.reshape(y.shape), s.reshape(y.shape)


def estimate_g(trace):
    """The decay per frame from the autocovariance at lags 1 and 2: for c_k = g c_{k-1} + s_k with white s, and white noise
    on top, cov(lag 2) / cov(lag 1) = g (the noise drops out of both).  Kept inside G_MIN .. G_MAX; a trace whose lag-1
    covariance is not positive, or of fewer than 4 frames, has no decay to find and gets G_MIN."""
    x = np.asarray(trace, np.float64).reshape(-1)
    x = x - x.mean()
    if x.shape[0] < 4:
        return G_MIN
    c1, c2 = float(np.mean(x[1:] * x[:-1])), float(np.mean(x[2:] * x[:-2]))
    if not c1 > 0.0:
        return G_MIN
    return float(min(G_MAX, max(G_MIN, c2 / c1)))


def noise(trace):
    """The noise of a trace: 1.4826 x the median absolute deviation of its first differences / sqrt(2)"""
    d = np.diff(np.asarray(trace, np.float64).reshape(-1))
    if d.shape[0] < 1:
        return 0.0
    return float(1.4826 * np.median(np.abs(d - np.median(d))) / np.sqrt(2.0))


def default_lam(g, sigma):
    """The penalty at which white noise of LAM_Z sigma leaves no event: a long pool of noise alone has the value
    (noise term of standard deviation sigma sqrt(1 - g^2)) - lam (1 - g)(1 + g), so lam = LAM_Z sigma / sqrt(1 - g^2)."""
    return float(LAM_Z * sigma / np.sqrt(1.0 - g * g))


def default_smin(sigma):
    """The least event that counts: SMIN_Z sigma"""
    return float(SMIN_Z * sigma)


def binarise(s, s_min):
    """s (..., F), s_min a scalar or one per row -> bool: the frames with an event of at least s_min (and more than 0)"""
    s = np.asarray(s, np.float64)
    thr = np.asarray(s_min, np.float64)
    thr = thr[..., None] if thr.ndim == s.ndim - 1 and thr.ndim else thr
    return (s >= thr) & (s > 0.0)


# ---- every pixel of the kept record, on the device ----------------------------------------------------------------------
def _record(who, body, what, half, q, floor, gain, g, lam):
    detrend._check(who, what, half, q, floor, gain)
    _check(who, g, lam)
    return BodyReadout.record(body, who)


def stats_add(body, g, lam, what="dff", half=detrend.DEFAULT_HALF, q=detrend.DEFAULT_Q, floor=detrend.DEFAULT_FLOOR,
              gain=detrend.DEFAULT_GAIN):
    """Begin the tracker's statistics afresh and feed them the event plane of every recorded frame -> frames added"""
    r = _record("events.stats_add", body, what, half, q, floor, gain, g, lam)
    r.body_stats_begin()
    r.body_rec_event_stats_add(what, half, q, floor, gain, g, lam)
    return r.body_stats_count()


def find_points(body, n, g, lam, radius=6, score="corr", min_score=None, **planes):
    """detrend.find_points on the event video: the n best local maxima of the local correlation (or "std", "range") of
    the events instead of the light -> (points (P <= n, 2) at the pixel centres, scores (P,))"""
    stats_add(body, g, lam, **planes)
    idx, sc, _ = body.r.body_stats_peaks(score, radius, -np.inf if min_score is None else float(min_score), int(n))
    return BodyReadout.pixel_points(body, idx), sc


def count_image(body, g, lam, s_min, what="dff", half=detrend.DEFAULT_HALF, q=detrend.DEFAULT_Q, floor=detrend.DEFAULT_FLOOR,
                gain=detrend.DEFAULT_GAIN):
    """(count (H, W) uint32, total (H, W) float64): per pixel the frames with an event of at least s_min, and the sum of
    its events over the record.  Cells that fire rarely but sharply stand out in the first."""
    r = _record("events.count_image", body, what, half, q, floor, gain, g, lam)
    if not (np.isfinite(s_min) and s_min >= 0.0):
        raise ValueError("events.count_image: s_min %r negative or not finite" % (s_min,))
    return r.body_rec_event_sums(what, half, q, floor, gain, g, lam, s_min)


def event_video(body, path, g, lam, what="dff", half=detrend.DEFAULT_HALF, q=detrend.DEFAULT_Q, floor=detrend.DEFAULT_FLOOR,
                gain=detrend.DEFAULT_GAIN, block=None, video_opts=None):
    """The event bytes of every recorded frame as a grey AVI (B = G = R; video_opts: AviWriter's codec options, an MJPEG
    video codes one component) in the body frame -> frames written.  Through the
    writer of detrend.write_video, `block` frames at a time (default: VIDEO_BYTES worth).  Every block is cut from the
    solution of the whole record, which the device works out again for it: the event planes do not stay there between
    calls, so the blocks are larger than detrend.write_video's."""
    r = _record("events.event_video", body, what, half, q, floor, gain, g, lam)
    return detrend.write_planes(body, path, lambda k0, n: r.body_rec_event_planes(what, half, q, floor, gain, g, lam, k0, n),
                                VIDEO_BYTES, block, video_opts)[0]
