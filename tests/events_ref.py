"""Restatement of the events per pixel of the kept registered video (include/hydra_mi.h: hm_body_rec_event_planes /
_stats_add / _sums; hydra_mi.events) in loops over Python floats and lists -- binary64, one operation at a time, in the
order of the rule -- and the planted video with known event frames that detection is measured on.  Shares no code with
hydra_mi/events.py."""
import math

import numpy as np

import roi_ref


def pos(a):
    """a where a > 0, else +0"""
    return a if a > 0.0 else 0.0


def powers(g, F):
    """pw[l] = g^l by repeated multiplication, and pw2[l] = pw[l] pw[l], l = 0 .. F"""
    pw = [1.0]
    for _ in range(F):
        pw.append(pw[-1] * g)
    return pw, [x * x for x in pw]


def pools(y, g, lam):
    """The pool stack [v, w, t, l] of the sequence y after its last frame"""
    F = len(y)
    pw, pw2 = powers(g, F)
    st = []
    for k in range(F):
        yk = float(y[k])
        st.append([yk - lam if k == F - 1 else yk - lam * (1.0 - g), 1.0, k, 1])
        while len(st) > 1:
            a, b = st[-2], st[-1]
            if not b[0] < pw[a[3]] * a[0]:
                break
            num = a[1] * a[0] + (pw[a[3]] * b[1]) * b[0]
            den = a[1] + pw2[a[3]] * b[1]
            a[0] = num / den
            a[1] = den
            a[3] += b[3]
            st.pop()
    return st, pw


def deconvolve(y, g, lam):
    """(c, s): lists of F floats"""
    F = len(y)
    st, pw = pools(y, g, lam)
    c, s = [0.0] * F, [0.0] * F
    for i, (v, _, t, l) in enumerate(st):
        for j in range(l):
            c[t + j] = pos(v) * pw[j]
        if i > 0:
            vp, lp = st[i - 1][0], st[i - 1][3]
            s[t] = pos(pos(v) - g * (pos(vp) * pw[lp - 1]))
    return c, s


def pixel(y, g, lam, s_min):
    """(E bytes (F), n, S) of one pixel's sequence"""
    s = deconvolve(y, g, lam)[1]
    E = [min(255, int(math.floor(x + 0.5))) for x in s]
    n = sum(1 for x in s if x >= s_min)
    S = 0.0
    for x in s:
        S += x
    return E, n, S


def video(planes, box, g, lam, s_min):
    """planes (F, H, W) uint8 (0 off the map) and the record's box (r0, r1, c0, c1), rows r0 .. r1 - 1 and columns
    c0 .. c1 - 1 -> (E (F, H, W) uint8, n (H, W) uint32, S (H, W) float64): the rule on every pixel of the box, 0 outside"""
    planes = np.asarray(planes, np.uint8)
    F, H, W = planes.shape
    E, n, S = np.zeros((F, H, W), np.uint8), np.zeros((H, W), np.uint32), np.zeros((H, W), np.float64)
    r0, r1, c0, c1 = box
    cache = {}
    for r in range(r0, r1):
        for c in range(c0, c1):
            key = planes[:, r, c].tobytes()
            if key not in cache:
                cache[key] = pixel(list(planes[:, r, c]), g, lam, s_min)
            e, n[r, c], S[r, c] = cache[key]
            E[:, r, c] = e
    return E, n, S


def box_of(inmap):
    """the bounding box (r0, r1, c0, c1) of a map, as hm_body_rec_begin forms it"""
    rows, cols = np.flatnonzero(inmap.any(1)), np.flatnonzero(inmap.any(0))
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def objective(c, y, g, lam):
    """1/2 sum (c - y)^2 + lam sum s, s_k = c_k - g c_{k-1} for k >= 1 (the rule's penalty: lam (1 - g) per c_k, lam for
    the last)"""
    F = len(y)
    o = 0.0
    for k in range(F):
        o += 0.5 * (c[k] - y[k]) ** 2 + (lam if k == F - 1 else lam * (1.0 - g)) * c[k]
    return o


def ar1(spikes, g):
    """c_k = g c_{k-1} + spikes_k, c_0 = spikes_0"""
    c, x = [], 0.0
    for sp in spikes:
        x = g * x + sp
        c.append(x)
    return c


# ---- the planted video with its event frames ---------------------------------------------------------------------------
PLANTED_G = 0.8                     # roi_ref.planted_video: a <- 0.8 a + event


def planted_events(seed):
    """roi_ref.planted_video(seed) with the frames its events fall on -> (video, centres, activity, events (12, F) bool).
    The events are drawn again as the generator draws them (same generator, same order); that they are the generator's is
    checked: the activity they give through a <- 0.8 a + event, clipped at 1, is the one it returned."""
    v, cs, act, _ = roi_ref.planted_video(seed)
    P = roi_ref.PLANTED
    rng = np.random.default_rng(seed)
    rng.integers(40, 121, (P["H"], P["W"]))
    for _ in range(12):
        rng.integers(-4, 5), rng.integers(-4, 5)
    for _ in range(P["K"]):
        rng.uniform(P["sigma_lo"], P["sigma_hi"], 2)
        rng.uniform(0.0, np.pi)
    ev = np.zeros((P["K"], P["F"]), bool)
    for i in range(P["K"]):
        ev[i] = rng.random(P["F"]) < 0.06
        a = 0.0
        for k in range(P["F"]):
            a = a * 0.8 + (1.0 if ev[i, k] else 0.0)
            assert act[i, k] == min(a, 1.0), "the events drawn again are not the generator's"
    return v, cs, act, ev


def disc_dff(v, centres, radius=3.0, q=10.0):
    """A plain trace per cell: the mean over the disc round its centre, less and over its q-th percentile over the record
    -> (cells, F) float64"""
    F, H, W = v.shape
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for cx, cy in centres:
        d = (xx - cx) ** 2 + (yy - cy) ** 2 <= radius * radius
        f = v[:, d].astype(np.float64).mean(1)
        b = np.percentile(f, q)
        out.append((f - b) / b)
    return np.array(out)


def pooled(pairs, tol=1):
    """[(found, planted), ...] of bool (F,) per cell -> (precision, recall) over all the cells' frames together"""
    right = n_found = hit = n_planted = 0
    for found, planted in pairs:
        fi, pi = np.flatnonzero(found), np.flatnonzero(planted)
        right += sum(1 for k in fi if len(pi) and np.abs(pi - k).min() <= tol)
        hit += sum(1 for k in pi if len(fi) and np.abs(fi - k).min() <= tol)
        n_found += len(fi)
        n_planted += len(pi)
    return right / max(n_found, 1), hit / max(n_planted, 1)


PLANTED_TRACE = dict(F=20000, g=0.9, rate=0.02, lo=0.5, hi=1.5, sigma=0.2)


def planted_trace(seed):
    """A long trace with a known decay: events Bernoulli(0.02) of size uniform 0.5..1.5 through c <- 0.9 c + s, white
    Gaussian noise of sigma 0.2 on top; generator np.random.default_rng(seed) -> (y (F,), events (F,))"""
    P = PLANTED_TRACE
    r = np.random.default_rng(seed)
    sp = (r.random(P["F"]) < P["rate"]) * r.uniform(P["lo"], P["hi"], P["F"])
    return np.array(ar1(list(sp), P["g"])) + r.normal(0.0, P["sigma"], P["F"]), sp


def estimate_g(y):
    """cov(lag 2) / cov(lag 1) of the trace less its mean, in loops"""
    F = len(y)
    mean = sum(float(v) for v in y) / F
    x = [float(v) - mean for v in y]
    c1 = sum(x[k] * x[k - 1] for k in range(1, F)) / (F - 1)
    c2 = sum(x[k] * x[k - 2] for k in range(2, F)) / (F - 2)
    return c2 / c1
