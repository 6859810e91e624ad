"""The kept registered video corrected for tissue compression (include/hydra_mi.h:
hm_body_rec_tri_maps / _tri_gain, csrc/deform_kernels.h; Renderer.body_rec_tri_maps / body_rec_tri_gain).

Compressed tissue is brighter: the same fluorophore sits in fewer body-frame pixels.  The tracker estimates the cause, the
area ratio J[k, t] of every triangle in every frame (hydra_mi.strain), and the record holds the effect.  The model is one
exponent for the whole animal, v ~ J^-gamma; gamma is fitted from the triangles' own mean brightness, and the record is
rewritten in place with the gain (J / Jref)^gamma of every pixel's home triangle, Jref the triangle's median J:

    out = correct(body, states)                  # body: BodyReadout(keep=True); states: those the frames were warped with
    out["gamma"], out["fit_r2"], out["gain"], out["clipped"], out["r_before"], out["r_after"]

Everything read from the record afterwards (roi.extract, demix.extract, detrend, residual, network, events) sees the
corrected frames.  The sums over the record and the rewrite are exact integers on the device; all of this file is host
arithmetic in NumPy binary64, nothing of it is compared to the device bit for bit.  Not reversible.
"""
import numpy as np

from . import strain
from .body import BodyReadout

ONE = 4096                            # the gain that changes nothing: hm_body_rec_tri_gain works in 1/4096
QMAX = 32767                          # the largest |q| hm_body_rec_tri_maps takes
Q_SCALE = 16384.0                     # the covariate Jref / J - 1 in 1/16384: +-2 fills the range
GAMMA_MAX = 3.0


def _kept(body, who):
    F = BodyReadout.record(body, "deform.%s" % who).body_rec_count()
    if F < 1:
        raise RuntimeError("deform.%s: no frame recorded" % who)
    return body.r, F


def triangle_means(body, exclude=None):
    """-> (M (F, T) float64: the mean record value of triangle t in frame k, NaN for a triangle without a pixel;
    n (T,) int64: its pixels).  exclude: (H, W) bool, pixels that do not count (cells, say).  One
    hm_body_rec_label_sums call with the body map as the label image."""
    r, F = _kept(body, "triangle_means")
    tri_of = np.asarray(body.tri_of_pixel)
    T = int(np.asarray(r.tri).shape[0])
    lab = tri_of.astype(np.int32)
    if exclude is not None:
        ex = np.asarray(exclude, bool)
        if ex.shape != lab.shape:
            raise ValueError("deform.triangle_means: exclude of shape %r for a map of %r" % (ex.shape, lab.shape))
        lab = np.where(ex, -1, lab).astype(np.int32)
    n = np.bincount(lab[lab >= 0], minlength=T).astype(np.int64)
    sums = np.asarray(r.body_rec_label_sums(lab, T)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = sums / n[None, :].astype(np.float64)
    return M, n


def fit_gamma(M, n, J, n_min=8):
    """The exponent of v ~ J^-gamma from the triangles' means: lm = log M and lj = log J of the triangles with n >= n_min
    in their frames with finite J > 0 and M > 0, each centred per triangle, gamma = -sum lm lj / sum lj^2 pooled over all
    of them and clipped to 0..3 -> dict: gamma; fitted (False, and gamma 0, where sum lj^2 is below 1e-6 x the number of
    values used: no deformation to fit from); r2, the pooled squared correlation of lm with lj; slopes (T,), the same
    ratio per triangle (NaN where it has none); used, the number of values."""
    M, J = np.asarray(M, np.float64), np.asarray(J, np.float64)
    n = np.asarray(n)
    if M.shape != J.shape or M.ndim != 2 or n.shape != (M.shape[1],):
        raise ValueError("deform.fit_gamma: means of shape %r, J of %r, counts of %r" % (M.shape, J.shape, n.shape))
    with np.errstate(invalid="ignore"):
        ok = (n >= n_min)[None, :] & np.isfinite(J) & (J > 0) & np.isfinite(M) & (M > 0)
    cnt = ok.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = np.where(ok, np.log(np.where(ok, M, 1.0)), 0.0)
        lj = np.where(ok, np.log(np.where(ok, J, 1.0)), 0.0)
        lm = np.where(ok, lm - lm.sum(0) / cnt, 0.0)
        lj = np.where(ok, lj - lj.sum(0) / cnt, 0.0)
        sxy, sxx, syy = (lm * lj).sum(0), (lj * lj).sum(0), (lm * lm).sum(0)
        slopes = np.where(sxx > 0.0, -sxy / sxx, np.nan)
    used = int(ok.sum())
    Sxy, Sxx, Syy = float(sxy.sum()), float(sxx.sum()), float(syy.sum())
    if used == 0 or Sxx < 1e-6 * used:
        return {"gamma": 0.0, "fitted": False, "r2": 0.0, "slopes": slopes, "used": used}
    r2 = Sxy * Sxy / (Sxx * Syy) if Syy > 0.0 else 0.0
    return {"gamma": float(np.clip(-Sxy / Sxx, 0.0, GAMMA_MAX)), "fitted": True, "r2": r2, "slopes": slopes, "used": used}


def _reference(J):
    """-> (J, Jref (T,): the median of every triangle's finite frames, NaN without one; ok (F, T): J finite and > 0 and
    Jref > 0)"""
    J = np.asarray(J, np.float64)
    if J.ndim != 2:
        raise ValueError("deform: J of shape %r (need frames x triangles)" % (J.shape,))
    Jref = np.full(J.shape[1], np.nan)
    for t in range(J.shape[1]):
        col = J[:, t][np.isfinite(J[:, t])]
        if len(col):
            Jref[t] = np.median(col)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(J) & (J > 0) & (Jref > 0)[None, :]
    return J, Jref, ok


def gains(J, gamma):
    """m (F, T) uint16 for hm_body_rec_tri_gain: clip(rint(4096 (J / Jref)^gamma), 1, 65535), Jref the triangle's median
    over its finite frames; 4096 where J is not finite or <= 0 (or Jref is)."""
    J, Jref, ok = _reference(J)
    with np.errstate(all="ignore"):
        g = np.power(np.where(ok, J / Jref[None, :], 1.0), np.float64(gamma))
        m = np.clip(np.rint(np.float64(ONE) * g), 1.0, 65535.0)
    return np.where(ok & np.isfinite(g), m, np.float64(ONE)).astype(np.uint16)


def covariate(J):
    """q (F, T) int32 for hm_body_rec_tri_maps: clip(rint(16384 (Jref / J - 1)), -32767, 32767), what the brightness of
    compressed tissue follows at gamma = 1; 0 where J is not finite or <= 0 (or Jref is)."""
    J, Jref, ok = _reference(J)
    with np.errstate(all="ignore"):
        x = np.clip(np.rint(Q_SCALE * (Jref[None, :] / np.where(ok, J, 1.0) - 1.0)), -float(QMAX), float(QMAX))
    return np.where(ok, x, 0.0).astype(np.int32)


def artifact_map(body, q):
    """Pearson's r over the recorded frames of every map pixel with the covariate of its own triangle, q (F, T) int32 ->
    (H, W) float64: (F c - w1 u1_t) / sqrt((F w2 - w1^2)(F u2_t - u1_t^2)) from the sums of hm_body_rec_tri_maps and the
    host's u1_t = sum q, u2_t = sum q^2; the whole numbers in int64 and Python integers, each rounded once to binary64.  NaN
    where either variance is 0 and off the map.  strain.artifact_score per pixel."""
    r, F = _kept(body, "artifact_map")
    q = np.ascontiguousarray(q, np.int32)
    tri_of = np.asarray(body.tri_of_pixel)
    m = tri_of >= 0
    c, w1, w2 = r.body_rec_tri_maps(q)
    c, w1, w2 = np.asarray(c).astype(np.int64), np.asarray(w1).astype(np.int64), np.asarray(w2).astype(np.int64)
    q64 = q.astype(np.int64)
    u1, u2 = q64.sum(0), (q64 * q64).sum(0)
    vb = np.array([float(F * int(b) - int(a) ** 2) for a, b in zip(u1, u2)], np.float64)
    t = np.where(m, tri_of, 0)
    num = (F * c - w1 * u1[t]).astype(np.float64)
    va = (F * w2 - w1 * w1).astype(np.float64)
    flat = (va == 0.0) | (vb[t] == 0.0) | ~m
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(flat, np.nan, num / np.sqrt(va * vb[t]))


def correct(body, states, gamma=None, exclude=None, n_min=8):
    """Take the brightness of compression out of the record of a BodyReadout(keep=True), in place.  states (F, 4N): the
    states the recorded frames were warped with (the filtered ones, also in a run that smooths).  gamma None: fitted from the
    triangles' means (fit_gamma), `exclude` kept out of them.  -> dict: J (F, T); q, the covariate; r_before, r_after, the
    artifact maps either side; M, n, the triangle means and counts before; gamma, fitted, fit_r2, fit_slopes; gain (F, T)
    uint16; clipped, the values the gain pushed past 255."""
    r, F = _kept(body, "correct")
    J = strain.triangles(r, states)["J"]
    if J.shape[0] != F:
        raise ValueError("deform.correct: %d states for a record of %d frames" % (J.shape[0], F))
    q = covariate(J)
    r_before = artifact_map(body, q)
    M, n = triangle_means(body, exclude)
    fit = fit_gamma(M, n, J, n_min)
    if gamma is not None:
        if not (np.isfinite(gamma) and 0.0 <= gamma <= GAMMA_MAX):
            raise ValueError("deform.correct: gamma %r outside 0..%g" % (gamma, GAMMA_MAX))
        fit = dict(fit, gamma=float(gamma), fitted=False)
    m = gains(J, fit["gamma"])
    clipped = r.body_rec_tri_gain(m)
    return {"J": J, "q": q, "r_before": r_before, "r_after": artifact_map(body, q), "M": M, "n": n, "gamma": fit["gamma"],
            "fitted": fit["fitted"], "fit_r2": fit["r2"], "fit_slopes": fit["slopes"], "gain": m, "clipped": int(clipped)}
