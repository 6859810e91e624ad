"""Stabilise the kept registered video: the residual motion of every patch of every frame, found on the device and taken
out of the record in place.

The tracker leaves about a pixel of residual motion in the registered video, and the cells are a few pixels wide.  The
record's box is cut into B x B patches; for every frame, patch and whole-pixel shift within +-S the device gives the exact
integer sums A = sum v(p + d) t(p), V1 = sum v(p + d), V2 = sum v(p + d)^2 over the patch's core (hm_body_rec_match in
include/hydra_mi.h, csrc/stab_kernels.h); the normalised correlation with the template, the choice of the shift and the
fallbacks are host arithmetic on those sums.  hm_body_rec_shift then gathers every patch at its shift, and roi.extract and
demix.extract read the stabilised record unchanged.

    body = BodyReadout(kf, keep=True)
    ... track ...
    est = stabilize.stabilize(body)          # estimate + apply
    res = roi.extract(body, points)

The first template is one recorded frame (k_ref), not the mean of the unstabilised video: on a textured animal the mean is
a blur that every frame locks onto at its most-visited shift.  A second pass matches against the rounded mean of the frames
at the first pass's shifts.  tests/stab_ref.py restates all of it in NumPy.

mode="field" takes the same motion out as a smooth sub-pixel shift field instead: every patch's shift is refined to 1/16 px
by a parabola through its score and its two neighbours' per axis, the field is bilinear between the patch centres (a patch
that fell back is filled in by its neighbours), and hm_body_rec_warp samples every frame bilinearly at it.  It is the
better choice where the residual motion is smooth and below a pixel, which is what the tracker leaves; where regions move
rigidly against each other with hard seams the patches are.  tests/stabfield_ref.py restates it.

    est = stabilize.stabilize(body, mode="field")
"""
import numpy as np

from .body import BodyReadout

#: halfway between the lowest best score of a correctly recovered patch (0.844) and the highest best score of a patch
#: matched against the template of another video, with nothing to lock onto (0.288), on the planted video with jitter
#: (tests/stab_ref.py, six seeds; tests/test_stab_cpu.py measures both)
DEFAULT_MIN_SCORE = 0.57

#: host memory the three outputs of one body_rec_match call may take (estimate walks the frames in blocks of this size)
MATCH_BYTES = 64 << 20


def patch_grid(inmap, B):
    """The record's box (the bounding box of the body map; one pixel at (0, 0) for an empty map) and the grid of B x B
    patches that tiles it from its top-left corner, row-major -> dict c0, r0, bw, bh, npx, npy, B."""
    m = np.asarray(inmap, bool)
    B = int(B)
    if B < 1:
        raise ValueError("stabilize: patch size %d" % B)
    if not m.any():
        c0 = r0 = 0
        bw = bh = 1
    else:
        rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        c0, r0 = int(cols[0]), int(rows[0])
        bw, bh = int(cols[-1]) - c0 + 1, int(rows[-1]) - r0 + 1
    return dict(c0=c0, r0=r0, bw=bw, bh=bh, npx=(bw + B - 1) // B, npy=(bh + B - 1) // B, B=B)


def core_mask(inmap, S):
    """(H, W) bool: the map pixels whose whole (2S + 1)^2 neighbourhood is on the frame and in the map."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    pad = np.zeros((H + 2 * S, W + 2 * S), bool)
    pad[S:S + H, S:S + W] = m
    out = np.ones((H, W), bool)
    for dy in range(2 * S + 1):
        for dx in range(2 * S + 1):
            out &= pad[dy:dy + H, dx:dx + W]
    return out


def _patch_sums(img, grid):
    """(H, W) int64 -> (patches,) int64: the sum over every patch of the grid"""
    B, npx, npy = grid["B"], grid["npx"], grid["npy"]
    box = np.zeros((npy * B, npx * B), np.int64)
    box[:grid["bh"], :grid["bw"]] = img[grid["r0"]:grid["r0"] + grid["bh"], grid["c0"]:grid["c0"] + grid["bw"]]
    return box.reshape(npy, B, npx, B).sum((1, 3)).reshape(-1)


def scores(A, V1, V2, n, St, Stt):
    """The normalised correlation of every (frame, patch, shift) from the whole-number sums: cov = n A - V1 St,
    var_v = n V2 - V1^2, var_t = n Stt - St^2 in int64, each rounded once to binary64 (they are exact there); then one
    product, one square root, one division.  -inf where a variance is 0 (an invalid shift)."""
    A, V1, V2 = (np.asarray(x).astype(np.int64) for x in (A, V1, V2))
    n, St, Stt = (np.asarray(x).astype(np.int64)[None, :, None] for x in (n, St, Stt))
    cov = (n * A - V1 * St).astype(np.float64)
    var_v = (n * V2 - V1 * V1).astype(np.float64)
    var_t = np.broadcast_to((n * Stt - St * St).astype(np.float64), var_v.shape)
    valid = (var_v > 0.0) & (var_t > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(valid, cov / np.sqrt(var_v * var_t), -np.inf)


def choose(sc, n_core, S, min_score, n_min):
    """sc (F, patches, (2S+1)^2) scores, -inf: invalid -> (shifts (F, patches, 2) int8 (dx, dy), score (F, patches) float64
    (NaN: no valid shift), fallback (F, patches) bool).  The highest score wins; ties go to the smaller dx^2 + dy^2, then
    to the lower shift index.  A patch with fewer than n_min core pixels, without a valid shift or with a best score below
    min_score gets (0, 0) and is flagged."""
    n1 = 2 * S + 1
    idx = np.arange(n1 * n1)
    dy, dx = idx // n1 - S, idx % n1 - S
    best = sc.max(2)
    key = np.where(sc == best[:, :, None], (dx * dx + dy * dy) * (n1 * n1) + idx, np.iinfo(np.int64).max)
    pick = key.argmin(2)
    found = best > -np.inf
    fallback = (np.asarray(n_core)[None, :] < n_min) | ~found | (np.where(found, best, 0.0) < min_score)
    shifts = np.stack((dx[pick], dy[pick]), 2).astype(np.int8)
    shifts[fallback] = 0
    return shifts, np.where(found, best, np.nan), fallback


def subpixel(sc, shifts, fallback, S):
    """The shifts refined to 1/16 px -> q (F, patches, 2) int16 (dx, dy).  sc (F, patches, (2S+1)^2) scores, -inf: invalid;
    shifts and fallback as choose gives them.  Per axis, with s0 the winner's score and s-, s+ those of its two neighbours
    along the axis: where the winner is strictly inside the search (|d| < S), both neighbours are valid and
    den = s- - 2 s0 + s+ < 0, off = (s- - s+) / (2 den) clipped to +-0.5, else 0; q = 16 d + floor(16 off + 0.5).  A patch
    that fell back has q = 0.  Every step is one binary64 operation in this order."""
    n1 = 2 * S + 1
    sh = np.asarray(shifts).astype(np.int64)
    fb = np.asarray(fallback, bool)
    idx = (sh[:, :, 1] + S) * n1 + sh[:, :, 0] + S
    s0 = np.take_along_axis(sc, idx[:, :, None], 2)[:, :, 0]
    q = np.zeros(sh.shape, np.int16)
    for axis, step in ((0, 1), (1, n1)):
        inside = (np.abs(sh[:, :, axis]) < S) & ~fb
        lo = np.take_along_axis(sc, np.where(inside, idx - step, idx)[:, :, None], 2)[:, :, 0]
        hi = np.take_along_axis(sc, np.where(inside, idx + step, idx)[:, :, None], 2)[:, :, 0]
        ok = inside & (lo > -np.inf) & (hi > -np.inf) & (s0 > -np.inf)
        lo, hi, mid = (np.where(ok, x, 0.0) for x in (lo, hi, s0))
        den = (lo - 2.0 * mid) + hi
        ok &= den < 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            off = np.where(ok, (lo - hi) / (2.0 * den), 0.0)
        off = np.minimum(np.maximum(off, -0.5), 0.5)
        q[:, :, axis] = (16 * sh[:, :, axis] + np.floor(16.0 * off + 0.5).astype(np.int64)).astype(np.int16)
    q[fb] = 0
    return q


def mean_template(sums, F):
    """The rounded mean of F frames from their per-pixel sums: (2 sum + F) // (2 F), uint8."""
    s = np.asarray(sums).astype(np.int64)
    return ((2 * s + F) // (2 * F)).astype(np.uint8)


MODES = ("patch", "field")


def estimate(body, B=16, S=3, k_ref=0, passes=1, min_score=None, n_min=None, mode="patch"):
    """The shift of every patch of every frame a BodyReadout(keep=True) has recorded.  -> dict:
      shifts (F, patches, 2) int8 (dx, dy)   gather the patch at p + d (body_rec_shift does)
      score (F, patches) float64             the best normalised correlation with the template (NaN: no valid shift)
      fallback (F, patches) bool             the patch keeps (0, 0): too few core pixels, no valid shift, or a low score
      n_core (patches,) uint32, grid (patch_grid), templates (one (H, W) uint8 per pass), B, S
    Pass 1 matches against record frame k_ref.  Pass p > 1 matches the ORIGINAL record against the rounded mean of the
    frames at the previous pass's shifts; its shifts replace the previous ones.  min_score None: DEFAULT_MIN_SCORE; n_min
    None: B B / 4 core pixels.
    mode "field" adds q (F, patches, 2) int16, the shifts refined to 1/16 px (subpixel), valid (F, patches) uint8, the
    patches that did not fall back, and mode; pass p > 1 then matches against the rounded mean of the frames sampled at the
    previous pass's field (body_rec_field_sums)."""
    if mode not in MODES:
        raise ValueError("stabilize.estimate: mode %r (one of %s)" % (mode, ", ".join(MODES)))
    r = BodyReadout.record(body, "stabilize.estimate")
    F = r.body_rec_count()
    if F < 1:
        raise RuntimeError("stabilize.estimate: no frame recorded")
    B, S, passes = int(B), int(S), int(passes)
    if not 0 <= int(k_ref) < F or passes < 1:
        raise ValueError("stabilize.estimate: k_ref %d of %d frames, %d passes" % (k_ref, F, passes))
    min_score = DEFAULT_MIN_SCORE if min_score is None else float(min_score)
    n_min = B * B / 4 if n_min is None else n_min
    m = np.asarray(body.tri_of_pixel) >= 0
    grid = patch_grid(m, B)
    core = core_mask(m, S)
    npatch, nsh = grid["npx"] * grid["npy"], (2 * S + 1) ** 2
    block = max(1, MATCH_BYTES // (3 * 4 * npatch * nsh))
    template = np.where(m, r.body_rec_fetch(int(k_ref), 1)[0], 0).astype(np.uint8)
    templates, out = [], None
    for p in range(passes):
        if p > 0 and mode == "field":
            template = mean_template(r.body_rec_field_sums(out["q"], out["valid"], B), F)
        elif p > 0:
            template = mean_template(r.body_rec_frame_sums(out["shifts"], B), F)
        templates.append(template)
        t = np.where(core, template, 0).astype(np.int64)
        St, Stt = _patch_sums(t, grid), _patch_sums(t * t, grid)
        shifts = np.zeros((F, npatch, 2), np.int8)
        q = np.zeros((F, npatch, 2), np.int16)
        score = np.full((F, npatch), np.nan)
        fallback = np.zeros((F, npatch), bool)
        n_core = None
        for k0 in range(0, F, block):
            n = min(block, F - k0)
            ms = r.body_rec_match(template, B, S, k0, n)
            n_core = ms["n_core"]
            if not np.array_equal(n_core.astype(np.int64), _patch_sums(core.astype(np.int64), grid)):
                raise RuntimeError("stabilize.estimate: the cores of the patches differ between host and device")
            sc = scores(ms["A"], ms["V1"], ms["V2"], n_core, St, Stt)
            shifts[k0:k0 + n], score[k0:k0 + n], fallback[k0:k0 + n] = choose(sc, n_core, S, min_score, n_min)
            if mode == "field":
                q[k0:k0 + n] = subpixel(sc, shifts[k0:k0 + n], fallback[k0:k0 + n], S)
        out = dict(shifts=shifts, score=score, fallback=fallback, n_core=n_core, grid=grid, templates=templates, B=B, S=S)
        if mode == "field":
            out.update(q=q, valid=(~fallback).astype(np.uint8), mode=mode)
    return out


def apply(body, est):
    """Rewrite the record in place at the estimated shifts (hm_body_rec_shift), or for an estimate of mode "field" at its
    field (hm_body_rec_warp); not reversible."""
    if est.get("mode", "patch") == "field":
        body.r.body_rec_warp(est["q"], est["valid"], est["B"])
    else:
        body.r.body_rec_shift(est["shifts"], est["B"])


def stabilize(body, **kw):
    """estimate(body, **kw), then apply -> the estimate."""
    est = estimate(body, **kw)
    apply(body, est)
    return est
