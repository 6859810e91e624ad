"""Cells hidden beside found ones: the residual video of the demixed model, and the seeds found in it (DESIGN.md
section 15).

find_points cannot return two cells closer than its window, so a cell beside a brighter one is never seeded and
hydra_mi.demix never hears of it.  Here the fitted light of the cells found so far is taken out of every frame of the
record a BodyReadout(keep=True) holds -- on the device, in exact integers (hm_body_rec_residual_planes /
hm_body_rec_residual_stats_add in include/hydra_mi.h, csrc/residual_kernels.h; tests/residual_ref.py restates it):

    R_k(p) = min(255, max(0, offset + v_k(p) - ((sum_j weights[j][p] traces[k][labels[j][p]] + 2^23) >> 24)))

with the shapes of demix.extract as weights and its traces, centred over time and scaled by 2^24, as traces.  A disc round
every known seed is blanked (R = 0: where the model misfits its own cell), and the local correlation of what is left
shows the partners:

    body = BodyReadout(kf, keep=True, stats=True)
    ... track ...
    points, scores = body.find_points(12, min_score=0.8)
    more = residual.find_more(body, points, min_score=0.8)
    more["points"], more["e"]["C"]                            # all the cells, and their demixed traces

The record stays raw.  The tracker's statistics are begun afresh and left holding the last residual video.
"""
import math

import numpy as np

from . import cellview, demix, detrend, roi
from .body import BodyReadout

TBITS = 24                 # traces are scaled by 2^24: a weight of 65535 and a trace of rint(l 2^24 / 65535) take l levels off
DEFAULT_BLANK = 2          # px round every known seed
DEFAULT_OFFSET = 64        # grey levels added so that what the model overshoots by stays visible
VIDEO_BYTES = 64 << 20     # host memory a block of write_video's planes takes at most
_ROI_ARGS = ("r_disc", "r_in", "r_out", "R", "thr")


def _points_of(who, e, points):
    if points is None:
        if "points" not in e:
            raise ValueError("%s: the dict carries no points (find_more's does): pass points=" % who)
        points = e["points"]
    return np.asarray(points, np.float64).reshape(-1, 2)


def _check(who, blank, offset):
    if blank is not None and (int(blank) != blank or blank < 0):
        raise ValueError("%s: blank %r (a whole number of pixels >= 0, or None)" % (who, blank))
    if int(offset) != offset or not 0 <= offset <= 255:
        raise ValueError("%s: offset %r outside 0..255 (a whole number)" % (who, offset))


def model(e, shape, n_layers=4, points=None):
    """The dict of demix.extract -> (labels (n_layers, H, W) int32, weights (n_layers, H, W) uint16, traces (F, P) int32,
    dropped): the layers of cellview.layers_from_shapes(e["shapes_q"], seeds, R, shape, n_layers) and
    traces[k, s] = rint(c~_s(k) 2^24), where c_s = C_s sum a_q,s / sum a_q,s^2 is the solution of G c = d that demix
    scaled to C and c~_s = c_s - mean_k c_s (the mean is the exactly rounded sum over F): the
    static texture stays in the residual, the local correlation does not see it.  points: the seeds of e (None:
    e["points"], which find_more's dicts carry).  A trace value outside int32 raises."""
    pts = _points_of("residual.model", e, points)
    a_q = np.asarray(e["shapes_q"])
    C = np.asarray(e["C"], np.float64)
    F, P = C.shape
    if a_q.ndim != 3 or a_q.shape[0] != P or pts.shape[0] != P or a_q.shape[1] != a_q.shape[2] or not a_q.shape[1] & 1:
        raise ValueError("residual.model: shapes of shape %r and %d points for traces of %d cells" % (a_q.shape, pts.shape[0], P))
    seeds = roi.seeds_of(pts)
    R = a_q.shape[1] // 2
    labels, weights, dropped = cellview.layers_from_shapes(a_q, seeds, R, shape, n_layers)
    traces = np.zeros((F, P), np.int32)
    A = a_q.astype(np.int64)
    for s in range(P):
        sa, g = int(A[s].sum()), int((A[s] * A[s]).sum())
        if g == 0:
            continue
        c = C[:, s] * (np.float64(sa) / np.float64(g))
        t = np.rint((c - np.float64(math.fsum(c.tolist()) / F)) * np.float64(2.0 ** TBITS))
        if not (np.abs(t) < 2.0 ** 31).all():                    # (NaN fails too)
            raise OverflowError("residual.model: the trace of cell %d does not fit int32 (largest %g)" % (s, np.abs(t).max()))
        traces[:, s] = t.astype(np.int32)
    return labels, weights, traces, dropped


def blank_discs(points, radius, shape):
    """(H, W) uint8: 1 on the discs dx^2 + dy^2 <= radius^2 round the pixel each point lies in, clipped to the frame."""
    H, W = int(shape[0]), int(shape[1])
    radius = int(radius)
    out = np.zeros((H, W), np.uint8)
    d = np.arange(-radius, radius + 1)
    disc = d[None, :] ** 2 + d[:, None] ** 2 <= radius * radius
    for c, r in roi.seeds_of(points):
        rr, cc, on = roi._window(H, W, (c, r), radius)
        out[rr[disc & on], cc[disc & on]] = 1
    return out


def _args(who, body, e, blank, offset, points):
    _check(who, blank, offset)
    pts = _points_of(who, e, points)
    labels, weights, traces, dropped = model(e, (body.H, body.W), points=pts)
    bl = None if blank is None else blank_discs(pts, blank, (body.H, body.W))
    return labels, weights, traces, bl, dropped


def summary(body, e, blank=DEFAULT_BLANK, offset=DEFAULT_OFFSET, points=None):
    """The summary images of detrend.summary for the residual video of the model of e (the dict of demix.extract; points:
    its seeds, None: e["points"]), a disc of `blank` px round every seed blanked (None: none) -> that dict plus "clipped"
    (values that left 0..255 before the clamp) and "dropped" ((pixel, cell) entries beyond the four layers).  Begins the
    tracker's statistics afresh and leaves them holding the residual video."""
    r = BodyReadout.record(body, "residual.summary")
    labels, weights, traces, bl, dropped = _args("residual.summary", body, e, blank, offset, points)
    r.body_stats_begin()
    clipped = r.body_rec_residual_stats_add(labels, weights, traces, bl, int(offset))
    mean, std, corr, vmax = r.body_stats_images()
    return {"frames": r.body_stats_count(), "mean": mean, "std": std, "max": vmax, "corr": corr, "clipped": clipped,
            "dropped": dropped}


def _rois_ok(body, points, r_disc=3.0, r_in=6.0, r_out=8.5, R=8, thr=None):
    """roi.extract up to its ROIs: does every seed keep an ROI pixel of its own?"""
    r = body.r
    m = body.tri_of_pixel >= 0
    seeds = roi.seeds_of(points)
    ss = r.body_rec_seed_sums(seeds, r_disc, r_in, r_out, R)
    rho = roi.footprints(ss, r.body_rec_count(), m, seeds, R)
    counts = roi.assign(rho, roi.DEFAULT_THR if thr is None else float(thr), m, seeds, R, r_disc)[1]
    return bool((counts >= 1).all())


def find_more(body, points, min_score, rounds=3, radius=6, score="corr", blank=DEFAULT_BLANK, offset=DEFAULT_OFFSET,
              max_new=None, **demix_args):
    """Seeds hidden beside the cells at `points` ((P, 2) in body coordinates).  Up to `rounds` times: demix.extract on
    the points so far (demix_args go to it), the statistics of the residual video (summary), and its peaks of `score`
    within (2 radius + 1)^2 windows that reach min_score.  The candidates are taken in score order; one is refused when
    it lies in a pixel already seeded ("seeded") or when with it roi.extract would leave a seed without an ROI pixel of
    its own ("roi").  A round that accepts none ends the search.  At most max_new points are added (None: no limit).

    min_score has no default: it is a property of the video.  Read it off the first pass: sort the scores of
    body.find_points(n) for a generous n; cells and background are separated by a gap, and min_score goes into it.  On
    the paired planted video the pair leaders score >= 0.89 and the best background peak 0.74;
    the residual passes show the same gap (hidden partners 5 or 6 px away >= 0.83, background <= 0.74), so the same
    value serves them.

    -> dict: points (old ones first, then the new in the order found), round (P,) the round that found each point (0:
    given), new_scores (the scores of the points added, in their order), scores [per round: the scores of its candidates, descending], accepted [per round: how many were taken],
    refused [(round, point (2,), score, reason)], clipped [per round], dropped, ended ("none accepted" or "rounds"),
    e: the last demix.extract dict, of all the points (with e["points"]), so the caller does not demix again."""
    r = BodyReadout.record(body, "residual.find_more")
    _check("residual.find_more", blank, offset)
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("residual.find_more: rounds %d" % rounds)
    if min_score is None or not np.isfinite(float(min_score)):
        raise ValueError("residual.find_more: min_score %r (a finite number: see the docstring)" % (min_score,))
    if max_new is not None and int(max_new) < 0:
        raise ValueError("residual.find_more: max_new %r" % (max_new,))
    pts = np.array(points, np.float64).reshape(-1, 2)
    if pts.shape[0] < 1:
        raise ValueError("residual.find_more: no point to start from")
    n_given = pts.shape[0]
    roi_args = {k: demix_args[k] for k in _ROI_ARGS if k in demix_args}
    out = dict(round=[0] * pts.shape[0], new_scores=[], scores=[], accepted=[], refused=[], clipped=[], dropped=0, ended="rounds")
    e = demix.extract(body, pts, **demix_args)
    for rnd in range(1, rounds + 1):
        e["points"] = pts.copy()
        s = summary(body, e, blank, offset)
        out["clipped"].append(s["clipped"])
        out["dropped"] = s["dropped"]
        idx, sc, _ = r.body_stats_peaks(score, radius, float(min_score))
        out["scores"].append(sc)
        taken = 0
        for i, v in zip(idx.tolist(), sc.tolist()):
            if max_new is not None and pts.shape[0] - n_given >= int(max_new):
                break
            cand = BodyReadout.pixel_points(body, [i])[0]
            if (roi.seeds_of(pts) == roi.seeds_of(cand)[0]).all(1).any():
                out["refused"].append((rnd, cand, v, "seeded"))
                continue
            trial = np.vstack((pts, cand))
            if not _rois_ok(body, trial, **roi_args):
                out["refused"].append((rnd, cand, v, "roi"))
                continue
            pts = trial
            out["round"].append(rnd)
            out["new_scores"].append(v)
            taken += 1
        out["accepted"].append(taken)
        if taken == 0:
            out["ended"] = "none accepted"
            break
        e = demix.extract(body, pts, **demix_args)
    e["points"] = pts.copy()
    out.update(points=pts, round=np.array(out["round"], np.int32), new_scores=np.array(out["new_scores"], np.float64), e=e)
    return out


def write_video(body, path, e, blank=None, offset=DEFAULT_OFFSET, points=None, block=None, video_opts=None):
    """The residual planes of every recorded frame as a grey AVI (B = G = R; video_opts: AviWriter's codec options, an
    MJPEG video codes one component) in the body frame -> (frames written,
    clipped).  The planes are fetched `block` frames at a time (default: VIDEO_BYTES worth), so host memory stays bounded
    for any record.  blank None: the video shows the misfit round the seeds too."""
    r = BodyReadout.record(body, "residual.write_video")
    labels, weights, traces, bl, _ = _args("residual.write_video", body, e, blank, offset, points)
    return detrend.write_planes(body, path, lambda k0, n: r.body_rec_residual_planes(labels, weights, traces, bl, int(offset), k0, n),
                                VIDEO_BYTES, block, video_opts)
