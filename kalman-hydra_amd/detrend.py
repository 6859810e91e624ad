"""A running baseline per pixel of the kept registered video: seeds that survive slow brightness changes, and a dF/F video.

Bleaching and the slow brightening of tissue as the animal contracts are common to neighbouring pixels: they inflate the
local correlation of the raw registered values everywhere, and seeds found there land on the drift instead of the cells.
Here every pixel of the record a BodyReadout(keep=True) holds gets a baseline of its own -- the value at rank
q (n - 1) // 100 of the n frames k - half .. k + half, clipped at the ends (np.percentile(method="lower")) -- on the
device, in exact integers (hm_body_rec_planes / hm_body_rec_stats_add in include/hydra_mi.h, csrc/detrend_kernels.h;
tests/detrend_ref.py restates it).  The excess max(v - baseline, 0) is what the summary images and the seeds are made
from; the dF/F byte min(255, gain excess // max(baseline, floor)) is what the video shows.

    body = BodyReadout(kf, keep=True)
    for each frame: kf.compute(...); body.registered(kf.state.X, raw_frame)
    points, scores = detrend.find_points(body, 12)            # seeds of the excess video
    detrend.write_video(body, "dff.avi")                      # the dF/F video, grey, in the body frame

The record stays raw: the ROI traces of hydra_mi.roi need the raw baseline for their denominator.
"""
import numpy as np

from .body import BodyReadout
from .videoio import AviWriter, grey_opts

KINDS = ("recorded", "baseline", "excess", "dff")
DEFAULT_HALF = 20          # frames either side of the window: wider windows leave drift in
DEFAULT_Q = 10
DEFAULT_FLOOR = 16         # grey levels: darker baselines do not blow the ratio up
DEFAULT_GAIN = 255         # dF/F = 1 is white
VIDEO_BYTES = 64 << 20     # host memory a block of write_video's planes takes at most


def _check(who, what, half, q, floor=1, gain=1):
    if what not in KINDS:
        raise ValueError("%s: what %r (one of %s)" % (who, what, ", ".join(KINDS)))
    for name, v, lo, hi in (("half", half, 0, 1024), ("q", q, 0, 100), ("floor", floor, 1, 255), ("gain", gain, 1, 65535)):
        if int(v) != v or not lo <= v <= hi:
            raise ValueError("%s: %s %r outside %d..%d (a whole number)" % (who, name, v, lo, hi))


def blocks(frames, block):
    """[(k0, n), ...]: `frames` frames walked in blocks of `block`"""
    frames, block = int(frames), int(block)
    if block < 1:
        raise ValueError("blocks of %d frames" % block)
    return [(k, min(block, frames - k)) for k in range(0, frames, block)]


def write_planes(body, path, fetch, video_bytes, block=None, video_opts=None):
    """The grey AVI (B = G = R; an MJPEG video codes one component) of planes of the kept record, in the body frame:
    the record is walked in blocks of `block` frames (default: video_bytes worth of planes), fetch(k0, n) gives the
    (n, H, W) uint8 planes of a block -- or (planes, a count) -- and every plane is written -> (frames written, the
    sum of the counts).  What detrend.write_video, events.event_video and residual.write_video share."""
    F = body.r.body_rec_count()
    if block is None:
        block = max(1, video_bytes // (body.W * body.H))
    walk = blocks(F, block)
    total = 0
    with AviWriter(path, body.W, body.H, **grey_opts(video_opts)) as video:
        for k0, n in walk:
            planes = fetch(k0, n)
            if isinstance(planes, tuple):
                planes, count = planes
                total += count
            for plane in planes:
                video.write_grey(plane)
        return video.frames, total


def summary(body, what="excess", half=DEFAULT_HALF, q=DEFAULT_Q, floor=DEFAULT_FLOOR, gain=DEFAULT_GAIN):
    """The summary images of BodyReadout.summary for the planes of kind `what` of the kept record (all recorded frames):
    {"frames": F, "mean", "std", "corr": (H, W) float64, NaN outside the mesh, "max": (H, W) uint8}.  Begins the
    tracker's statistics afresh and leaves them holding these planes (find_points searches them); what
    BodyReadout.summary returned before stays as it is in the caller's hands."""
    _check("detrend.summary", what, half, q, floor, gain)
    r = BodyReadout.record(body, "detrend.summary")
    r.body_stats_begin()
    r.body_rec_stats_add(what, half, q, floor, gain)
    mean, std, corr, vmax = r.body_stats_images()
    return {"frames": r.body_stats_count(), "mean": mean, "std": std, "max": vmax, "corr": corr}


def find_points(body, n, radius=6, score="corr", min_score=None, what="excess", half=DEFAULT_HALF, q=DEFAULT_Q):
    """BodyReadout.find_points on the summary images of the planes of kind `what`: the n best local maxima of "corr",
    "std" or "range" within (2 radius + 1)^2 windows -> (points (P <= n, 2) float64 at the pixel centres, scores (P,))."""
    _check("detrend.find_points", what, half, q)
    r = BodyReadout.record(body, "detrend.find_points")
    r.body_stats_begin()
    r.body_rec_stats_add(what, half, q, DEFAULT_FLOOR, DEFAULT_GAIN)
    idx, sc, _ = r.body_stats_peaks(score, radius, -np.inf if min_score is None else float(min_score), int(n))
    return BodyReadout.pixel_points(body, idx), sc


def write_video(body, path, half=DEFAULT_HALF, q=DEFAULT_Q, floor=DEFAULT_FLOOR, gain=DEFAULT_GAIN, block=None, video_opts=None):
    """The dF/F bytes of every recorded frame as a grey AVI (B = G = R; video_opts: AviWriter's codec options, an MJPEG
    video codes one component) in the body frame -> frames written.  The planes
    are fetched `block` frames at a time (default: VIDEO_BYTES worth), so host memory stays bounded for any record."""
    _check("detrend.write_video", "dff", half, q, floor, gain)
    r = BodyReadout.record(body, "detrend.write_video")
    return write_planes(body, path, lambda k0, n: r.body_rec_planes("dff", half, q, floor, gain, k0, n), VIDEO_BYTES, block,
                        video_opts)[0]
