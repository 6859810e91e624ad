#!/usr/bin/env python
"""optical_flow_ext.py [--video-codec raw|mjpeg] [--video-quality Q] [--depth-range LO,HI] [--depth-percentiles LO_PPM,HI_PPM]
                       [--depth-gamma G] <video> <output prefix> [alpha] [gamma] [scale_factor]
                       [inner_it] [outer_it] [solver_it]

The flow tool of the reference (reference src/optical_flow_ext.cpp:441-507) on MI355X:
for every consecutive frame pair computes the Brox flow and writes
<prefix>_%03d_x.mat and <prefix>_%03d_y.mat (format: src/optical_flow_ext.cpp:47-108).
Parameters and defaults as there (:453-488): alpha 0.197, gamma 50, scale_factor 0.8,
inner 10, outer 77, solver 10.  The video is a .npy / .npz array (frames, H, W[, 3]) uint8
(no OpenCV on this path).  All pairs of the video go to the GPU as one batch per
`HYDRA_MI_FLOW_BATCH` (default 16) pairs -- they are independent.
With HYDRA_MI_FLOW_PREVIEW=1 it also writes <prefix>.avi (:336-389): frame n is frame n + 1 as read blended
0.4 / 0.6 with the flow of pair n in the Middlebury colour code, saturating at 15 px (hm_flow_preview; the AVI is
the library's, uncompressed, 20 frames/s) -- the same bytes as the native tool writes.  --video-codec mjpeg (default
raw) writes the preview as Motion-JPEG at --video-quality (1..100, default 90) instead.
A 16-bit video (a uint16 array, a TIFF stack of 16-bit gray pages) is mapped to 8 bits through one window for the whole
recording (hydra_mi.deepio): --depth-range gives it, --depth-percentiles (parts per million, default 1000,999990) asks for
the one of the recording's histogram, --depth-gamma bends the table; run_kalmanfilter.py takes the same flags and resolves
them through the same function.
"""
import os
import sys

import numpy as np

import hydra_mi  # noqa: F401
from hydra_mi import brox, deepio, matio, pipeline, videoio


def _video_opts(av):
    """takes --video-codec / --video-quality out of the arguments -> (the rest, AviWriter's options or None on a bad one)"""
    rest, opts = [], {}
    it = iter(av)
    for s in it:
        if s in ("--video-codec", "--video-quality"):
            v = next(it, None)
            if v is None:
                return rest, None
            opts[s] = v
        else:
            rest.append(s)
    codec = opts.get("--video-codec", "raw")
    try:
        quality = int(opts.get("--video-quality", "90"))
    except ValueError:
        return rest, None
    if codec not in ("raw", "mjpeg") or not 1 <= quality <= 100:
        return rest, None
    return rest, (dict(codec="mjpeg", quality=quality) if codec == "mjpeg" else {})


def _depth_opts(av):
    """takes --depth-range / --depth-percentiles / --depth-gamma out of the arguments -> (the rest, load_video's depth);
    ValueError for a bad one"""
    rest, opts = [], {}
    it = iter(av)
    for s in it:
        if s in ("--depth-range", "--depth-percentiles", "--depth-gamma"):
            v = next(it, None)
            if v is None:
                raise ValueError("%s needs a value" % s)
            opts[s] = v
        else:
            rest.append(s)
    return rest, deepio.depth_option(opts.get("--depth-range"), opts.get("--depth-percentiles"), opts.get("--depth-gamma"))


def main(av):
    av, vopts = _video_opts(list(av))
    if vopts is None:
        sys.stderr.write("--video-codec is raw or mjpeg, --video-quality 1..100\n")
        return 1
    try:
        av, depth = _depth_opts(av)
    except ValueError as exc:
        sys.stderr.write("%s\n" % exc)
        return 1
    if len(av) < 3:
        print(__doc__)
        return 1
    try:                                             # BGR -> gray as cvtColor(BGR2GRAY) (:366-368)
        raw = pipeline.load_video(av[1], gray=False, depth=depth)
        a = np.ascontiguousarray(pipeline.to_gray(raw))
    except (OSError, ValueError) as exc:
        sys.stderr.write("Failed to open the video: %s\n" % exc)
        return 1
    prefix = av[2]
    vals = [0.197, 50.0, 0.8, 10, 77, 10]
    for i, s in enumerate(av[3:9]):
        vals[i] = float(s) if i < 3 else int(s)
    alpha, gamma, scale, inner, outer, solver = vals
    print("Using Brox optic flow parameters:\n   alpha = %g\n   gamma = %g\n   scale_factor = %g\n"
          "   inner_iterations = %d\n   outer_iterations = %d\n   solver_iterations = %d"
          % (alpha, gamma, scale, inner, outer, solver))
    B = max(1, int(os.environ.get("HYDRA_MI_FLOW_BATCH", "16")))
    n = a.shape[0] - 1
    try:
        bf = brox.BroxOpticalFlow(a.shape[2], a.shape[1], alpha, gamma, scale, inner, outer, solver,
                                  max_batch=min(B, max(n, 1)))
    except RuntimeError as exc:                      # e.g. a pyramid level of one pixel
        sys.stderr.write("%s\n" % exc)
        return 1
    preview = None
    if os.environ.get("HYDRA_MI_FLOW_PREVIEW", "") == "1":
        preview = videoio.AviWriter(prefix + ".avi", a.shape[2], a.shape[1], **vopts)
    for s in range(0, n, B):
        e = min(n, s + B)
        fx, fy = bf.calc_batch(np.ascontiguousarray(a[s:e]), np.ascontiguousarray(a[s + 1:e + 1]))
        for k in range(s, e):
            matio.write_flow(prefix, k, fx[k - s], fy[k - s])
        if preview is not None:
            for img in videoio.flow_preview(raw[s + 1:e + 1], fx[:e - s], fy[:e - s]):
                preview.write(img)
    if preview is not None:
        preview.close()
    print("Finished.")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
