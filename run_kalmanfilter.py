#!/usr/bin/env python
"""run_kalmanfilter.py [input_video] [optic_flow_path] [output_file] -- HydraGL tracker on MI355X.

Same arguments as the reference CLI (reference run_kalmanfilter.py:38-53):

    fn_in            input video.  No OpenCV here: a .npy / .npz array of shape (frames, H, W)
                     or (frames, H, W, 3) (BGR, converted as cvtColor BGR2GRAY does), 8-bit; or an .avi,
                     Motion-JPEG (decoded on the GPU, hydra_mi.videoio.MjpegDecoder; a colour file gives its
                     luma plane) or uncompressed 24-bit.  With a Motion-JPEG file and the flow computed
                     in-process, the decoder fills the pipeline's frame ring itself (videoio.AviSource): frames of
                     512 or more restart intervals reach the GPU as JPEG bytes; for others the Huffman decoding
                     runs on the CPU and the coefficients are uploaded, 2 bytes a pixel
    flow_in          optic flow path prefix: <flow_in>_%03d_x.mat / _y.mat as written by the
                     flow tool (optical_flow_ext.py); if no flow files exist the flow is
                     computed in-process with the same Brox defaults, streamed to the filter on
                     the GPU (hydra_mi.pipeline.FlowEKFPipeline)
    fn_out           output file: the tracked states of all frames (np.savez; a name without .npz gets it
                     appended).  When it ends in .avi the overlay video of the run is written there as well
                     (reference :43-44; uncompressed 24-bit AVI at 20 frames/s, hydra_mi.videoio) and the
                     states go to <fn_out>.npz
    -n/--name        when given: the reference's screenshots of every frame k (:89),
                     screenshots/<name>_frame_<k>_{raw,overlay,texture,mask,flowx,flowy,forces}.png
                     (no time stamp in the names, unlike the reference)
    -t/--threshold   threshold intensity below which is background (default 9)
    -s/--gridsize    edge length for mesh (default 22)
    -c/--cuda        whether to do the analysis on the GPU (default True; there is no CPU path)
    --registered OUT.avi   the registered video: every raw frame pulled back through the tracked mesh into body
                     coordinates (the frame-0 grid of the initial mesh; hydra_mi.body)
    --points FILE.csv      points in body coordinates, lines name,x,y (reference synth.py:227-231), followed through
                     the mesh and read out over discs of --point-radius px (default 3)
    With --registered or --points the states file also gets tri_means (frames x triangles) and tri_counts, and with
    --points points (frames x P x 2), point_means (frames x P), point_counts and <fn_out>_points.txt (one line
    neurons,x0,y0,... per frame, reference synth.py:245-266).  Rows line up with X.
    --find-points N  find the cells: the statistics of the registered video are accumulated on the GPU while it is
                     tracked (hydra_mi.body, BodyReadout(stats=True)); the states file gets the summary images body_mean,
                     body_std, body_max, body_corr (H x W; NaN, body_max 0, outside the mesh) and found_points (P <= N, 2),
                     found_scores: the N best local maxima of --find-score (corr: mean correlation with the 8 neighbours,
                     the default; std; range: max - mean) within windows of --find-radius px (default 6).  A second pass
                     over the recorded states then reads them out as --points would (points, point_means, point_counts,
                     <fn_out>_points.txt); --points-out FILE.csv writes them in the format --points reads.  Not together
                     with --points.
    --rois           with --find-points or --points: keep the registered video on the device while tracking (hydra_mi.body,
                     BodyReadout(keep=True), at most --rois-max-gb GiB) and build footprints, ROIs and neuropil-corrected
                     dF/F traces of the points from it (hydra_mi.roi.extract): roi_points (indices of the points inside
                     the mesh, the rows of the rest), roi_footprints, roi_labels (H x W), roi_counts, roi_ring_counts,
                     roi_F, roi_Fnp, roi_dff (frames x points), roi_seed_fallback.  With --find-points the disc traces
                     come from the record as well: no second pass over the video.  A video whose record would not fit is
                     said to be so and read out as without --rois.
    --demix          --rois, and the overlapping cells demixed (hydra_mi.demix.extract: shapes and traces fitted in turn
                     to the kept video, --demix-iters rounds): demix_shapes (points x 17 x 17), demix_C, demix_dff
                     (frames x points), demix_change (the relative change of demix_C per round).
    --stabilize      with --rois or --demix: before the cells are read out, take the residual motion out of the kept
                     registered video (hydra_mi.stabilize): every patch of --stab-patch px (default 16) of every frame is
                     matched against a template within +-(--stab-search) px (default 3) on the device and gathered at its best
                     shift, --stab-passes times (default 1; from the second pass on the template is the mean of the
                     stabilised frames).  The states file gets stab_shifts (frames x patches x 2, (dx, dy)), stab_score,
                     stab_fallback (frames x patches).  Everything read from the kept record sees the stabilised frames:
                     the roi_* and demix_* arrays and, with --find-points, point_means.  What is summed while tracking does
                     not: tri_means, the summary images body_* and the points found in them, point_means of --points.
                     --cells-video keeps drawing at the tracked states.
                     --stab-mode field (default patch) takes the motion out as a smooth shift field instead of one whole
                     pixel vector per patch: the shifts refined to 1/16 px, bilinear between the patch centres, fallback
                     patches filled in by their neighbours, the frames sampled bilinearly.  The choice for the smooth
                     sub-pixel motion a tracker leaves; patch for regions that move rigidly against each other.  The states
                     file then also gets stab_q (frames x patches x 2, int16, (dx, dy) in 1/16 px).
    --deform-correct with --rois or --demix: take the brightness of compressed tissue out of the kept registered video
                     (hydra_mi.deform), after --stabilize and before everything that reads the record: every pixel of every
                     frame times (J / Jref)^gamma of its home triangle, J the triangle's area ratio at the filtered states the
                     frames were warped with (also with --smooth), Jref its median, gamma fitted from the triangles' mean
                     brightness (--deform-gamma G: taken as given, 0..3).  The states file gets deform_gamma, deform_fit_r2,
                     deform_gain (frames x triangles, uint16, 4096 = 1), deform_clipped, and deform_r_before,
                     deform_r_after: every pixel's correlation with its triangle's Jref / J either side of the correction.
                     What is summed while tracking keeps the uncorrected frames: tri_means, body_*, point_means of --points.
    --detrend        with --find-points: search the summary images of the excess video instead of the raw one (hydra_mi.detrend):
                     every pixel of the kept registered video less its own running baseline, the value at rank
                     q (n - 1) // 100 of the n frames k - half .. k + half (--detrend-half, default 20; --detrend-q, default
                     10), computed on the device.  Seeds found this way survive bleaching and slow brightness changes of the
                     tissue.  Keeps the registered video on the device as --rois does (same budget, --rois-max-gb; a video
                     that does not fit is said to be so and searched raw).  The states file gets detrend_mean, detrend_std,
                     detrend_max, detrend_corr, the summary images of the excess video; body_* stay those of the frames as
                     tracked.  With --stabilize the record is stabilised first and the seeds are found after it.
    --resummarize    with --stabilize, without --detrend: detrend_* are the summary images of the stabilised record as it is,
                     and --find-points searches those.
    --dff-video OUT.avi   the dF/F video in the body frame, grey: min(255, gain excess // max(baseline, floor)) per pixel
                     (--dff-gain, default 255; --dff-floor, default 16; the window of --detrend-half, --detrend-q), of the
                     stabilised record with --stabilize.  Keeps the registered video on the device as --rois does.
    --find-min-score S   with --find-points: only local maxima that score at least S are points (default: no threshold).
    --find-more ROUNDS   with --find-points and --find-min-score: look for cells hidden beside the ones found
                     (hydra_mi.residual.find_more; implies --demix).  Up to ROUNDS times the points so far are demixed, the
                     fitted light of their cells is taken out of the kept registered video on the device, a disc of
                     --find-blank px (default 2) round every point is blanked, and the local maxima of --find-score of
                     that residual video that reach S become points.  A round that adds none ends the search.
                     found_points, found_scores and --points-out get all the points, the new ones last; the states file
                     also gets residual_round (per point: the round that found it, 0 the first pass), residual_scores and
                     residual_scores_round (every candidate's score and its round), residual_clipped (per round: values
                     that left 0..255 before the clamp).  The demix_* arrays are those of all the points.
    --video-codec raw|mjpeg   the codec of every video this command writes (fn_out.avi, --registered, --dff-video,
                     --residual-video, --cells-video, --strain-video, --events-video).  raw (default): uncompressed 24-bit
                     AVI.  mjpeg: Motion-JPEG, every frame a baseline JPEG coded on the device (hydra_mi.videoio); the four
                     grey videos (--registered, --dff-video, --residual-video, --events-video) are coded with one component.
                     videoio.read_avi reads either back.
    --video-quality Q   with --video-codec mjpeg: the JPEG quality, 1..100 (default 90)
    --residual-video OUT.avi   with --demix or --find-more: the registered video less the demixed cells' light plus 64,
                     grey, in the body frame (hydra_mi.residual.write_video): what the model does not explain.
    --smooth         also smooth the track backward (Rauch-Tung-Striebel, hydra_mi.smooth): the states file gets Xs
                     (frames x 4N, each frame's estimate from all frames) and Xs_std (the square roots of the
                     diagonals of the smoothed covariances).  The record of the filter takes (4N)^2 doubles of device
                     memory per frame; a video beyond --smooth-max-gb fails before tracking starts.
    --cells-video OUT.avi  after tracking: the cells on the moving animal (hydra_mi.cellview) -- every raw frame with the
                     demixed shapes (--demix) or the ROIs (--rois) of the points blended in by their dF/F of that frame,
                     outlined, and a marker on every tracked point; with --points or --find-points alone the markers only.
                     Needs one of --points, --find-points, --rois, --demix.  Drawn at the smoothed states Xs with
                     --smooth, else at the filtered ones (--cells-video-states filtered|smoothed overrides).  One more
                     pass over the frames of the input video.
    --strain         the deformation of the tracked mesh (hydra_mi.strain): the states file gets strain_J (the area ratio of
                     every triangle against the body frame), strain_l1, strain_l2 (its principal stretches), strain_axis (the
                     direction of l1 in the body frame, radians), strain_rotation (frames x triangles) and strain_body_area
                     (frames: the area of the whole mesh over its rest area) -- of the smoothed states Xs with --smooth, else
                     of the filtered ones.  With cells (--points, --find-points, --rois, --demix) also strain_cell_J,
                     strain_cell_l1, strain_cell_l2 (frames x cells): their mean over the pixels of every cell, the ROI
                     with --rois, else the disc of --point-radius; and with dF/F traces (--rois, --demix) strain_artifact_r
                     (cells): Pearson's r between a cell's local area ratio and its dF/F -- compressed tissue is brighter,
                     so a cell whose trace follows its tissue's area change is suspect.  A diagnostic, not a correction.
    --strain-video OUT.avi   after tracking: every raw frame with --strain-which (J, l1 or l2; default J) of the triangle under
                     each pixel painted on, blue compressed, white unchanged, red stretched: level 128 + --strain-gain
                     (value - 1) (default 256) of a 256-colour table, blended at --strain-alpha / 255 (default 128).  At the
                     states --strain uses.  One more pass over the frames of the input video.
    --network        with --rois or --demix: the cells that fire together (hydra_mi.network), from the dF/F of --demix if on,
                     else of --rois, as it is.  net_r (cells x cells x 2 LAG + 1): Pearson's r of every pair of traces at
                     the lags -LAG..LAG (--network-lag, default 10); net_labels (cells): the ensemble of every cell, the
                     connected components of r at lag 0 >= --network-thr, -1 for a cell alone; net_ens_traces (ensembles x
                     frames): their mean dF/F; net_lead_lag, net_lead_r (ensembles x ensembles): the lag at which the
                     second follows the first best, and that r; net_rho (ensembles x H x W): the correlation of every pixel
                     of the kept registered video with every ensemble's trace, made on the device and rounded to float32
                     here; net_map (H x W, int16): per pixel the ensemble with the largest rho if that is >=
                     --network-map-thr, else -1; with --strain also net_strain_r (ensembles x triangles): Pearson's r
                     between an ensemble's trace and a triangle's area ratio.
    --network-map OUT.png   with --network: net_map in the ensembles' colours over the mean registered frame (with
                     --network-null: net_map_sig).
    --network-null N   with --network: significance against N circular shifts of the traces (all of them if there are no
                     more; a shift is at least --network-guard + 1 frames from 0 either way, default 10; drawn with
                     --network-seed, default 0).  net_p_r (cells x cells): per ordered pair the share of shifted second
                     traces that correlate with the first at least as well; net_rho_max (ensembles x shifts): per shifted
                     ensemble trace the largest rho over the whole map, made on the device; net_p_map (ensembles x H x W,
                     float32): the share of those maxima that reach the pixel's rho, a p-value that holds for the whole
                     map at once; net_sig (bool): net_p_map <= --network-alpha (default 0.05); net_map_sig: net_map with
                     -1 where the winning ensemble's pixel is not significant.
    --events         with --rois or --demix: the events behind the traces (hydra_mi.events), AR(1) deconvolution of the dF/F
                     of --demix if on, else of --rois: c_k = g c_{k-1} + s_k with s >= 0, least squares with the penalty
                     lambda on the events.  Per cell g from the trace's autocovariance (events.estimate_g), lambda and the
                     least event that counts from its noise (events.noise, default_lam, default_smin), unless --events-g,
                     --events-lambda, --events-smin fix them for all cells.  ev_g, ev_lambda (cells); ev_c, ev_s (cells x
                     frames): the calcium and the events; ev_binary (bool): s >= s_min.  The same rule on every pixel of
                     the dF/F bytes of the kept registered video, on the device, with one g (the median over the cells) and
                     the cells' median lambda and s_min in bytes (x --dff-gain; s_min at least 1): ev_count_image (H x W,
                     uint32: frames with an event >= s_min), ev_sum_image (H x W: the events summed, rounded to float32 here);
                     ev_params: g, lambda, s_min of the pixels, then half, q, floor, gain of their dF/F bytes.  With
                     --network also net_r_events: network.coactivity of ev_s, as net_r is of the traces.
    --waves          with a kept record (--rois, --demix, --detrend, --dff-video) and --network or --waves-frames: where every
                     ensemble's events start and how they travel (hydra_mi.waves).  The triggers are the onsets of the
                     ensembles' traces (waves.triggers) whose windows lie inside the record; around each, every map pixel's
                     dF/F bytes, summed over bins of (2 --waves-bin + 1)^2 pixels (default 2), are followed on the device from a
                     baseline of --waves-pre frames (8) that ends --waves-lead frames (8) before the trigger to their maximum
                     within --waves-post frames (24) after it; the latency is the sub-frame time of half that rise, kept where
                     the rise is at least --waves-min-rise grey levels (8).  wave_triggers, wave_trigger_ens (events);
                     wave_lat_mean, wave_lat_sd (ensembles x H x W, frames after the trigger, float32), wave_count (uint32: the
                     events a pixel is valid in); wave_nodes (nodes x 2: column, row of a grid every --waves-step pixels, 8),
                     wave_velocity (ensembles x nodes x 2, pixels per frame: per node the median over the events of the plane
                     fit within --waves-fit pixels, 6), wave_speed (ensembles: its median length over the nodes),
                     wave_origin (ensembles x 2: column, row of the least mean latency; -1 none), wave_params: pre, lead,
                     post, bin, min_rise, step, fit, then half, q, floor, gain of the dF/F bytes.
    --waves-frames FILE   with --waves: the trigger frames of one ensemble from a text file of whole numbers (frames of the
                     record, 0 the first tracked frame) instead of the ensembles of --network.
    --waves-keep     with --waves: also wave_lat, wave_rise (events x H x W, int32), wave_why (uint8: 0 valid, 1 still rising at
                     the window's end, 2 rise too small, 3 at half height when the search starts, 255 off the map) and
                     wave_fit (events x nodes x 9, int64: the fit's sums).
    --waves-map OUT.png   with --waves: the mean latency of the ensemble with the most valid pixels, early blue to late red,
                     over the mean registered frame.
    --events-video OUT.avi   with --events: the event bytes min(255, floor(s + 0.5)) of every pixel and frame in the body
                     frame, grey (hydra_mi.events.event_video), through the writer of --dff-video.
    --pca K          with --rois or --demix: the K dominant modes of the kept registered video with nobody naming a cell
                     (hydra_mi.pca), from the Gram matrix of its frames made on the device's matrix cores; on the record as
                     it stands after --stabilize and --deform-correct, before anything else reads it.  pca_lambda, pca_share
                     (K): the eigenvalues of the video with every pixel's mean taken out, and their shares of its variance;
                     pca_temporal (frames x K): the temporal vectors; pca_rho (K x H x W): every component's correlation
                     image, rounded to float32 here; pca_frame_score (frames): per frame the median of Pearson's r over the
                     pixels with every other frame, low where the track slipped.  At most 8192 frames.
    --pca-frames     with --pca: also pca_frame_r (frames x frames, float32): Pearson's r of every two frames.
    --depth-range LO,HI   16-bit input (a uint16 .npy / .npz array, a TIFF stack of 16-bit gray pages; hydra_mi.deepio): the
                     window that becomes 0..255, given outright.
    --depth-percentiles LO_PPM,HI_PPM   16-bit input: the window from the histogram of every pixel of the recording,
                     made on the device: LO_PPM parts per million of the pixels lie below lo, at most 10^6 - HI_PPM above
                     hi (default 1000,999990).
    --depth-gamma G  16-bit input: the exponent of the table between lo and hi (default 1: linear, rounded half up).
                     optical_flow_ext.py takes the same three flags and resolves them through the same function, so the
                     tracker sees the frames its flow was computed on.  With the flow computed in-process the 16-bit
                     pixels themselves go to the GPU, 2 bytes a pixel, and the device maps them as they enter the frame
                     ring (deepio.DeepSource).  The states file gains depth_lo, depth_hi, depth_gamma and depth_clipped
                     (frames x 2: every frame's pixels below lo and above hi), and one warning line is printed when
                     more than ten times the share the window allows of some frame's pixels lie above hi.
    --deep-traces    16-bit input with --rois, --demix or --points: a second pass over the file once the track and the cells
                     are known (hydra_mi.deeptrace).  The 16-bit frames are uploaded again, only the body pixels of the ROIs,
                     rings and shapes are pulled back through the tracked mesh, and summed at full depth: deep_F_roi,
                     deep_F_np, deep_dff (frames x cells) by the expressions of roi_F, roi_Fnp, roi_dff, with --demix also
                     deep_demix_c; with --points alone deep_point_means.  Where the cells are stays the 8-bit pipeline's
                     decision.  Refused with 8-bit input, and with --stabilize or --deform-correct, which rewrite the kept
                     record in a way the second pass does not repeat.
    --deep-offset N  with --deep-traces: the camera's black level, subtracted from the means before dF/F (default 0).
"""
import argparse
import contextlib
import os
import sys

import numpy as np

import hydra_mi  # noqa: F401
from hydra_mi import (cellview, deepio, deeptrace, deform, demix, detrend, events, kalman, network, pca, residual, roi,
                      stabilize, strain, waves)
from hydra_mi.body import (BodyReadout, read_out, read_out_recorded, read_points_csv, record_bytes, write_points_csv,
                           write_points_txt)
from hydra_mi.distmesh_dyn import DistMesh
from hydra_mi.pipeline import FlowEKFPipeline, VideoStream
from hydra_mi.renderer import FlowStream
from hydra_mi.smooth import RTSSmoother, check_budget
from hydra_mi.videoio import AviWriter


def add_depth_arguments(parser):
    parser.add_argument("--depth-range", default=None, metavar="LO,HI", help="16-bit input: the window that becomes 0..255")
    parser.add_argument("--depth-percentiles", default=None, metavar="LO_PPM,HI_PPM",
                        help="16-bit input: the window from the recording's histogram, in parts per million (default %d,%d)"
                        % (deepio.DEFAULT_LO_PPM, deepio.DEFAULT_HI_PPM))
    parser.add_argument("--depth-gamma", default=None, metavar="G", help="16-bit input: the exponent of the table (default 1)")


def depth_of(args):
    """the ``depth`` of pipeline.load_video from the three flags (ValueError for a bad one)"""
    return deepio.depth_option(args.depth_range, args.depth_percentiles, args.depth_gamma)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("fn_in", default="./video/johntest_brightcontrast_short.npy", nargs="?",
                        help="input video file (.npy/.npz, frames x H x W[ x 3], uint8)")
    parser.add_argument("flow_in", default="./video/johntest_brightcontrast_short/flow", nargs="?",
                        help="input optic flow path")
    parser.add_argument("fn_out", default="./video/johntest_brightcontrast_short_output.npz", nargs="?",
                        help="output file (tracked states)")
    parser.add_argument("-n", "--name", default=None, nargs="?", const="johntest_brightcontrast_short",
                        help="name for saving run images (screenshots/<name>_frame_<k>_*.png; none without -n)")
    parser.add_argument("-t", "--threshold", default=9, type=int,
                        help="threshold intensity below which is background")
    parser.add_argument("-s", "--gridsize", default=22, type=int,
                        help="edge length for mesh (smaller is finer; unstable much further below 18)")
    parser.add_argument("-c", "--cuda", default=True, type=bool, help="whether or not to do analysis on the GPU")
    parser.add_argument("--registered", default=None, help="write the registered (body-frame) video here (.avi)")
    parser.add_argument("--points", default=None, help="points to track, CSV lines name,x,y in body coordinates")
    parser.add_argument("--point-radius", default=3.0, type=float, help="radius of the point discs read out (px)")
    parser.add_argument("--find-points", default=None, type=int, metavar="N",
                        help="find the N best cells from the statistics of the registered video and read them out")
    parser.add_argument("--find-radius", default=6, type=int, help="half width of the window a cell is the maximum of (1..16)")
    parser.add_argument("--find-score", default="corr", choices=("corr", "std", "range"), help="the summary image searched")
    parser.add_argument("--find-min-score", default=None, type=float, metavar="S", help="the least score of a point found")
    parser.add_argument("--find-more", default=None, type=int, metavar="ROUNDS",
                        help="rounds of looking for cells beside the found ones in the residual video of the demixed model "
                             "(implies --demix, needs --find-min-score)")
    parser.add_argument("--find-blank", default=residual.DEFAULT_BLANK, type=int, help="radius blanked round every known point (px)")
    parser.add_argument("--residual-video", default=None, metavar="OUT.avi",
                        help="write the registered video less the demixed cells here (.avi)")
    parser.add_argument("--points-out", default=None, help="write the points found here (CSV lines name,x,y)")
    parser.add_argument("--rois", action="store_true", help="footprints, ROIs and dF/F traces of the points (roi_* arrays)")
    parser.add_argument("--rois-max-gb", default=8.0, type=float, help="device memory the kept registered video may take (GiB)")
    parser.add_argument("--roi-thr", default=None, type=float, help="footprint threshold of an ROI (default %g)" % roi.DEFAULT_THR)
    parser.add_argument("--roi-alpha", default=0.7, type=float, help="share of the ring trace taken off the ROI trace")
    parser.add_argument("--demix", action="store_true", help="--rois, and overlapping cells demixed (demix_* arrays)")
    parser.add_argument("--demix-iters", default=6, type=int, help="rounds of shapes given traces, traces given shapes")
    parser.add_argument("--stabilize", action="store_true",
                        help="with --rois or --demix: stabilise the kept registered video before the cells are read out "
                             "(stab_* arrays); --cells-video keeps drawing at the tracked states")
    parser.add_argument("--stab-patch", default=16, type=int, help="edge of the patches that are matched (4..64 px)")
    parser.add_argument("--stab-search", default=3, type=int, help="the shifts searched: +-N px (0..8)")
    parser.add_argument("--stab-passes", default=1, type=int, help="passes of estimating the shifts")
    parser.add_argument("--stab-mode", default="patch", choices=stabilize.MODES,
                        help="patch: one whole-pixel shift per patch; field: a smooth sub-pixel shift field between the patch "
                             "centres (stab_q in the states file)")
    parser.add_argument("--deform-correct", action="store_true",
                        help="with --rois or --demix: correct the kept registered video for tissue compression before the cells "
                             "are read out (deform_* arrays)")
    parser.add_argument("--deform-gamma", default=None, type=float, metavar="G",
                        help="with --deform-correct: the exponent of brightness ~ J^-G (0..3) instead of the fitted one")
    parser.add_argument("--detrend", action="store_true",
                        help="with --find-points: find the cells in the excess video, every pixel less its running baseline "
                             "(detrend_* arrays)")
    parser.add_argument("--detrend-half", default=detrend.DEFAULT_HALF, type=int, help="frames either side of the baseline's window (0..1024)")
    parser.add_argument("--detrend-q", default=detrend.DEFAULT_Q, type=int, help="the baseline's percentile (0..100, a whole number)")
    parser.add_argument("--resummarize", action="store_true",
                        help="with --stabilize: the summary images of the stabilised record (detrend_* arrays), searched by --find-points")
    parser.add_argument("--dff-video", default=None, metavar="OUT.avi", help="write the dF/F video in the body frame here (.avi)")
    parser.add_argument("--dff-floor", default=detrend.DEFAULT_FLOOR, type=int, help="the least denominator of dF/F (1..255 grey levels)")
    parser.add_argument("--dff-gain", default=detrend.DEFAULT_GAIN, type=int, help="the byte dF/F = 1 becomes (1..65535)")
    parser.add_argument("--smooth", action="store_true", help="smooth the track backward: Xs, Xs_std in the states file")
    parser.add_argument("--smooth-max-gb", default=8.0, type=float, help="device memory the smoother may take (GiB)")
    parser.add_argument("--cells-video", default=None, metavar="OUT.avi",
                        help="after tracking, write the cells and tracked points painted onto the video (.avi); needs one "
                             "of --points, --find-points, --rois, --demix; one more pass over the frames of the input video")
    parser.add_argument("--cells-video-states", default=None, choices=("filtered", "smoothed"),
                        help="the states the cells video is drawn at (default: smoothed with --smooth, else filtered)")
    parser.add_argument("--strain", action="store_true", help="the deformation of every triangle, and of the tissue under every cell (strain_* arrays)")
    parser.add_argument("--strain-video", default=None, metavar="OUT.avi", help="after tracking, write the strain painted onto the video (.avi)")
    parser.add_argument("--strain-which", default="J", choices=strain.WHICH, help="what the strain video shows: area ratio or a principal stretch")
    parser.add_argument("--strain-gain", default=strain.DEFAULT_GAIN, type=float, help="colour levels per unit of (value - 1)")
    parser.add_argument("--strain-alpha", default=strain.DEFAULT_ALPHA, type=int, help="weight of the colour over the frame (0..255)")
    parser.add_argument("--network", action="store_true", help="with --rois or --demix: ensembles of co-active cells, their lags and maps (net_* arrays)")
    parser.add_argument("--network-thr", default=None, type=float, help="the least r at lag 0 that joins two cells (default %g)" % network.DEFAULT_THR)
    parser.add_argument("--network-lag", default=network.DEFAULT_LAG, type=int, help="the lags looked at: +-N frames")
    parser.add_argument("--network-map-thr", default=None, type=float,
                        help="the least rho that gives a pixel to an ensemble (default %g)" % network.DEFAULT_MAP_THR)
    parser.add_argument("--network-map", default=None, metavar="OUT.png", help="with --network: write the ensemble map here (.png)")
    parser.add_argument("--network-null", default=0, type=int, metavar="N",
                        help="with --network: significance against N circularly shifted traces (net_p_r, net_p_map, net_rho_max, net_sig, net_map_sig)")
    parser.add_argument("--network-alpha", default=0.05, type=float, help="with --network-null: the level a pixel is significant at")
    parser.add_argument("--network-guard", default=network.DEFAULT_LAG, type=int, help="with --network-null: no shift within N frames of 0")
    parser.add_argument("--pca", default=None, type=int, metavar="K",
                        help="with --rois or --demix: the K dominant modes of the kept registered video (pca_* arrays)")
    parser.add_argument("--pca-frames", action="store_true", help="with --pca: also pca_frame_r, Pearson's r of every two frames")
    parser.add_argument("--waves", action="store_true", help="with a kept record and --network or --waves-frames: latency maps, velocity and origin of every ensemble's events (wave_* arrays)")
    parser.add_argument("--waves-frames", default=None, metavar="FILE", help="with --waves: the trigger frames of one ensemble, a text file of whole numbers")
    parser.add_argument("--waves-pre", default=None, type=int, help="with --waves: frames of the baseline (default %d)" % waves.DEFAULT_PRE)
    parser.add_argument("--waves-lead", default=None, type=int, help="with --waves: frames before the trigger at which the search starts (default %d)" % waves.DEFAULT_LEAD)
    parser.add_argument("--waves-post", default=None, type=int, help="with --waves: frames after the trigger at which the search ends (default %d)" % waves.DEFAULT_POST)
    parser.add_argument("--waves-bin", default=None, type=int, help="with --waves: bins of (2 N + 1)^2 pixels (default %d)" % waves.DEFAULT_BIN)
    parser.add_argument("--waves-min-rise", default=None, type=int, help="with --waves: the least rise in grey levels (default %d)" % waves.DEFAULT_MIN_RISE)
    parser.add_argument("--waves-step", default=None, type=int, help="with --waves: a fit node every N pixels (default %d)" % waves.DEFAULT_STEP)
    parser.add_argument("--waves-fit", default=None, type=int, help="with --waves: the fit takes the pixels within N of a node (default %d)" % waves.DEFAULT_FIT)
    parser.add_argument("--waves-keep", action="store_true", help="with --waves: also the planes per event (wave_lat, wave_rise, wave_why, wave_fit)")
    parser.add_argument("--waves-map", default=None, metavar="OUT.png", help="with --waves: write the mean latency map here (.png)")
    parser.add_argument("--network-seed", default=0, type=int, help="with --network-null: the seed the shifts are drawn with")
    parser.add_argument("--events", action="store_true", help="with --rois or --demix: events behind the dF/F traces and per pixel (ev_* arrays)")
    parser.add_argument("--events-g", default=None, type=float, help="the decay per frame, 0 < g < 1 (default: estimated per cell)")
    parser.add_argument("--events-lambda", default=None, type=float, help="the penalty on the events (default: from each cell's noise)")
    parser.add_argument("--events-smin", default=None, type=float, help="the least event that counts (default: from each cell's noise)")
    parser.add_argument("--events-video", default=None, metavar="OUT.avi", help="with --events: write the event video in the body frame here (.avi)")
    parser.add_argument("--video-codec", default="raw", choices=("raw", "mjpeg"), help="the codec of every video written (default raw)")
    parser.add_argument("--video-quality", default=90, type=int, help="with --video-codec mjpeg: JPEG quality 1..100 (default 90)")
    add_depth_arguments(parser)
    parser.add_argument("--deep-traces", action="store_true",
                        help="16-bit input with --rois, --demix or --points: the cells' traces read again from the 16-bit frames (deep_* arrays)")
    parser.add_argument("--deep-offset", type=float, default=0.0, metavar="N",
                        help="with --deep-traces: the camera's black level, subtracted from the means (default 0)")
    return parser


def check_args(parser, args):
    """Every refusal that needs no file, in this order (where two apply, the first is the one the user reads), and the
    implications: --find-more implies --demix implies --rois.  -> the derived options, the keywords of Run."""
    try:
        depth = depth_of(args)
    except ValueError as exc:
        parser.error(str(exc))
    if not 1 <= args.video_quality <= 100:
        parser.error("--video-quality is 1..100")
    # (raw: the writers are called exactly as before)
    vopts = dict(codec="mjpeg", quality=args.video_quality) if args.video_codec == "mjpeg" else {}
    vkw = dict(video_opts=vopts) if vopts else {}
    gopts = dict(vopts, channels=1) if vopts else {}
    if not 0 <= args.strain_alpha <= 255 or not np.isfinite(args.strain_gain):
        parser.error("the strain video needs a --strain-alpha in 0..255 and a finite --strain-gain")
    if args.cells_video is not None and args.points is None and args.find_points is None:
        parser.error("--cells-video draws cells or points: it needs one of --points, --find-points, --rois, --demix")
    if args.cells_video_states is not None and args.cells_video is None:
        parser.error("--cells-video-states goes with --cells-video")
    if args.cells_video_states == "smoothed" and not args.smooth:
        parser.error("--cells-video-states smoothed needs --smooth")
    if args.find_points is not None:
        if args.points is not None:
            parser.error("--find-points finds the points itself: not together with --points")
        if args.find_points < 1 or not 1 <= args.find_radius <= 16:
            parser.error("--find-points needs N >= 1 and a --find-radius in 1..16")
    elif args.points_out is not None:
        parser.error("--points-out goes with --find-points")
    if args.find_min_score is not None and (args.find_points is None or not np.isfinite(args.find_min_score)):
        parser.error("--find-min-score is the least score of --find-points: it needs --find-points and a finite number")
    if args.find_more is not None:
        if args.find_points is None or args.find_min_score is None:
            parser.error("--find-more looks beside the points found: it needs --find-points and --find-min-score")
        if args.find_more < 1 or args.find_blank < 0:
            parser.error("--find-more needs at least one round and a --find-blank >= 0")
        args.demix = True
    if args.residual_video is not None and not args.demix:
        parser.error("--residual-video shows what the demixed model leaves: it needs --demix or --find-more")
    if args.demix:
        args.rois = True
        if args.demix_iters < 1:
            parser.error("--demix-iters needs at least one round")
    if args.rois and args.find_points is None and args.points is None:
        parser.error("--rois reads cells out: it needs --find-points or --points")
    if args.events and not args.rois:
        parser.error("--events reads the cells' traces: it needs --rois or --demix")
    if args.events_video is not None and not args.events:
        parser.error("--events-video shows the events: it needs --events")
    if args.events:
        if args.events_g is not None and not 0.0 < args.events_g < 1.0:
            parser.error("--events-g must lie inside 0 < g < 1")
        if any(v is not None and not (np.isfinite(v) and v >= 0.0) for v in (args.events_lambda, args.events_smin)):
            parser.error("--events-lambda and --events-smin must be finite and >= 0")
    if args.network and not args.rois:
        parser.error("--network reads the cells' traces: it needs --rois or --demix")
    if args.network_map is not None and not args.network:
        parser.error("--network-map draws the ensembles: it needs --network")
    if args.network and (args.network_lag < 0 or any(t is not None and not np.isfinite(t) for t in (args.network_thr, args.network_map_thr))):
        parser.error("--network needs a --network-lag >= 0 and finite thresholds")
    if args.network_null and not args.network:
        parser.error("--network-null tests the ensembles' maps: it needs --network")
    if args.network_null < 0 or args.network_guard < 0 or not 0.0 < args.network_alpha <= 1.0:
        parser.error("--network-null and --network-guard must be >= 0 and --network-alpha in (0, 1]")
    if args.detrend and args.find_points is None:
        parser.error("--detrend finds the cells in the excess video: it needs --find-points")
    if args.resummarize and (not args.stabilize or args.detrend):
        parser.error("--resummarize sums the stabilised record up: it needs --stabilize, and not --detrend")
    keep_record = args.detrend or args.resummarize or args.dff_video is not None
    check_waves_args(parser, args, keep_record)
    if (keep_record or args.events or args.waves) and not (0 <= args.detrend_half <= 1024 and 0 <= args.detrend_q <= 100 and 1 <= args.dff_floor <= 255
                            and 1 <= args.dff_gain <= 65535):
        parser.error("the running baseline needs a --detrend-half in 0..1024, a --detrend-q in 0..100, a --dff-floor in 1..255 "
                     "and a --dff-gain in 1..65535")
    if args.stabilize:
        if not (args.rois or keep_record):
            parser.error("--stabilize works on the kept record: it needs --rois or --demix")
        if not (4 <= args.stab_patch <= 64 and 0 <= args.stab_search <= 8 and args.stab_passes >= 1):
            parser.error("--stabilize needs a --stab-patch in 4..64, a --stab-search in 0..8 and at least one pass")
    if args.deform_correct and not (args.rois or keep_record):
        parser.error("--deform-correct works on the kept record: it needs --rois or --demix")
    if args.deform_gamma is not None and not (args.deform_correct and 0.0 <= args.deform_gamma <= deform.GAMMA_MAX):
        parser.error("--deform-gamma needs --deform-correct and an exponent in 0..%g" % deform.GAMMA_MAX)
    if args.pca is not None:
        if not (args.rois or keep_record):
            parser.error("--pca reads the kept record: it needs --rois or --demix")
        if args.pca < 1:
            parser.error("--pca needs at least one component")
    if args.pca_frames and args.pca is None:
        parser.error("--pca-frames adds the frame similarity: it needs --pca")
    if args.deep_traces:
        if not (args.rois or args.points is not None):
            parser.error("--deep-traces reads cells out of the 16-bit frames: it needs --rois, --demix or --points")
        if args.stabilize:
            parser.error("--deep-traces reads the frames as they were tracked: --stabilize rewrites the kept record, and the "
                         "second pass does not repeat that")
        if args.deform_correct:
            parser.error("--deep-traces reads the frames as they were tracked: --deform-correct rewrites the kept record, and the "
                         "second pass does not repeat that")
        if not np.isfinite(args.deep_offset):
            parser.error("--deep-offset needs a finite number")
    elif args.deep_offset != 0.0:
        parser.error("--deep-offset goes with --deep-traces")
    return dict(depth=depth, vopts=vopts, vkw=vkw, gopts=gopts, keep_record=keep_record)


WAVES_OPTIONS = (("waves_pre", "pre", waves.DEFAULT_PRE, 1, waves.PRE_MAX), ("waves_lead", "lead", waves.DEFAULT_LEAD, 0, waves.LEAD_MAX),
                 ("waves_post", "post", waves.DEFAULT_POST, 1, waves.POST_MAX), ("waves_bin", "b", waves.DEFAULT_BIN, 0, waves.B_MAX),
                 ("waves_min_rise", "min_rise", waves.DEFAULT_MIN_RISE, 1, 255), ("waves_step", "step", waves.DEFAULT_STEP, 1, waves.STEP_MAX),
                 ("waves_fit", "Rf", waves.DEFAULT_FIT, 1, waves.RF_MAX))


def read_trigger_frames(path):
    """The file of --waves-frames: whole numbers separated by white space -> int64 array; ValueError says what is wrong"""
    try:
        with open(path) as f:
            words = f.read().split()
    except OSError as exc:
        raise ValueError("--waves-frames %s cannot be read: %s" % (path, exc.strerror))
    try:
        return np.array([int(w) for w in words], np.int64)
    except ValueError:
        raise ValueError("--waves-frames %s holds something that is no whole number" % path)


def check_waves_args(parser, args, keep_record):
    """The refusals of --waves and its options, in check_args' style and order: an option without --waves, --waves without a
    kept record, --waves without triggers, a number out of range, a file of trigger frames that cannot be read (it is read
    here, into args.waves_trigger_frames, before anything is tracked).  Then the defaults are filled in."""
    flag = lambda name: "--" + name.replace("_", "-")
    given = [flag(n) for n in ("waves_frames", "waves_map") + tuple(o[0] for o in WAVES_OPTIONS) if getattr(args, n) is not None]
    given += ["--waves-keep"] if args.waves_keep else []
    message = None
    if given and not args.waves:
        message = "%s goes with --waves" % given[0]
    elif args.waves and not (args.rois or keep_record):
        message = "--waves works on the kept record: it needs --rois or --demix"
    elif args.waves and not (args.network or args.waves_frames is not None):
        message = "--waves needs trigger frames: the ensembles of --network or a file of them (--waves-frames)"
    elif args.waves:
        for name, _, _, lo, hi in WAVES_OPTIONS:
            v = getattr(args, name)
            if v is not None and not lo <= v <= hi:
                message = "%s %d outside %d..%d" % (flag(name), v, lo, hi)
                break
        args.waves_trigger_frames = None
        if message is None and args.waves_frames is not None:
            try:
                args.waves_trigger_frames = read_trigger_frames(args.waves_frames)
            except ValueError as exc:
                message = str(exc)
    if message is not None:
        parser.error(message)
    for name, _, default, _, _ in WAVES_OPTIONS:
        if getattr(args, name) is None:
            setattr(args, name, default)


class Run:
    """One run of the command: what every stage takes and fills (DESIGN.md §26 says which stage sets what)."""

    def __init__(self, parser, args, depth, vopts, vkw, gopts, keep_record):
        self.parser, self.args, self.depth = parser, args, depth
        self.vopts, self.vkw, self.gopts, self.keep_record = vopts, vkw, gopts, keep_record
        self.find = args.find_points is not None
        self.deep = self.deep_stack = self.video = self.reg_video = self.points = self.kf = self.body = self.sm = None
        self.states, self.errors, self.extra = [], [], {}       # extra: the arrays of the states file after X, err, p, t
        self.found = self.scores = self.more = self.e = None    # the points found, their scores, what --find-more found, the cells
        self.inside = []                                        # the indices of the points inside the mesh: cell s is point inside[s]
        self.cv_cells = self.cv_levels = self.cv_points = None  # what --cells-video draws when there are cells
        self.st_cells = self.st_dff = None                      # what --strain reads the tissue under: the cells' labels, their dF/F

    kept = property(lambda self: self.body is not None and self.body.keep)      # the registered video is kept on the device
    record_ready = property(lambda self: self.kept and len(self.states) > 0)    # ... and holds a frame
    pts = property(lambda self: self.found if self.find else self.points)       # the points found, else those given, else None
    dff = property(lambda self: self.e["dff_demixed"] if self.args.demix else self.e["dff"])    # the cells' dF/F, frames x cells
    tracked_frames = property(lambda self: self.capture.frames[1:1 + len(self.states)])         # state k: frame k + 1

    @contextlib.contextmanager
    def second_pass(self):
        """the 16-bit frames of the input once more (--deep-traces); a TIFF stack is closed after it"""
        src16 = deepio.open_deep(self.args.fn_in)
        try:
            yield src16
        finally:
            if isinstance(src16, deepio.TiffStack):
                src16.close()

    def keep_points(self, res):
        """a disc read-out of the points: into the states file and <fn_out>_points.txt"""
        self.extra.update(points=res["points"], point_means=res["point_means"], point_counts=res["point_counts"])
        fn_pts = os.path.splitext(self.args.fn_out)[0] + "_points.txt"
        write_points_txt(fn_pts, res["points"])
        print("Tracked points: %s" % fn_pts)


def open_input(run, args):
    """The input, the mesh on its first frame, the flow files, the writers; and the four refusals that need the input."""
    parser = run.parser
    deep = run.deep = deepio.load_deep(args.fn_in, run.depth)  # 16-bit input: mapped through its window; None for 8-bit
    if args.deep_traces and deep is None:
        parser.error("--deep-traces reads 16-bit frames: %s holds none (8-bit input has no more depth than the kept record)"
                     % args.fn_in)
    if deep is not None:                                       # (deep_stack: the mapped file behind it, which DeepSource reads)
        run.deep_stack = deep["source"] if isinstance(deep["source"], deepio.TiffStack) else None
        if not 0 <= args.threshold <= 255:                     # (the device compares on the 8-bit scale and refuses others)
            if run.deep_stack is not None:
                run.deep_stack.close()
            parser.error("-t/--threshold %d: with 16-bit input the threshold lies in 0..255, the scale of the mapped frames"
                         % args.threshold)
        print("16-bit input: window %d..%d (gamma %g) becomes 0..255; %d pixels below it, %d above"
              % (deep["lo"], deep["hi"], deep["gamma"], int(deep["clipped"][:, 0].sum()), int(deep["clipped"][:, 1].sum())))
        warn = deepio.clip_warning(deep["clipped"], deep["frames"].shape[1] * deep["frames"].shape[2], deep["hi_ppm"])
        if warn:
            print(warn)
        run.extra.update(depth_lo=np.int32(deep["lo"]), depth_hi=np.int32(deep["hi"]), depth_gamma=np.float64(deep["gamma"]),
                         depth_clipped=deep["clipped"])
    capture = run.capture = VideoStream(args.fn_in if deep is None else deep["frames"], args.threshold)  # reference run_kalmanfilter.py:58
    frame = run.frame = capture.current_frame()
    if args.pca is not None:                                   # before any tracking
        n_rec = capture.frames.shape[0] - 1
        if n_rec > pca.GRAM_MAX:
            parser.error("--pca: a record of %d frames, one Gram matrix takes %d at the most" % (n_rec, pca.GRAM_MAX))
        if args.pca > n_rec - 1:
            parser.error("--pca: %d components of %d frames (need 1..%d)" % (args.pca, n_rec, n_rec - 1))
    mask, ctrs, fd = capture.backsub()
    run.distmesh = DistMesh(frame, h0=args.gridsize)           # reference run_kalmanfilter.py:62-63
    run.distmesh.createMesh(ctrs, fd, frame, plot=False)
    run.smooth_budget, run.smooth_frames = int(args.smooth_max_gb * (1 << 30)), 2
    if args.smooth:
        run.smooth_frames = max(capture.frames.shape[0] - 1, 2)                  # one record per compute(), frames 1 .. F-1
        check_budget(run.distmesh.size(), run.smooth_frames, run.smooth_budget)  # before any tracking
    run.flowstream = FlowStream(args.flow_in)
    run.flow_ready, run.flowframe = run.flowstream.peek()
    H, W = frame.shape[:2]
    run.video = AviWriter(args.fn_out, W, H, **run.vopts) if args.fn_out.lower().endswith(".avi") else None
    if args.name is not None:
        os.makedirs("screenshots", exist_ok=True)
    run.points = read_points_csv(args.points)[1] if args.points is not None else None
    run.reg_video = AviWriter(args.registered, W, H, **run.gopts) if args.registered is not None else None


def make_body(run, args):
    """The body-frame readout, None when no flag asks for one; a record beyond --rois-max-gb is said to be so and not kept."""
    points = run.points
    if not (args.registered is not None or points is not None or run.find or run.keep_record):
        return None
    keep, budget = args.rois or run.keep_record, int(args.rois_max_gb * (1 << 30))
    if keep:
        need = record_bytes(run.kf.state.renderer.body_map()[0], max(run.capture.frames.shape[0] - 1, 1))
        if need > budget:
            print("The registered video takes %d bytes on the device, --rois-max-gb allows %d: no ROIs, %sthe disc read-out instead" % (
                need, budget, ("no stabilisation, " if args.stabilize else "") + ("no deformation correction, " if args.deform_correct else "")))
            if run.keep_record:
                print("No running baseline either: no --detrend, --resummarize or --dff-video")
            keep = False
    body = BodyReadout(run.kf, points=points, point_radius=args.point_radius, video=run.reg_video, stats=run.find, keep=keep, keep_bytes=budget)
    for i in np.flatnonzero(body.outside):
        print("Warning: point %d (%g, %g) lies outside the mesh: NaN in every frame" % (i, points[i, 0], points[i, 1]))
    return body


def make_smoother(run, args):
    return RTSSmoother(run.kf, run.smooth_frames, covariances=True, max_bytes=run.smooth_budget) if args.smooth else None


def keep_state(run, e, count):
    run.states.append(run.kf.state.X.reshape(-1).copy())
    run.errors.append([float(e[0]), float(e[1]), float(e[2]), float(e[3])])
    if run.args.name is not None:                              # reference :89, imageoutput of compute()
        run.kf.screenshots("screenshots/%s_frame_%d" % (run.args.name, count))


def track_from_flow_files(run, args):
    """the reference's loop (:78-89): one flow file per frame"""
    capture = run.capture
    if run.deep_stack is not None:
        run.deep_stack.close()                                 # (the mapped frames are all this loop reads)
    kf = run.kf = kalman.IteratedMSKalmanFilter(run.distmesh, run.frame, run.flowframe, cuda=args.cuda, sparse=True, multi=True)
    body = run.body = make_body(run, args)
    sm = run.sm = make_smoother(run, args)
    count = 0
    while capture.isOpened():
        count += 1
        ret, _, grayframe, m = capture.read()
        ret_flow, flowframe = run.flowstream.read()
        if ret is False or ret_flow is False:
            break
        print("Frame %d" % count)
        keep_state(run, kf.compute(grayframe, flowframe, m), count)
        if sm is not None:
            sm.record()
        if run.video is not None:
            run.video.write(kf.state.renderer.view(kf.state.X, "overlay"))
        if body is not None:
            body.frame(kf.state.X, capture.frame)              # the raw frame, as the pipeline reads it


def track_in_process(run, args):
    """no flow files: flow and filter in one process, the flow of the coming frames computed on the GPU beside the filter
    (hydra_mi.pipeline; replaces the file hand-off of reference README.md:26-31)"""
    capture, deep = run.capture, run.deep
    print("Cannot read flow stream at %s*: computing Brox flow in-process" % args.flow_in)
    run.kf = kalman.IteratedMSKalmanFilter(run.distmesh, run.frame, np.zeros(run.frame.shape + (2,), np.float32), cuda=args.cuda,
                                           sparse=True, multi=True)
    source = capture                                 # frames, masks and background-subtracted frames read from the stream
    if str(args.fn_in).lower().endswith(".avi"):
        from hydra_mi.videoio import AviReader, AviSource
        with AviReader(args.fn_in) as reader:
            mjpeg = reader.mjpeg
        if mjpeg:                                    # the device decoder writes the frame ring's planes
            source = AviSource(args.fn_in, args.threshold, frames=capture.frames)
    if deep is not None:                             # the device maps the 16-bit pixels into the frame ring's planes
        source = deepio.DeepSource(deep["source"], deep["lut"], deep["lo"], deep["hi"], args.threshold, frames=capture.frames)
    pipe = None
    try:
        pipe = FlowEKFPipeline(run.kf, source)
        run.body, run.sm = make_body(run, args), make_smoother(run, args)

        def on_frame(k, e):
            print("Frame %d" % (k + 1))
            keep_state(run, e, k + 1)
        pipe.run(on_frame=on_frame, video=run.video, body=run.body, smoother=run.sm)
    finally:                                         # also when tracking fails: the pipeline first, then what fed it
        if pipe is not None:
            pipe.close()
        if source is not capture:
            source.close()
        if run.deep_stack is not None:
            run.deep_stack.close()


def stage_results(run, args):
    body, extra = run.body, run.extra
    if run.video is not None:
        run.video.close()
        print("Overlay video: %d frames in %s" % (run.video.frames, args.fn_out))
    if body is None:
        return
    res = body.results()
    extra.update(tri_means=res["tri_means"], tri_counts=res["tri_counts"])       # (beside depth_* of a 16-bit input)
    if run.points is None:
        return
    run.keep_points(res)
    # the discs of the points, read from the 16-bit frames (with ROIs the cells' traces are read instead, in stage_cells)
    if args.deep_traces and not (args.rois and body.keep) and body.L > 0 and len(run.states):
        with run.second_pass() as src16:
            dsum = deeptrace.run(body, src16, run.states, deeptrace.columns(body.labels, body.L), first=1)   # (state k: frame k + 1)
        extra.update(deep_point_means=deeptrace.point_means(dsum, body.label_counts, args.deep_offset), deep_offset=np.float64(args.deep_offset))
        print("Full-depth traces: the discs of %d points over %d frames" % (body.L, len(run.states)))


def stage_stabilize(run, args):
    if not (args.stabilize and run.record_ready):
        return
    est = stabilize.stabilize(run.body, B=args.stab_patch, S=args.stab_search, passes=args.stab_passes, mode=args.stab_mode)
    run.extra.update(stab_shifts=est["shifts"], stab_score=est["score"], stab_fallback=est["fallback"])
    moved = est["shifts"].astype(np.float64)
    if args.stab_mode == "field":
        run.extra.update(stab_q=est["q"])
        moved = est["q"].astype(np.float64) / 16.0
    print("Stabilised%s: %d patches of %d px, search %d, %d passes: %.1f %% fallbacks, mean |shift| %.3f px" % (
        " (field)" if args.stab_mode == "field" else "", est["shifts"].shape[1], args.stab_patch, args.stab_search,
        args.stab_passes, 100.0 * est["fallback"].mean(), np.abs(moved).sum(2).mean()))


def stage_deform_correct(run, args):
    if not (args.deform_correct and run.record_ready):
        return
    dc = deform.correct(run.body, np.array(run.states), gamma=args.deform_gamma)        # at the filtered states: the frames were warped with them
    run.extra.update(deform_gamma=np.float64(dc["gamma"]), deform_fit_r2=np.float64(dc["fit_r2"]), deform_gain=dc["gain"],
                     deform_clipped=np.uint64(dc["clipped"]), deform_r_before=dc["r_before"].astype(np.float32),
                     deform_r_after=dc["r_after"].astype(np.float32))
    with np.errstate(invalid="ignore"):
        med = [float(np.nanmedian(np.abs(dc[key]))) if np.isfinite(dc[key]).any() else np.nan for key in ("r_before", "r_after")]
    print("Deformation corrected: gamma %.3f (%s, r2 %.3f), gains %.3f .. %.3f over %d triangles, %d values clipped, "
          "median |r| with the area change %.3f -> %.3f" % (
              dc["gamma"], "fitted" if dc["fitted"] else "given" if args.deform_gamma is not None else "nothing to fit from",
              dc["fit_r2"], dc["gain"].min() / 4096.0, dc["gain"].max() / 4096.0, dc["gain"].shape[1], dc["clipped"], *med))


def stage_pca(run, args):
    if not (args.pca is not None and run.record_ready):
        return
    pc = pca.pca(run.body, min(args.pca, max(len(run.states) - 1, 1)), frames=args.pca_frames)      # (a run that ended early)
    run.extra.update(pca_lambda=pc["lam"], pca_share=pc["share"], pca_temporal=pc["temporal"], pca_rho=pc["rho"].astype(np.float32),
                     pca_frame_score=pc["frame_score"])
    if args.pca_frames:
        run.extra.update(pca_frame_r=pc["frame_r"].astype(np.float32))
    print("PCA: %d components of %d frames carry %s of the variance; lowest frame score %.3f at frame %d" % (
        len(pc["lam"]), len(run.states), " ".join("%.4f" % v for v in pc["share"]),
        np.nanmin(pc["frame_score"]) if np.isfinite(pc["frame_score"]).any() else np.nan,
        int(np.nanargmin(pc["frame_score"])) + 1 if np.isfinite(pc["frame_score"]).any() else -1))


def detrended_summary(run, args, kind):
    """the statistics begun afresh on the device and fed the kept record's planes: find_points searches these"""
    d_img = detrend.summary(run.body, kind, args.detrend_half, args.detrend_q)
    run.extra.update(detrend_mean=d_img["mean"], detrend_std=d_img["std"], detrend_max=d_img["max"], detrend_corr=d_img["corr"])
    if kind == "excess":
        print("Detrended: the excess over the running baseline (half %d, q %d) of %d frames summed up" % (
            args.detrend_half, args.detrend_q, d_img["frames"]))
    else:
        print("Resummarised: %d frames of the stabilised record summed up" % d_img["frames"])


def search_more(run, args, found, scores):
    """the cells beside the ones found: the demixed model taken out of the kept record, and searched again"""
    more = run.more = residual.find_more(run.body, found, args.find_min_score, rounds=args.find_more, radius=args.find_radius,
                                         score=args.find_score, blank=args.find_blank, iters=args.demix_iters,
                                         r_disc=args.point_radius, thr=args.roi_thr, alpha=args.roi_alpha)
    rs = more["scores"]
    run.extra.update(residual_round=more["round"], residual_scores=np.concatenate(rs),
                     residual_scores_round=np.concatenate([np.full(len(s), k + 1, np.int32) for k, s in enumerate(rs)]),
                     residual_clipped=np.array(more["clipped"], np.uint64))
    print("Found %d more points in %d rounds of the residual video (%d candidates refused, %d values clipped)" % (
        len(more["points"]) - len(found), len(rs), len(more["refused"]), sum(more["clipped"])))
    return more["points"], np.concatenate((scores, more["new_scores"]))


def stage_search(run, args):
    """The summary images of --detrend or --resummarize, and with --find-points the search: the cells need the whole video
    and the traces need the cells, so a second pass over the recorded states reads them out."""
    body = run.body
    kind = ("excess" if args.detrend else "recorded" if args.resummarize else None) if run.record_ready else None
    if not run.find:
        if kind is not None:
            detrended_summary(run, args, kind)
            run.kf.state.renderer.body_stats_end()
        return
    sm_img = body.summary()
    if kind is not None:
        detrended_summary(run, args, kind)
    found, scores = body.find_points(args.find_points, radius=args.find_radius, score=args.find_score, min_score=args.find_min_score)
    if args.find_more is not None and run.record_ready and len(found):
        found, scores = search_more(run, args, found, scores)
    run.found, run.scores = found, scores
    run.kf.state.renderer.body_stats_end()
    run.extra.update(body_mean=sm_img["mean"], body_std=sm_img["std"], body_max=sm_img["max"], body_corr=sm_img["corr"],
                     found_points=found, found_scores=scores)
    print("Found %d points (%s, radius %d) in %d frames" % (len(found), args.find_score, args.find_radius, sm_img["frames"]))
    if body.keep:                # the registered video is on the device: the discs are summed there
        res = read_out_recorded(body, run.states, found, args.point_radius)
    else:
        res = read_out(run.kf, run.states, run.tracked_frames, found, args.point_radius)
    run.keep_points(res)
    if args.points_out is not None:
        write_points_csv(args.points_out, found)
        print("Points found: %s" % args.points_out)


def stage_cells(run, args):
    """The dF/F video; the cells of the points inside the mesh, demixed (those of --find-more reused when they are all the
    points) or ROIs; the residual video; the roi_* arrays; the same cells at full depth."""
    body, extra, pts = run.body, run.extra, run.pts
    if not run.kept:
        return
    if args.dff_video is not None and len(run.states):
        n_dff = detrend.write_video(body, args.dff_video, args.detrend_half, args.detrend_q, args.dff_floor, args.dff_gain, **run.vkw)
        print("dF/F video: %d frames in %s" % (n_dff, args.dff_video))
    inside = run.inside = np.flatnonzero(body.locate(pts)[0] >= 0) if args.rois else []
    if not (len(inside) and len(run.states)):
        return
    cell = dict(r_disc=args.point_radius, thr=args.roi_thr, alpha=args.roi_alpha)
    if args.demix:
        if run.more is not None and len(inside) == len(pts):           # (demixed already, with all the points)
            e = run.more["e"]
        else:
            e = demix.extract(body, pts[inside], iters=args.demix_iters, **cell)
        extra.update(demix_shapes=e["shapes"], demix_C=e["C"], demix_dff=e["dff_demixed"], demix_change=e["demix_change"])
        print("Demixed: %d cells, %d rounds, last change %.3g" % (len(inside), args.demix_iters, e["demix_change"][-1]))
        if args.residual_video is not None:
            n_res, n_clip = residual.write_video(body, args.residual_video, e, points=pts[inside], **run.vkw)
            print("Residual video: %d frames in %s (%d values clipped)" % (n_res, args.residual_video, n_clip))
    else:
        e = roi.extract(body, pts[inside], **cell)
    run.e = e
    extra.update(roi_points=inside, roi_footprints=e["footprints"], roi_labels=e["roi_labels"], roi_counts=e["roi_counts"],
                 roi_ring_counts=e["ring_counts"], roi_F=e["F_roi"], roi_Fnp=e["F_np"], roi_dff=e["dff"], roi_seed_fallback=e["seed_fallback"])
    print("ROIs: %d cells, %d..%d pixels, %d kept their disc" % (len(inside), e["roi_counts"].min(), e["roi_counts"].max(), e["seed_fallback"].sum()))
    if args.deep_traces:                                               # the second pass: the same cells, the camera's numbers
        with run.second_pass() as src16:
            de = deeptrace.extract(body, src16, run.states, e, demixed=e if args.demix else None, alpha=args.roi_alpha,
                                   offset=args.deep_offset, first=1)    # (state k belongs to frame k + 1)
        extra.update(deep_F_roi=de["deep_F_roi"], deep_F_np=de["deep_F_np"], deep_dff=de["deep_dff"], deep_offset=np.float64(args.deep_offset))
        if args.demix:
            extra.update(deep_demix_c=de["deep_demix_c"])
        print("Full-depth traces: %d cells over %d frames, F_roi %.1f..%.1f" % (
            len(inside), len(run.states), np.nanmin(de["deep_F_roi"]), np.nanmax(de["deep_F_roi"])))


def stage_events(run, args):
    body, extra = run.body, run.extra
    if run.e is None or not args.events:
        return
    tr = np.ascontiguousarray(run.dff.T, np.float64)
    fixed = lambda v, rule: np.full(len(tr), v, np.float64) if v is not None else np.array(rule, np.float64)
    sig = [events.noise(x) for x in tr]
    ev_g = fixed(args.events_g, [events.estimate_g(x) for x in tr])
    ev_lam = fixed(args.events_lambda, [events.default_lam(g, sg) for g, sg in zip(ev_g, sig)])
    ev_smin = fixed(args.events_smin, [events.default_smin(sg) for sg in sig])
    ev_c, ev_s = events.deconvolve(tr, ev_g, ev_lam)
    # every pixel of the dF/F bytes: one g, and the cells' median penalty and threshold in bytes
    px = dict(what="dff", half=args.detrend_half, q=args.detrend_q, floor=args.dff_floor, gain=args.dff_gain)
    g_px, lam_px = float(np.median(ev_g)), float(np.median(ev_lam)) * args.dff_gain
    smin_px = max(1.0, float(np.median(ev_smin)) * args.dff_gain)
    ev_n, ev_sum = events.count_image(body, g_px, lam_px, smin_px, **px)
    extra.update(ev_g=ev_g, ev_lambda=ev_lam, ev_c=ev_c, ev_s=ev_s, ev_binary=events.binarise(ev_s, ev_smin),
                 ev_count_image=ev_n, ev_sum_image=ev_sum.astype(np.float32),
                 ev_params=np.array([g_px, lam_px, smin_px, px["half"], px["q"], px["floor"], px["gain"]], np.float64))
    print("Events: %d cells, g %.3f..%.3f, %d events; per pixel g %.3f, lambda %.3g, s_min %.3g: %d events" % (
        len(tr), ev_g.min(), ev_g.max(), extra["ev_binary"].sum(), g_px, lam_px, smin_px, ev_n.sum()))
    if args.network:
        extra.update(net_r_events=network.coactivity(ev_s, args.network_lag))
    if args.events_video is not None:
        n_ev = events.event_video(body, args.events_video, g_px, lam_px, **px, **run.vkw)
        print("Event video: %d frames in %s" % (n_ev, args.events_video))


def stage_network(run, args):
    if run.e is None or not args.network:
        return
    net = network.extract(run.body, run.dff.T, thr=args.network_thr, max_lag=args.network_lag, map_thr=args.network_map_thr,
                          null=args.network_null, guard=args.network_guard, seed=args.network_seed, alpha=args.network_alpha)
    run.extra.update(net_r=net["r"], net_labels=net["labels"], net_ens_traces=net["ens_traces"], net_lead_lag=net["lead_lag"],
                     net_lead_r=net["lead_r"], net_rho=net["rho"].astype(np.float32), net_map=net["map"])
    print("Network: %d ensembles of %d cells, %d cells alone, %d pixels mapped" % (
        net["ens_traces"].shape[0], (net["labels"] >= 0).sum(), (net["labels"] < 0).sum(), (net["map"] >= 0).sum()))
    if args.network_null:
        run.extra.update(net_p_r=net["p_r"], net_p_map=net["p_map"].astype(np.float32), net_rho_max=net["rho_max"],
                         net_sig=net["sig"], net_map_sig=net["map_sig"])
        for k in range(net["rho_max"].shape[0]):
            print("Null: ensemble %d: the largest rho of %d shifted traces %.4f, %d significant pixels" % (
                k, net["rho_max"].shape[1], net["rho_max"][k].max(), net["sig"][k].sum()))
    if args.network_map is not None:
        network.colour_map(net["map_sig"] if args.network_null else net["map"], net["gray"], args.network_map)
        print("Ensemble map: %s" % args.network_map)


def stage_waves(run, args):
    if not args.waves:
        return
    if not run.record_ready:
        print("Waves: nothing read: the registered video was not kept, or no frame was tracked")
        return
    par = {key: getattr(args, name) for name, key, _, _, _ in WAVES_OPTIONS}
    win = {k: par[k] for k in ("pre", "lead", "post")}
    F = run.body.r.body_rec_count()
    if args.waves_frames is not None:
        t = args.waves_trigger_frames
        ok = waves.admissible(t, F=F, **win)
        if not ok.all():
            print("Waves: %d of %d trigger frames dropped: their windows leave the record of %d frames" % ((~ok).sum(), len(t), F))
        trig = [t[ok].astype(np.int32)]
    elif "net_ens_traces" in run.extra:
        trig = waves.triggers(run.extra["net_ens_traces"], F=F, **win)
    else:
        print("Waves: nothing read: there are no cells, so no ensembles")
        return
    px = dict(what="dff", half=args.detrend_half, q=args.detrend_q, floor=args.dff_floor, gain=args.dff_gain)
    w = waves.extract(run.body, trig=trig, keep=args.waves_keep, **px, **par)
    run.extra.update(wave_triggers=w["triggers"], wave_trigger_ens=w["trigger_ens"], wave_lat_mean=w["lat_mean"], wave_lat_sd=w["lat_sd"],
                     wave_count=w["count"], wave_nodes=w["nodes"], wave_velocity=w["velocity"], wave_speed=w["speed"],
                     wave_origin=w["origin"],
                     wave_params=np.array([par[k] for k in ("pre", "lead", "post", "b", "min_rise", "step", "Rf")]
                                          + [px[k] for k in ("half", "q", "floor", "gain")], np.float64))
    if args.waves_keep:
        run.extra.update(wave_lat=w["lat"], wave_rise=w["rise"], wave_why=w["why"], wave_fit=w["fit"])
    for k, t in enumerate(trig):
        print("Waves: ensemble %d: %d events, %.1f%% of their map pixels valid, origin (%d, %d), median speed %.3g px/frame" % (
            k, len(t), 100.0 * w["valid"][k], w["origin"][k, 0], w["origin"][k, 1], w["speed"][k]))
    if args.waves_map is not None:
        best = int(np.argmax((w["count"] > 0).sum((1, 2)))) if len(trig) else -1
        waves.colour_map(w["lat_mean"][best] if best >= 0 else np.full(w["gray"].shape, np.nan), w["gray"], args.waves_map)
        print("Wave map: %s" % args.waves_map)


def stage_record_end(run, args):
    """What --strain and --cells-video are handed of the cells; then the kept record is freed and the registered video closed."""
    e, n = run.e, len(run.inside)
    if e is not None and args.strain:
        run.st_cells, run.st_dff = {"labels": e["roi_labels"], "L": n}, run.dff
    if e is not None and args.cells_video is not None:
        if args.demix:
            lab, w, dropped = cellview.layers_from_shapes(e["shapes_q"], roi.seeds_of(run.pts[run.inside]),
                                                          (e["shapes_q"].shape[1] - 1) // 2, run.frame.shape[:2])
            if dropped:
                print("Cells video: %d (pixel, cell) entries beyond two cells per pixel are not drawn" % dropped)
            run.cv_cells, run.cv_levels = (lab, w), cellview.levels(e["dff_demixed"])
        else:
            run.cv_cells, run.cv_levels = cellview.layers_from_labels(e["roi_labels"]), cellview.levels(e["dff"])
        run.cv_points = run.pts[run.inside]                    # (cell s and marker s share a colour)
        if int(run.cv_cells[0].max()) + 1 != n:                # (the last cells own no pixel: no level for them)
            run.cv_levels = run.cv_levels[:, :int(run.cv_cells[0].max()) + 1]
    if run.kept:
        run.kf.state.renderer.body_rec_end()
    if run.reg_video is not None:
        run.reg_video.close()
        print("Registered video: %d frames in %s" % (run.reg_video.frames, args.registered))


def stage_smooth(run, args):
    sm = run.sm
    if sm is None:
        return
    if len(sm) > 0:
        xs, var = sm.run()
        run.extra.update(Xs=xs, Xs_std=np.sqrt(var))
    else:
        run.extra.update(Xs=np.zeros((0, 4 * run.kf.N)), Xs_std=np.zeros((0, 4 * run.kf.N)))
    sm.close()
    print("Smoothed track: Xs, Xs_std (%d frames)" % len(run.states))


def stage_cells_video(run, args):
    if args.cells_video is None or not len(run.states):
        return
    use = args.cells_video_states or ("smoothed" if args.smooth else "filtered")
    if run.cv_cells is not None and int(run.cv_cells[0].max()) < 0:
        run.cv_cells = run.cv_levels = None
    n_cv = cellview.write_video(run.kf, run.extra["Xs"] if use == "smoothed" else run.states, run.tracked_frames, args.cells_video,
                                cells=run.cv_cells, levels=run.cv_levels, points=run.pts if run.cv_points is None else run.cv_points, **run.vkw)
    print("Cells video: %d frames (%s states) in %s" % (n_cv, use, args.cells_video))


def stage_strain(run, args):
    extra = run.extra
    if not ((args.strain or args.strain_video is not None) and len(run.states)):
        return
    st_states = extra["Xs"] if args.smooth else np.array(run.states)
    if args.strain:
        d = strain.triangles(run.kf, st_states)
        extra.update(strain_J=d["J"], strain_l1=d["l1"], strain_l2=d["l2"], strain_axis=d["axis"], strain_rotation=d["rotation"],
                     strain_body_area=d["body_area"])
        print("Strain: %d triangles, body area %.4f .. %.4f of the rest area" % (d["J"].shape[1], np.nanmin(d["body_area"]), np.nanmax(d["body_area"])))
        if "net_ens_traces" in extra:
            extra.update(net_strain_r=network.strain_coupling(extra["net_ens_traces"], d["J"]))
        st_cells = run.st_cells                                # the cells' labels; without cells the discs of the points
        if st_cells is None and run.pts is not None:
            st_cells = {"points": run.pts, "point_radius": args.point_radius}
        if st_cells is not None and (len(st_cells["points"]) if "points" in st_cells else st_cells["L"]):
            c = strain.labels(run.kf, st_states, **st_cells)
            extra.update(strain_cell_J=c["J"], strain_cell_l1=c["l1"], strain_cell_l2=c["l2"])
            if run.st_dff is not None:
                extra.update(strain_artifact_r=strain.artifact_score(c["J"], run.st_dff))
    if args.strain_video is not None:
        n_sv = strain.write_video(run.kf, st_states, run.tracked_frames, args.strain_video, which=args.strain_which,
                                  gain=args.strain_gain, alpha=args.strain_alpha, **run.vkw)
        print("Strain video: %d frames (%s) in %s" % (n_sv, args.strain_which, args.strain_video))


def stage_save(run, args):
    if args.deep_traces and "deep_offset" not in run.extra:
        print("Full-depth traces: nothing read: no frame was tracked, no point lies inside the mesh, or the registered video "
              "did not fit and the points were found, not given")
    np.savez(args.fn_out, X=np.array(run.states), err=np.array(run.errors), p=run.distmesh.p, t=run.kf.state.tri, **run.extra)
    print("Finished: %d frames, states in %s" % (len(run.states), args.fn_out))


# The order is a contract: every stage says what it must come after, and why.  A new flag's stage goes where its inputs are
# ready and before whatever rewrites or frees them.
STAGES = (
    stage_results,          # after tracking: what was summed while it ran, first into the states file (beside depth_*)
    stage_stabilize,        # before every reader of the kept record: they see the stabilised frames; what was summed while tracking did not
    stage_deform_correct,   # after the stabiliser (it moves pixels across seams: the gain stays the home triangle's), before every other reader
    stage_pca,              # after both rewrites of the record, before anything else reads it
    stage_search,           # the record is final; ends the statistics (body_stats_end) once it has searched them
    stage_cells,            # after the search: it needs the points, and reuses the cells of --find-more
    stage_events,           # after the cells: their dF/F; before the network (ev_*, net_r_events, then net_*)
    stage_network,          # after the cells and the events
    stage_waves,            # after the network: the ensembles' traces give the triggers; the last reader of the kept record
    stage_record_end,       # after the last reader of the kept record: body_rec_end frees it; the readout is done with its writer
    stage_smooth,           # after the record is freed: the smoother's device memory; before what draws at Xs
    stage_cells_video,      # after the smoother: drawn at Xs with --smooth
    stage_strain,           # after the smoother (of Xs with --smooth) and the network (net_strain_r)
    stage_save,             # last: the --deep-traces notice when nothing was read, np.savez, the last line
)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    run = Run(parser, args, **check_args(parser, args))
    if len(sys.argv) == 1 and argv is None:
        print("No command line arguments provided, using defaults")
    open_input(run, args)
    (track_from_flow_files if run.flow_ready else track_in_process)(run, args)
    for stage in STAGES:
        stage(run, args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
