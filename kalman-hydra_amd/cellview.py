"""The cell overlay video: ROIs, demixed shapes and their activity painted onto the video, on the animal as it moves
(Renderer.view_set_cells / view_cells, include/hydra_mi.h: hm_view_cells).

The cells live in body coordinates, as hydra_mi.roi and hydra_mi.demix give them; the view looks up, per pixel of the
image at a tracked state, the body pixel under it and blends the colours of the cells there by weight x level:

    layers, weights, dropped = layers_from_shapes(e["shapes_q"], roi.seeds_of(points), R, (H, W))   # or layers_from_labels
    write_video(kf, states, source, "cells.avi", cells=(layers, weights), levels=levels(e["dff_demixed"]), points=points)
"""
import numpy as np

from . import body as _body
from .taps import write_painted_video

#: twelve B G R colours far apart in hue, none of them gray (the frame under them is)
_PALETTE = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [255, 0, 255], [255, 255, 0],
                     [0, 128, 255], [255, 128, 0], [128, 0, 255], [0, 255, 128], [255, 0, 128], [128, 255, 0]], np.uint8)


def palette(L):
    """(L, 3) uint8 B G R: a fixed table of distinct colours, cycled."""
    return _PALETTE[np.arange(int(L)) % len(_PALETTE)].copy()


def layers_from_labels(roi_labels):
    """A label image (H, W), -1: none -> (labels (1, H, W) int32, weights (1, H, W) uint16, 65535 everywhere)."""
    lab = np.ascontiguousarray(roi_labels, np.int32)[None]
    return lab, np.full(lab.shape, 65535, np.uint16)


def layers_from_shapes(shapes_q, seeds, R, shape, n_layers=2):
    """Shapes (P, 2R+1, 2R+1) uint16 in windows round the seeds (P, 2) (column, row), as hydra_mi.demix quantises them,
    -> (labels (n_layers, H, W) int32, weights (n_layers, H, W) uint16, dropped).  Per body pixel the cells whose window
    value there is > 0, in ascending cell index; the first n_layers are kept, one per layer, with that value as weight;
    dropped is the number of (pixel, cell) entries left out."""
    H, W = int(shape[0]), int(shape[1])
    n_layers, R = int(n_layers), int(R)
    if not 1 <= n_layers <= 4:
        raise ValueError("layers_from_shapes: n_layers %d outside 1..4" % n_layers)
    a = np.asarray(shapes_q)
    sd = np.asarray(seeds).reshape(-1, 2)
    S = 2 * R + 1
    if a.shape != (sd.shape[0], S, S):
        raise ValueError("shapes of shape %r for %d seeds and windows of %d x %d" % (a.shape, sd.shape[0], S, S))
    labels = np.full((n_layers, H, W), -1, np.int32)
    weights = np.zeros((n_layers, H, W), np.uint16)
    depth = np.zeros((H, W), np.int64)                  # cells seen so far per pixel
    dropped = 0
    for s in range(sd.shape[0]):
        c0, r0 = int(sd[s, 0]) - R, int(sd[s, 1]) - R
        ra, rb, ca, cb = max(r0, 0), min(r0 + S, H), max(c0, 0), min(c0 + S, W)
        if ra >= rb or ca >= cb:
            continue
        win = a[s, ra - r0:rb - r0, ca - c0:cb - c0]
        rr, cc = np.nonzero(win > 0)
        rr, cc = rr + ra, cc + ca
        d = depth[rr, cc]
        keep = d < n_layers
        labels[d[keep], rr[keep], cc[keep]] = s
        weights[d[keep], rr[keep], cc[keep]] = win[rr[keep] - ra, cc[keep] - ca]
        dropped += int((~keep).sum())
        depth[rr, cc] = d + 1
    return labels, weights, dropped


def levels(dff, lo=10.0, hi=99.0):
    """Traces (F, L) -> (F, L) uint8: per cell rint(255 clip((x - p_lo) / (p_hi - p_lo), 0, 1)), p_lo and p_hi the lo-th
    and hi-th percentile of the cell's finite values; 0 where p_hi == p_lo (or no value is finite), NaN -> 0."""
    x = np.asarray(dff, np.float64)
    x = x.reshape(x.shape[0], -1)
    out = np.zeros(x.shape, np.uint8)
    for s in range(x.shape[1]):
        v = x[:, s]
        ok = np.isfinite(v)
        if not ok.any():
            continue
        p_lo, p_hi = np.percentile(v[ok], [lo, hi])
        if not p_hi > p_lo:
            continue
        u = np.clip((np.where(ok, v, p_lo) - p_lo) / (p_hi - p_lo), 0.0, 1.0)
        out[:, s] = np.where(np.isnan(v), 0, np.rint(255.0 * u)).astype(np.uint8)
    return out


def write_video(kf_or_renderer, states, source, path, cells=None, levels=None, points=None, point_radius=2, outline=True,
                wire=False, fps=20, video_opts=None):
    """The overlay video of a finished track: frame k of `source` (``frame_at(k)`` -> raw frame, ...; or an array
    (frames, H, W) uint8) with the cells and markers at states[k], written to the AVI `path` (uncompressed; video_opts: AviWriter's codec
    options, e.g. dict(codec="mjpeg", quality=90)).

    cells: (labels, weights) as layers_from_* give them, or a label image (H, W); None: markers only.  levels: (F, L)
    uint8 (None: 255).  points: (P, 2) body coordinates, followed through the mesh (body.locate / body.track); each
    gets its palette colour.  The frames are uploaded one by one, the views queued on the tracker's stream into a ring of
    device slots and written by the writer thread of a taps.VideoTap: the disk is not waited for.  -> frames written."""
    r = _body.renderer_of(kf_or_renderer)
    F = len(states)
    if cells is None and points is None:
        raise ValueError("write_video: neither cells nor points to draw")
    L = 0
    if cells is not None:
        lab, w = cells if isinstance(cells, tuple) else layers_from_labels(cells)
        L = int(np.max(lab)) + 1
        if L < 1:
            raise ValueError("write_video: the label planes hold no cell")
        r.view_set_cells(lab, w, palette(L))
    else:
        r.view_set_cells(None)
    if levels is not None:
        levels = np.ascontiguousarray(levels, np.uint8)
        if levels.shape != (F, L):
            raise ValueError("levels of shape %r for %d states and %d cells" % (levels.shape, F, L))
    loc = colours = None
    if points is not None:
        pts = np.asarray(points, np.float64).reshape(-1, 2)
        t, ids, l1, l2 = _body.locate(r.uv, r.tri, pts)
        loc, colours = (ids, l1, l2, t >= 0), palette(pts.shape[0])

    def paint(k, X, d_frame, d_out, stream):
        p = None if loc is None else _body.track(X[:2 * r.n], *loc)
        r.view_cells_dev(X, d_frame, d_out, None if levels is None else levels[k], outline, wire, p, colours, point_radius,
                         stream)
    return write_painted_video(r, states, source, path, paint, fps, video_opts, done=lambda: r.view_set_cells(None))
