"""The tissue deformation readout: per-triangle stretch, a strain video, and the local area change under every cell
(Renderer.strain_tri / strain_labels / view_strain, include/hydra_mi.h: hm_strain_tri).

The tracker estimates a deforming mesh; on every triangle the map body -> frame is affine, and its gradient gives the area
ratio J, the principal stretches l1 >= l2, the axis of l1 in the body frame and the rotation:

    d = triangles(kf, states)                       # J, l1, l2, axis, rotation (frames x triangles), body_area (frames)
    c = labels(kf, states, points=points)           # J, l1, l2 under every cell (frames x cells)
    r = artifact_score(c["J"], dff)                 # a cell whose dF/F follows its tissue's area change is suspect
    write_video(kf, states, source, "strain.avi")   # J painted onto the animal, blue compressed, red stretched
"""
import numpy as np

from . import body as _body
from .taps import write_painted_video

WHICH = ("J", "l1", "l2")
DEFAULT_GAIN = 256.0        # levels per unit of (value - 1): 0.5 .. 1.5 fills the table
DEFAULT_ALPHA = 128


def default_lut():
    """(256, 3) uint8, B G R: blue (level 0, compressed) through white (128, unchanged) to red (255, stretched), linear
    in every channel either side of the middle."""
    lv = np.arange(256, dtype=np.float64)
    down = np.rint(255.0 * np.clip(lv / 128.0, 0.0, 1.0))                  # 0 at level 0, 255 from 128 on
    up = np.rint(255.0 * np.clip((255.0 - lv) / 127.0, 0.0, 1.0))          # 255 up to 128, 0 at level 255
    return np.stack((up, np.minimum(down, up), down), axis=1).astype(np.uint8)


def body_order(uv, tri):
    """The vertex ids (T, 3) of every triangle in the body map's order: i1 and i2 swapped where the triangle's area at
    the positions rint(256 uv) is negative (the render's orientation swap at X = uv)."""
    P = np.rint(np.asarray(uv, np.float32).astype(np.float64) * 256.0).astype(np.int64)
    ids = np.array(tri, np.int64).reshape(-1, 3)
    a, b, c = P[ids[:, 0]], P[ids[:, 1]], P[ids[:, 2]]
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    ids[area < 0] = ids[area < 0][:, [0, 2, 1]]
    return ids


def rest_area(uv, tri):
    """(T,) float64: the signed area of every triangle in body coordinates, d0 / 2 of hm_strain_tri."""
    U = np.asarray(uv, np.float32).astype(np.float64)
    ids = body_order(uv, tri)
    p, q = U[ids[:, 1]] - U[ids[:, 0]], U[ids[:, 2]] - U[ids[:, 0]]
    return (p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]) / 2.0


def triangles(kf_or_renderer, states):
    """The deformation of every triangle in every state (frames, 4N) -> dict: J (area ratio), l1 >= l2 (principal
    stretches), axis (radians in (-pi/2, pi/2]: the direction of l1 in the body frame), rotation (radians), each
    (frames, triangles), NaN for a triangle that is collapsed in the body frame or has a vertex that is not finite;
    area0 (triangles,) the rest areas; body_area (frames,) the area of the whole mesh over its rest area,
    sum |area0| J / sum |area0| over the triangles that are not NaN; n_bad (frames,) the number of those that are."""
    r = _body.renderer_of(kf_or_renderer)
    v = r.strain_tri(states)
    area0 = rest_area(r.uv, r.tri)
    J = v[:, :, 0]
    bad = np.isnan(J)
    w = np.where(bad, 0.0, np.abs(area0)[None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        body_area = (w * np.where(bad, 0.0, J)).sum(axis=1) / w.sum(axis=1)
    return {"J": J.copy(), "l1": v[:, :, 1].copy(), "l2": v[:, :, 2].copy(),
            "axis": 0.5 * np.arctan2(v[:, :, 4], v[:, :, 3]), "rotation": np.arctan2(v[:, :, 6], v[:, :, 5]),
            "area0": area0, "body_area": body_area, "n_bad": bad.sum(axis=1)}


def labels(kf_or_renderer, states, labels=None, points=None, point_radius=3.0, L=None):
    """The mean deformation under every cell -> dict: J, l1, l2 (frames, cells), counts (cells,) the body-map pixels of
    each.  The cells: a label image `labels` (H, W) in body coordinates (-1: none), or discs of point_radius px round
    `points` (P, 2) (body.disc_labels: a cell for every point, NaN for one off the mesh), or, with neither, the label
    image in place on the handle (Renderer.body_set_labels).  L: the number of cells of a label image whose last cells may
    own no pixel (default: its largest label + 1)."""
    r = _body.renderer_of(kf_or_renderer)
    if labels is not None and points is not None:
        raise ValueError("strain.labels: a label image or points, not both")
    if points is not None:
        pts = np.asarray(points, np.float64).reshape(-1, 2)
        lab, L = _body.disc_labels(r.body_map()[0], pts, point_radius), pts.shape[0]
    elif labels is not None:
        lab = np.ascontiguousarray(labels, np.int32)
        L = int(lab.max()) + 1 if L is None else int(L)
    else:
        lab, L = None, r.body_labels[0]
    if L < 1:
        raise ValueError("strain.labels: no cell (an empty label image, no points, or no label image in place)")
    tr, cnt = r.strain_labels(states, lab, L)
    return {"J": tr[:, :, 0].copy(), "l1": tr[:, :, 1].copy(), "l2": tr[:, :, 2].copy(), "counts": cnt}


def artifact_score(cell_J, dff):
    """Pearson's r per cell between its local area ratio (frames, cells) and its dF/F (frames, cells), over the frames in
    which both are finite -> (cells,).  Compressed tissue is brighter: a trace that follows its tissue's area change
    (r near -1, or +1) is suspect.  NaN for a constant trace or fewer than two such frames.  A diagnostic, on the host."""
    a = np.asarray(cell_J, np.float64)
    b = np.asarray(dff, np.float64)
    a = a.reshape(a.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    if a.shape != b.shape:
        raise ValueError("artifact_score: traces of shape %r against %r" % (a.shape, b.shape))
    out = np.full(a.shape[1], np.nan)
    for s in range(a.shape[1]):
        ok = np.isfinite(a[:, s]) & np.isfinite(b[:, s])
        if ok.sum() < 2:
            continue
        x, y = a[ok, s] - a[ok, s].mean(), b[ok, s] - b[ok, s].mean()
        den = np.sqrt((x * x).sum() * (y * y).sum())
        if den > 0.0 and np.ptp(a[ok, s]) > 0.0 and np.ptp(b[ok, s]) > 0.0:
            out[s] = float(np.clip((x * y).sum() / den, -1.0, 1.0))
    return out


def write_video(kf_or_renderer, states, source, path, which="J", gain=DEFAULT_GAIN, alpha=DEFAULT_ALPHA, lut=None,
                wire=False, fps=20, video_opts=None):
    """The strain video of a finished track: frame k of `source` (``frame_at(k)`` -> raw frame, ...; or an array
    (frames, H, W) uint8) with `which` (J, l1, l2) of the mesh at states[k] painted on (Renderer.view_strain), written
    to the AVI `path` (uncompressed; video_opts: AviWriter's codec options) by the writer thread of a taps.VideoTap, as cellview.write_video does: the disk is
    not waited for.  Pass the smoothed states of a run that has them.  -> frames written."""
    r = _body.renderer_of(kf_or_renderer)
    if which not in WHICH:
        raise ValueError("write_video: which %r (one of %s)" % (which, ", ".join(WHICH)))
    lut = default_lut() if lut is None else np.ascontiguousarray(lut, np.uint8)

    def paint(k, X, d_frame, d_out, stream):
        r.view_strain_dev(X, d_frame, d_out, which, gain, alpha, lut, wire, stream)
    return write_painted_video(r, states, source, path, paint, fps, video_opts)
