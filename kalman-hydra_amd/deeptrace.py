"""Full-depth traces: the brightness of the cells read again from the 16-bit frames, once the track and the cells are
known (include/hydra_mi.h, "Full-depth traces").

Tracking, cell finding, footprints, ROIs and demixing work on the 8 bits the frames are mapped to as they enter the frame
ring (hydra_mi.deepio).  That decides where the cells are.  How bright they are is read here in a second pass over the
file: the original frames are uploaded run by run, only the body pixels that belong to some column -- an ROI, a ring, a
shape -- are pulled back through the tracked mesh by the body warp's own rule, and summed in exact integers.

    cols = deeptrace.columns(labels, L, windows=[(seeds, ring_weights, Rg)])
    sums = deeptrace.run(body, stack, states, cols)                 # (F, C) uint64
    res = deeptrace.extract(body, stack, states, roi.extract(body, points))

tests/deeptrace_ref.py restates the rules; with device=None the same bytes come from NumPy on the host (HostMap stands in
for the tracker there).
"""
import collections

import numpy as np

from . import _lib, deepio, roi

C_MAX = 4096
COORD_MAX = 1048576.0
SUB = 256          # the render's sub-pixel grid (csrc/ekf_kernels.h EKF_SUB)

#: col_ptr (C + 1,) int64, pix (M,) int32, wt (M,) uint16, and the directory: {"labels": (first column, end) or None,
#: "windows": [(first column, end) per window set]}
Columns = collections.namedtuple("Columns", "col_ptr pix wt directory")


def columns(labels=None, L=0, windows=(), shape=None):
    """The columns of a readout in compressed-column form.  labels: an (H, W) label image (-1: none), one column per label
    0 .. L - 1 with weight 1 per pixel, in raster order.  windows: any number of (seeds (P, 2) int (column, row), weights
    (P, 2R+1, 2R+1) uint16, R) sets laid out as hm_body_rec_weighted_sums takes them, one column per seed in the window's
    raster order; entries with zero weight or off the frame are dropped.  shape: (H, W), needed without a label image.
    -> Columns; the label columns come first, then the window sets in turn."""
    if labels is not None:
        labels = np.asarray(labels)
        if labels.ndim != 2:
            raise ValueError("deeptrace.columns: a label image is (H, W), got %r" % (labels.shape,))
        if shape is not None and tuple(shape) != labels.shape:
            raise ValueError("deeptrace.columns: shape %r for a label image of %r" % (tuple(shape), labels.shape))
        shape = labels.shape
    if shape is None:
        raise ValueError("deeptrace.columns: without a label image the frame's shape (H, W) is needed")
    H, W = int(shape[0]), int(shape[1])
    L = int(L) if labels is not None else 0
    ptr, pix, wt = [0], [], []
    directory = {"labels": None, "windows": []}
    if labels is not None:
        if L < 1 or int(labels.max(initial=-1)) >= L:
            raise ValueError("deeptrace.columns: %d labels for an image whose largest is %d" % (L, int(labels.max(initial=-1))))
        flat = labels.reshape(-1)
        on = np.flatnonzero(flat >= 0)
        order = on[np.argsort(flat[on], kind="stable")]             # by label, raster order within one
        pix.append(order.astype(np.int32))
        wt.append(np.ones(order.shape[0], np.uint16))
        cnt = np.bincount(flat[on], minlength=L)
        ptr.extend(np.cumsum(cnt).tolist())
        directory["labels"] = (0, L)
    for seeds, weights, R in windows:
        seeds = np.asarray(seeds).reshape(-1, 2)
        P, R = seeds.shape[0], int(R)
        w = np.asarray(weights)
        if w.shape != (P, 2 * R + 1, 2 * R + 1) or w.dtype.kind not in "ui" or (w.size and (w.min() < 0 or w.max() > 65535)):
            raise ValueError("deeptrace.columns: weights %s %r for %d seeds of radius %d (uint16 (P, 2R+1, 2R+1))"
                             % (w.dtype, w.shape, P, R))
        first = len(ptr) - 1
        d = np.arange(-R, R + 1)
        for s in range(P):
            rr, cc = np.meshgrid(int(seeds[s][1]) + d, int(seeds[s][0]) + d, indexing="ij")
            take = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W) & (w[s] > 0)
            pix.append((rr[take] * W + cc[take]).astype(np.int32))
            wt.append(w[s][take].astype(np.uint16))
            ptr.append(ptr[-1] + int(take.sum()))
        directory["windows"].append((first, first + P))
    C = len(ptr) - 1
    if not 1 <= C <= C_MAX:
        raise ValueError("deeptrace.columns: %d columns outside 1..%d" % (C, C_MAX))
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dt), dt)
    return Columns(np.array(ptr, np.int64), cat(pix, np.int32), cat(wt, np.uint16), directory)


# ---- the host path -----------------------------------------------------------------------------------------------------
class HostMap:
    """The body map of a mesh on the host, for run(device=None): what a tracker's handle computes on the device, from the
    texture coordinates uv (N, 2) and the triangles (T, 3) alone.  It restates the rule of k_body_map (csrc/body_kernels.h;
    body.locate has it for single points) and must stay in step with it: the snap to 1/256 px, exact integer edge
    functions at the pixel centre, top-left ties, the orientation swap, the lowest covering triangle.  What ties it to the
    device is tests/test_deeptrace_gpu.py, where the host path's sums equal the device's.  tri_of (H, W) int64, -1: none; l1, l2 (H, W) float64;
    ids (T, 3) the vertex ids after the orientation swap."""

    def __init__(self, uv, tri, W, H):
        self.nx, self.ny = int(W), int(H)
        self.n = int(np.asarray(uv).reshape(-1, 2).shape[0])
        P = np.rint(np.asarray(uv, np.float32).astype(np.float64).reshape(-1, 2) * SUB).astype(np.int64)
        tri = np.asarray(tri, np.int64).reshape(-1, 3)
        W, H = self.nx, self.ny
        self.tri_of = np.full((H, W), -1, np.int64)
        self.l1, self.l2 = np.zeros((H, W)), np.zeros((H, W))
        self.ids = tri.copy()
        half = SUB // 2
        for t in range(tri.shape[0]):
            i0, i1, i2 = (int(v) for v in tri[t])
            (x0, y0), (x1, y1), (x2, y2) = P[i0].tolist(), P[i1].tolist(), P[i2].tolist()
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if area == 0:
                continue
            if area < 0:
                i1, i2, x1, y1, x2, y2, area = i2, i1, x2, y2, x1, y1, -area
            self.ids[t] = (i0, i1, i2)
            c_lo, c_hi = max(0, (min(x0, x1, x2) - half) // SUB), min(W - 1, (max(x0, x1, x2) - half) // SUB + 1)
            r_lo, r_hi = max(0, (min(y0, y1, y2) - half) // SUB), min(H - 1, (max(y0, y1, y2) - half) // SUB + 1)
            if c_lo > c_hi or r_lo > r_hi:
                continue
            px = (np.arange(c_lo, c_hi + 1, dtype=np.int64) * SUB + half)[None, :]
            py = (np.arange(r_lo, r_hi + 1, dtype=np.int64) * SUB + half)[:, None]
            inside = np.ones((r_hi - r_lo + 1, c_hi - c_lo + 1), bool)
            e = []
            for (ax, ay), (bx, by) in (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1))):
                dx, dy = bx - ax, by - ay
                v = dx * (py - ay) - dy * (px - ax)
                inside &= (v > 0) | ((v == 0) & bool(dy > 0 or (dy == 0 and dx < 0)))        # the top-left rule
                e.append(v)
            sl = (slice(r_lo, r_hi + 1), slice(c_lo, c_hi + 1))
            take = inside & (self.tri_of[sl] < 0)                    # the lowest index wins
            self.tri_of[sl] = np.where(take, t, self.tri_of[sl])
            self.l1[sl] = np.where(take, e[1].astype(np.float64) / np.float64(area), self.l1[sl])
            self.l2[sl] = np.where(take, e[2].astype(np.float64) / np.float64(area), self.l2[sl])

    def plane(self, X, frame):
        """One frame (H, W) of uint16 values at state X -> the registered plane (H, W) uint16"""
        H, W = self.ny, self.nx
        P = np.asarray(X, np.float64).reshape(-1)[:2 * self.n].reshape(self.n, 2)
        on = self.tri_of >= 0
        v = self.ids[np.where(on, self.tri_of, 0)]
        a, b, c = P[v[..., 0]], P[v[..., 1]], P[v[..., 2]]
        with np.errstate(invalid="ignore", over="ignore"):
            xy = (a + self.l1[..., None] * (b - a)) + self.l2[..., None] * (c - a)
            x, y = xy[..., 0], xy[..., 1]
            ok = on & (x >= -COORD_MAX) & (x <= COORD_MAX) & (y >= -COORD_MAX) & (y <= COORD_MAX)
        u, w = np.where(ok, x, 0.5) - 0.5, np.where(ok, y, 0.5) - 0.5
        fc, fr = np.floor(u), np.floor(w)
        ax, bx = u - fc, w - fr
        c0, r0 = fc.astype(np.int64), fr.astype(np.int64)
        ca, cb = np.clip(c0, 0, W - 1), np.clip(c0 + 1, 0, W - 1)
        ra, rb = np.clip(r0, 0, H - 1), np.clip(r0 + 1, 0, H - 1)
        f = np.asarray(frame).astype(np.float64)
        val = (1.0 - bx) * ((1.0 - ax) * f[ra, ca] + ax * f[ra, cb]) + bx * ((1.0 - ax) * f[rb, ca] + ax * f[rb, cb])
        return np.where(ok, np.rint(val), 0.0).astype(np.uint16)


def _column_sums(plane, cols):
    """sums (C,) uint64 of one registered plane: products below 2^32, a column's sum below 2^63 -- exact in uint64"""
    prod = cols.wt.astype(np.uint64) * plane.reshape(-1)[cols.pix].astype(np.uint64)
    run = np.concatenate((np.zeros(1, np.uint64), np.cumsum(prod, dtype=np.uint64)))       # (wraps mod 2^64: differences hold)
    return run[cols.col_ptr[1:]] - run[cols.col_ptr[:-1]]


def _renderer(kf_or_body):
    from .body import renderer_of
    return kf_or_body.r if hasattr(kf_or_body, "r") else renderer_of(kf_or_body)


def _states(states, N):
    x = np.asarray(states, np.float64)
    x = x.reshape(x.shape[0], -1) if x.ndim >= 2 else x.reshape(1, -1)
    if x.shape[1] < 2 * N:
        raise ValueError("deeptrace: states of %d entries for a mesh of %d vertices" % (x.shape[1], N))
    out = np.zeros((x.shape[0], 4 * N))
    out[:, :min(4 * N, x.shape[1])] = x[:, :4 * N]
    return out


def run(kf_or_body, source, states, cols, planes=False, device=0, first=1, run_frames=8):
    """The second pass.  kf_or_body: a tracker, its renderer or its BodyReadout (device=None: a HostMap); source: a
    TiffStack or a uint16 array (frames, H, W), as DeepSource takes them; states: S of them, state k for frame
    `first` + k of the source.  first = 1 is the body readout's pairing: frame 0 is the template and the state of step k
    belongs to frame k + 1, however many steps were tracked -- a run that ended early reads frames 1 .. S and leaves the
    rest of the file alone.  The pairing is never guessed from the counts: states that reach past the last frame are
    refused.  cols: Columns, or None with planes=True.
    -> sums (S, C) uint64, or (sums or None, planes (S, H, W) uint16) with planes=True.  run_frames: frames per run of
    the upload (the handle's max_run)."""
    fr = source if isinstance(source, deepio._Frames) else deepio._Frames(source)
    r = kf_or_body if device is None and isinstance(kf_or_body, HostMap) else _renderer(kf_or_body)
    if (r.ny, r.nx) != (fr.H, fr.W):
        raise ValueError("deeptrace.run: frames of %dx%d for a tracker of %dx%d" % (fr.W, fr.H, r.nx, r.ny))
    X = _states(states, r.n)
    S = X.shape[0]
    first = int(first)
    if S < 1 or first < 0 or first + S > fr.F:
        raise ValueError("deeptrace.run: %d states from frame %d on (first = %d), the source has %d frames" % (S, first, first, fr.F))
    if cols is None and not planes:
        raise ValueError("deeptrace.run: neither columns nor planes asked for")
    n = fr.H * fr.W
    if cols is not None and cols.pix.size and (int(cols.pix.min()) < 0 or int(cols.pix.max()) >= n):
        raise ValueError("deeptrace.run: a column entry outside the frame's %d pixels" % n)
    C = 0 if cols is None else len(cols.col_ptr) - 1
    sums = np.zeros((S, C), np.uint64) if cols is not None else None
    out = np.zeros((S, fr.H, fr.W), np.uint16) if planes else None
    if device is None:
        hm = r if isinstance(r, HostMap) else HostMap(r.uv, r.tri, r.nx, r.ny)
        for i in range(S):
            p = hm.plane(X[i], fr.values(first + i, first + i + 1)[0])
            if cols is not None:
                sums[i] = _column_sums(p, cols)
            if planes:
                out[i] = p
    else:
        L = _lib.lib()
        h = deepio._Handle(fr.W, fr.H, int(run_frames), device)
        try:
            if cols is not None:
                _lib.check(L.hm_deep_body_set_columns(h._h, r._h, C, _lib.ptr(cols.col_ptr), _lib.ptr(cols.pix) if cols.pix.size
                                                      else _lib.ptr(np.zeros(1, np.int32)), _lib.ptr(cols.wt) if cols.wt.size
                                                      else _lib.ptr(np.zeros(1, np.uint16))), "hm_deep_body_set_columns")
            # an array goes over in large pieces, a stack in pieces of a few runs (its pages are put together first): the
            # upload of a run goes beside the kernels of the run before within a piece
            step = max(int(run_frames), (64 << 20) // (2 * n)) if fr.stack is None else 4 * int(run_frames)
            for i0 in range(0, S, step):
                i1 = min(i0 + step, S)
                block = np.ascontiguousarray(fr.block(first + i0, first + i1))
                _lib.check(L.hm_deep_body_run(h._h, r._h, i1 - i0, _lib.ptr(block), int(fr.swap), _lib.ptr(np.ascontiguousarray(X[i0:i1])),
                                              _lib.ptr(sums[i0:i1]) if cols is not None else None,
                                              _lib.ptr(out[i0:i1]) if planes else None), "hm_deep_body_run")
        finally:
            h.close()
    return (sums, out) if planes else sums


# ---- traces ------------------------------------------------------------------------------------------------------------
def point_means(sums, counts, offset=0.0):
    """Sums (F, P) over labels of `counts` pixels -> the means less `offset` (F, P) float64, NaN for a label without pixels"""
    return roi._means(np.asarray(sums), counts, np.nan) - np.float64(offset)


def traces(roi_sums, roi_counts, ring_sums, ring_counts, alpha=0.7, q=10.0, half=100, offset=0.0):
    """roi.extract's expressions on full-depth sums -> (F_roi, F_np, dff), each (F, P) float64: the means (roi._means: NaN
    for an ROI without pixels, 0 for an empty ring), `offset` -- the camera's black level -- subtracted from both, then
    F_c = F_roi - alpha F_np and dff = (F_c - F0) / F0_raw with roi.baseline's running percentiles."""
    F_roi = roi._means(np.asarray(roi_sums), roi_counts, np.nan)
    F_np = roi._means(np.asarray(ring_sums), ring_counts, 0.0)
    if offset != 0.0:
        F_roi = F_roi - np.float64(offset)
        for s in range(F_np.shape[1]):
            if ring_counts[s] > 0:                                  # (an empty ring stays 0: there is nothing to correct with)
                F_np[:, s] = F_np[:, s] - np.float64(offset)
    F_c = F_roi - np.float64(alpha) * F_np
    dff = np.empty(F_c.shape)
    for s in range(F_c.shape[1]):
        with np.errstate(invalid="ignore", divide="ignore"):
            dff[:, s] = (F_c[:, s] - roi.baseline(F_c[:, s], q, half)) / roi.baseline(F_roi[:, s], q, half)
    return F_roi, F_np, dff


def extract(body, source, states, rois, demixed=None, alpha=0.7, q=10.0, half=100, offset=0.0, device=0, first=1):
    """The full-depth traces of the cells roi.extract found: rois is its dict (or demix.extract's), demixed optionally
    demix.extract's dict; states are the filtered ones the kept record was warped at, one per recorded frame, state k for
    frame `first` + k of the source (run: 1 is the body readout's pairing).  One pass over
    the file with the ROIs (roi_labels), the rings (roi.ring_weights) and, with demixed, the shapes (shapes_q) as columns.
    -> dict: deep_F_roi, deep_F_np, deep_dff (F, P) float64 by roi.extract's own expressions (`offset`, the camera's black
    level, is subtracted from both means first: with offset 0 and values that fit 8 bits deep_dff equals dff bit for bit);
    with demixed also deep_demix_c (F, P) float64, the traces step of demix.extract on the full-depth weighted sums (its
    last shapes and their overlap matrix demix_G); deep_roi_sums, deep_ring_sums (F, P) uint64."""
    from . import demix
    labels = np.asarray(rois["roi_labels"])
    counts = np.asarray(rois["roi_counts"])
    seeds = np.asarray(rois["seeds"])
    P = seeds.shape[0]
    r_in, r_out = (float(v) for v in rois["ring_radii"])
    inmap = np.asarray(body.tri_of_pixel) >= 0
    w, ring_counts, Rg = roi.ring_weights(labels, inmap, seeds, r_in, r_out)
    windows = [(seeds, w, Rg)]
    if demixed is not None:
        a_q = np.asarray(demixed["shapes_q"], np.uint16)
        windows.append((seeds, a_q, (a_q.shape[1] - 1) // 2))
    cols = columns(labels, P, windows)
    sums = run(body, source, states, cols, device=device, first=first)
    (g0, g1) = cols.directory["windows"][0]
    # (label sums count map pixels alone, as hm_body_rec_label_sums: a pixel off the map adds 0 and roi_counts leaves it out)
    lsum, gsum = sums[:, :P], sums[:, g0:g1]
    F_roi, F_np, dff = traces(lsum, counts, gsum, ring_counts, alpha, q, half, offset)
    out = dict(deep_F_roi=F_roi, deep_F_np=F_np, deep_dff=dff, deep_roi_sums=lsum, deep_ring_sums=gsum)
    if demixed is not None:
        (s0, s1) = cols.directory["windows"][1]
        ngs = [max(int(v), 1) for v in ring_counts]
        Cn, _, bad = demix.solve_traces(np.asarray(demixed["demix_G"], np.int64), a_q.astype(np.int64), roi._ints(sums[:, s0:s1]),
                                        roi._ints(gsum), ngs)
        if Cn is None:
            raise np.linalg.LinAlgError("deeptrace.extract: the shapes' overlap matrix does not factor at seed %d" % bad)
        out["deep_demix_c"] = Cn
    return out
