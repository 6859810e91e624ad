"""Body-frame readout of a track: the frames in the animal's own coordinates, points marked in frame 0 followed through
the mesh, and intensity traces of body regions (the neuron tracking the reference's synthetic neurons are made for,
reference gen_synthetic_neurons.py, synth.py:219-266, and that its test_neurontracking.py:15 leaves unbuilt).

Body coordinates are the frame-0 pixel grid of the texture coordinates uv (the initial vertices).  The mesh maps every
triangle from uv to its place in frame k (the state X); pulling frame k back through that piecewise-affine map gives the
registered frame.  The registered frames and the sums of their values per triangle and per label are computed on the
device (hm_body_* in include/hydra_mi.h, csrc/body_kernels.h); points are located and tracked here, on the host, by the
same coverage rule and the same position formula, so a point at a pixel centre gets exactly that pixel's position.

    body = BodyReadout(kf, points=read_points_csv("neurons.csv")[1])
    for each frame: kf.compute(...); reg, tri_means, point_means = body.frame(kf.state.X, raw_frame)
    res = body.results()          # tri_means (F x T), points (F x P x 2), point_means (F x P), ...

FlowEKFPipeline.run(body=body) queues the same readout on the device after every step (BodyTap).

Where the cells are: BodyReadout(kf, stats=True) accumulates per-pixel sums of the registered frames on the device while
the video is tracked (hm_body_stats_*); summary() gives the mean, standard deviation, maximum and local correlation
images, find_points(n) the n best local maxima of one of them in the format `points` takes, and read_out(kf, states,
frames, points) the second pass over the recorded states that reads their traces.

BodyReadout(kf, keep=True) keeps the registered video itself on the device (hm_body_rec_*): hydra_mi.roi.extract builds
footprints, ROIs and neuropil-corrected dF/F traces from it, and the traces of points found afterwards need no second pass.
"""
import ctypes

import numpy as np

from .taps import SlotRing

SUB = 256          # the render's sub-pixel grid (csrc/ekf_kernels.h EKF_SUB)


def read_points_csv(path):
    """reference synth.py:227-231: lines ``name,x,y`` -> (names, (P, 2) float64 in body coordinates)."""
    names, pts = [], []
    with open(path) as f:
        for line in f:
            parts = line.strip().split(",")
            if len(parts) < 3:
                continue
            try:
                x, y = float(parts[1]), float(parts[2])
            except ValueError:               # a header line
                continue
            names.append(parts[0])
            pts.append([x, y])
    return names, np.array(pts, np.float64).reshape(-1, 2)


def write_points_csv(path, points, names=None):
    """The inverse of read_points_csv: lines ``name,x,y`` (names default to p0, p1, ...), the coordinates as repr() of
    the float, so they read back exactly."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    if names is None:
        names = ["p%d" % i for i in range(pts.shape[0])]
    if len(names) != pts.shape[0]:
        raise ValueError("%d names for %d points" % (len(names), pts.shape[0]))
    with open(path, "w") as f:
        for name, (x, y) in zip(names, pts):
            if "," in str(name):
                raise ValueError("a comma in the point name %r" % (name,))
            f.write("%s,%r,%r\n" % (name, float(x), float(y)))


def write_points_txt(path, points):
    """reference synth.py:245-266: one line ``neurons,x0,y0,x1,y1,...`` per frame; points (F, P, 2).  Values are written
    as repr() of the float (``nan`` for a point outside the mesh), so they read back exactly."""
    pts = np.asarray(points, np.float64)
    with open(path, "w") as f:
        for row in pts.reshape(pts.shape[0], -1):
            f.write("neurons," + ",".join(repr(float(v)) for v in row) + "\n")


def read_points_txt(path):
    """The inverse of write_points_txt -> (F, P, 2)."""
    rows = []
    with open(path) as f:
        for line in f:
            parts = line.strip().split(",")
            if parts and parts[0] == "neurons":
                rows.append([float(v) for v in parts[1:]])
    return np.array(rows, np.float64).reshape(len(rows), -1, 2)


def disc_labels(tri_of_pixel, points, radius):
    """Label image of point discs: each map pixel (tri_of_pixel >= 0) whose centre (c + 0.5, r + 0.5) lies within
    `radius` of a point, distance^2 <= radius^2 in float64, gets that point's index; the nearest point wins, the lower
    index on a tie.  -1 elsewhere."""
    tri = np.asarray(tri_of_pixel)
    H, W = tri.shape
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    lab = np.full((H, W), -1, np.int32)
    best = np.full((H, W), np.inf)
    r = float(radius)
    r2 = r * r
    for i, (qx, qy) in enumerate(pts):
        if not (np.isfinite(qx) and np.isfinite(qy)):
            continue
        c0, c1 = max(0, int(np.floor(qx - r - 1))), min(W, int(np.ceil(qx + r + 1)) + 1)
        r0, r1 = max(0, int(np.floor(qy - r - 1))), min(H, int(np.ceil(qy + r + 1)) + 1)
        if c0 >= c1 or r0 >= r1:
            continue
        cx = np.arange(c0, c1, dtype=np.float64) + 0.5
        cy = np.arange(r0, r1, dtype=np.float64) + 0.5
        d2 = (cx[None, :] - qx) ** 2 + (cy[:, None] - qy) ** 2
        sl = (slice(r0, r1), slice(c0, c1))
        take = (d2 <= r2) & (d2 < best[sl]) & (tri[sl] >= 0)      # (strictly nearer: a tie keeps the lower index)
        best[sl] = np.where(take, d2, best[sl])
        lab[sl] = np.where(take, i, lab[sl])
    return lab


def locate(uv, tri, points):
    """Points q (P, 2) in body coordinates -> (triangle (P,) int64, -1 outside every triangle; l1, l2 (P,) float64).
    The render's coverage rule at the snapped point rint(256 q) instead of a pixel centre (positions uv snapped to
    1/256 px, exact integer edge functions, top-left ties, the orientation swap), the lowest triangle index first;
    l1 = e1 / area, l2 = e2 / area, the vertex ids in the swapped order."""
    P = np.rint(np.asarray(uv, np.float64) * SUB).astype(np.int64)
    q = np.asarray(points, np.float64).reshape(-1, 2)
    tri = np.asarray(tri, np.int64)
    n = q.shape[0]
    out_t = np.full(n, -1, np.int64)
    out_ids = np.zeros((n, 3), np.int64)
    l1 = np.zeros(n)
    l2 = np.zeros(n)
    for k in range(n):
        if not (np.isfinite(q[k]).all() and np.abs(q[k]).max() < 2.0 ** 24):
            continue
        px, py = (int(v) for v in np.rint(q[k] * SUB))
        for t, (i0, i1, i2) in enumerate(tri):
            i0, i1, i2 = int(i0), int(i1), int(i2)
            (x0, y0), (x1, y1), (x2, y2) = P[i0].tolist(), P[i1].tolist(), P[i2].tolist()
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if area == 0:
                continue
            if area < 0:
                i1, i2 = i2, i1
                (x1, y1), (x2, y2) = (x2, y2), (x1, y1)
                area = -area
            e0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
            e1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
            e2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)

            def inside(e, dx, dy):
                return e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dx < 0)))
            if inside(e0, x2 - x1, y2 - y1) and inside(e1, x0 - x2, y0 - y2) and inside(e2, x1 - x0, y1 - y0):
                out_t[k] = t
                out_ids[k] = (i0, i1, i2)
                l1[k] = e1 / area                        # Python integers: one correctly rounded division
                l2[k] = e2 / area
                break
    return out_t, out_ids, l1, l2


def track(pos, ids, l1, l2, inside):
    """Positions (P, 2) in the frame whose vertex positions are pos (2N values, x0, y0, x1, ...):
    (X[i0] + l1 (X[i1] - X[i0])) + l2 (X[i2] - X[i0]) in binary64; NaN for the points not inside."""
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    n = len(l1)
    out = np.full((n, 2), np.nan)
    if n == 0:
        return out
    a, b, c = pos[ids[:, 0]], pos[ids[:, 1]], pos[ids[:, 2]]
    p = (a + l1[:, None] * (b - a)) + l2[:, None] * (c - a)
    out[inside] = p[inside]
    return out


def _means(sums, counts):
    s = np.asarray(sums, np.float64)
    c = np.asarray(counts, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, s / np.where(c > 0, c, 1.0), np.nan)


def renderer_of(kf_or_renderer):
    """The renderer.Renderer of a kalman.*KalmanFilter, or the renderer itself"""
    return kf_or_renderer.state.renderer if hasattr(kf_or_renderer, "state") else kf_or_renderer


class BodyReadout:
    """The body-frame readout of one tracker (a kalman.*KalmanFilter or a renderer.Renderer).

    points: (P, 2) points in body coordinates, followed through the mesh (``track``) and read out over discs of
    point_radius px (``disc_labels``); labels: an (H, W) int32 label image in body coordinates (-1: none) instead of
    the discs; video: an AviWriter of the frame size that receives the registered frames (B = G = R); stats: start the
    tracker's statistics of the registered video (every frame read out from now on is added: summary, find_points);
    keep: keep the registered video itself in device memory (hm_body_rec_*, at most keep_bytes; the frame that would pass
    them raises and is not read out), for hydra_mi.roi.extract and the traces of points found afterwards."""

    def __init__(self, kf_or_renderer, points=None, point_radius=3.0, labels=None, video=None, stats=False, keep=False,
                 keep_bytes=8 << 30):
        r = self.r = renderer_of(kf_or_renderer)
        self.H, self.W, self.T = r.ny, r.nx, int(r.tri.shape[0])
        self.video = video
        if video is not None and (video.width, video.height) != (self.W, self.H):
            raise ValueError("a %dx%d video for %dx%d frames" % (video.width, video.height, self.W, self.H))
        self.tri_of_pixel, self.tri_counts = r.body_map()
        if points is not None and labels is not None:
            raise ValueError("BodyReadout: give points (their discs are the labels) or a label image, not both")
        self.points = None if points is None else np.asarray(points, np.float64).reshape(-1, 2)
        self.point_radius = float(point_radius)
        self.outside = np.zeros(0, bool)
        if self.points is not None:
            self.locate(self.points)
            labels = disc_labels(self.tri_of_pixel, self.points, self.point_radius)
            L = self.points.shape[0]
        elif labels is not None:
            labels = np.ascontiguousarray(labels, np.int32)
            L = int(labels.max()) + 1 if labels.size else 0
        self.labels = labels
        self.L = 0
        # the handle holds one label image: this readout sets (or clears) it, and a later readout or body_set_labels on
        # the same tracker replaces it -- this one then refuses to go on (_own_labels)
        if labels is not None and L > 0:
            self.label_counts = r.body_set_labels(labels, L)
            self.L = L
        else:
            self.label_counts = r.body_set_labels(None, 0)
        self._labels = r.body_labels
        self._rows = []         # per state passed: [positions or None, tri sums, label sums]
        self.stats = bool(stats)
        if self.stats:
            r.body_stats_begin()
        self.keep = bool(keep)
        if self.keep:
            r.body_rec_begin(int(keep_bytes))

    # -- points -----------------------------------------------------------------------------------------
    def locate(self, points):
        """-> (triangle, l1, l2) of every point (triangle -1: outside the mesh); keeps them for ``track``."""
        t, ids, l1, l2 = locate(self.r.uv, self.r.tri, points)
        self._loc = (t, ids, l1, l2)
        self.outside = t < 0
        return t, l1, l2

    def track(self, X):
        """Positions (P, 2) of the located points in the frame of state X (NaN outside the mesh)."""
        t, ids, l1, l2 = self._loc
        x = np.asarray(X, np.float64).reshape(-1)[:2 * self.r.n]
        return track(x, ids, l1, l2, t >= 0)

    # -- frames -----------------------------------------------------------------------------------------
    def registered(self, X, frame):
        """Frame (H, W) uint8 pulled back through the mesh at state X -> (H, W) uint8 in body coordinates."""
        self._own_labels()
        return self.r.body_warp(X, frame)[0]

    def frame(self, X, frame):
        """Read out one frame: -> (registered (H, W) uint8, triangle means (T,), label means (L,)); kept for results()
        and written to the video, if any."""
        self._own_labels()
        reg, ts, ls = self.r.body_warp(X, frame)
        self._keep(X, ts, ls)
        if self.video is not None:
            self.video.write(reg if getattr(self.video, "channels", 3) == 1 else np.repeat(reg[:, :, None], 3, axis=2))
        return reg, _means(ts, self.tri_counts), _means(ls, self.label_counts) if ls is not None else np.zeros(0)

    def _own_labels(self):
        if self.r.body_labels != self._labels:
            raise RuntimeError("BodyReadout: the tracker's label image has been replaced since this readout set it (one "
                               "readout per tracker at a time)")

    def _keep(self, X, ts, ls):
        pos = self.track(X) if self.points is not None else None
        self._rows.append([pos, ts, ls])

    # -- where the cells are ----------------------------------------------------------------------------
    def summary(self):
        """Summary images of the frames read out since the readout was made (stats=True): {"frames": F, "mean", "std",
        "corr": (H, W) float64, NaN outside the mesh, "max": (H, W) uint8}.  Waits for the frames queued so far."""
        if not self.stats:
            raise RuntimeError("BodyReadout.summary: the readout was made without stats=True")
        frames = self.r.body_stats_count()
        mean, std, corr, vmax = self.r.body_stats_images()
        return {"frames": frames, "mean": mean, "std": std, "max": vmax, "corr": corr}

    def find_points(self, n, radius=6, score="corr", min_score=None):
        """The n best local maxima of a summary image ("corr", "std" or "range" = max - mean) within (2 radius + 1)^2
        windows, at least min_score (None: no threshold) -> (points (P <= n, 2) float64 at the pixel centres
        (c + 0.5, r + 0.5) in body coordinates, what ``points=`` and read_points_csv speak; scores (P,))."""
        if not self.stats:
            raise RuntimeError("BodyReadout.find_points: the readout was made without stats=True")
        idx, sc, _ = self.r.body_stats_peaks(score, radius, -np.inf if min_score is None else float(min_score), int(n))
        return self.pixel_points(idx), sc

    def pixel_points(self, idx):
        """Raster indices (P,) of the body frame -> (P, 2) float64, the pixel centres (c + 0.5, r + 0.5)"""
        rr, cc = np.divmod(np.asarray(idx).astype(np.int64), self.W)
        return np.stack((cc + 0.5, rr + 0.5), 1).astype(np.float64).reshape(-1, 2)

    def record(self, who):
        """The renderer that holds this readout's kept record (keep=True); `who` names the caller in the refusal.
        (Called as BodyReadout.record(body, who): a stand-in for a readout need carry `keep` and `r` alone.)"""
        if not getattr(self, "keep", False):
            raise RuntimeError("%s: the readout was made without keep=True" % who)
        return self.r

    def results(self):
        """Arrays with one row per state passed: tri_sums / tri_means (F x T), tri_counts (T); with labels label_sums /
        label_means (F x L), label_counts; with points also points (F x P x 2), point_means (F x P), point_counts (P)."""
        F = len(self._rows)
        ts = np.array([r[1] for r in self._rows], np.uint64).reshape(F, self.T)
        out = {"tri_sums": ts, "tri_means": _means(ts, self.tri_counts[None, :]), "tri_counts": self.tri_counts.copy()}
        if self.L > 0:
            ls = np.array([r[2] for r in self._rows], np.uint64).reshape(F, self.L)
            out.update(label_sums=ls, label_means=_means(ls, self.label_counts[None, :]),
                       label_counts=self.label_counts.copy())
        if self.points is not None:
            P = self.points.shape[0]
            out["points"] = np.array([r[0] for r in self._rows], np.float64).reshape(F, P, 2)
            out["point_counts"] = self.label_counts.copy() if self.L > 0 else np.zeros(P, np.uint32)
            out["point_means"] = out["label_means"] if self.L > 0 else np.full((F, P), np.nan)
        return out


def read_out(kf_or_renderer, states, frames, points, point_radius=3.0):
    """The second pass: a fresh BodyReadout with these points over recorded states and the raw frames they belong to
    (any iterable of (H, W) uint8 frames, one per state), no tracking -> its results().  The traces need the cells and the
    cells need the whole video: two passes over the frames, one tracking run."""
    b = BodyReadout(kf_or_renderer, points=points, point_radius=point_radius)
    it = iter(frames)
    for X in states:
        try:
            f = next(it)
        except StopIteration:
            raise ValueError("read_out: fewer frames than states (%d)" % len(states)) from None
        b.frame(X, f)
    return b.results()


def record_bytes(tri_of_pixel, frames):
    """Device memory the kept registered video of `frames` frames takes (hm_body_rec_*): the bounding box of the body
    map, one byte per pixel, rows padded to 4 bytes and frames to 16."""
    m = np.asarray(tri_of_pixel) >= 0
    if not m.any():
        return 16 * int(frames)
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)
    return ((((bw + 3) // 4 * 4) * bh + 15) // 16 * 16) * int(frames)


def read_out_recorded(body, states, points, point_radius=3.0):
    """What read_out gives for `points`, from the registered video a BodyReadout(keep=True) holds on the device instead
    of a second pass over the frames: the discs' sums of every recorded frame in one call (hm_body_rec_label_sums), the
    positions from the recorded states.  One state per recorded frame."""
    r = body.r
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    P = pts.shape[0]
    F = r.body_rec_count()
    if len(states) != F:
        raise ValueError("read_out_recorded: %d states for %d recorded frames" % (len(states), F))
    t, ids, l1, l2 = locate(r.uv, r.tri, pts)
    x = np.asarray(states, np.float64).reshape(F, -1)[:, :2 * r.n]
    pos = np.array([track(row, ids, l1, l2, t >= 0) for row in x], np.float64).reshape(F, P, 2)
    labels = disc_labels(body.tri_of_pixel, pts, point_radius)
    counts = np.bincount(labels[labels >= 0], minlength=P).astype(np.uint32) if P else np.zeros(0, np.uint32)
    if P and F:
        sums = r.body_rec_label_sums(labels, P)
        means = _means(sums, counts[None, :])
    else:
        means = np.full((F, P), np.nan)
    return {"points": pos, "point_means": means, "point_counts": counts}


class BodyTap(SlotRing):
    """The readout of a pipeline run (FlowEKFPipeline.run(body=...)): after every step the warp of the raw frame at the
    state the frame ended with is queued on the filter's stream (hm_body_warp_dev) into a ring of device slots -- its
    sums, and the registered frame as B = G = R when the readout has a video --, copied into page-locked memory on a copy
    stream of its own that waits for the warp, and taken by a writer thread (sums into the readout's rows, frames into
    the video).  The frame ring may reuse the slot of a frame the warp reads only after the warp: ``frame`` hands the
    ring a fence (hm_body_fence) that its copy stream waits on before its next upload.

    With an MJPEG video the warp writes the registered frame with as many channels as the video codes (one for a grey
    video), the video's encoder is queued behind it on the same stream, and only the sums are downloaded with the slot:
    the writer thread copies the stream's own bytes (videoio.MjpegSlots)."""

    def __init__(self, body, device=0, slots=4):
        self.b = body
        r = body.r
        self.npx = r.nx * r.ny
        self.ns = 8 * (body.T + body.L)                 # a slot: the sums (8-byte aligned), then the frame, if any
        self.nv = 3 * self.npx if body.video is not None else 0
        self.ch = 3
        mjpeg = body.video is not None and getattr(body.video, "mjpeg", False)
        if mjpeg:
            self.ch = body.video.channels
            self.nv = self.ch * self.npx
        self.stride = self.ns + self.nv
        # (MJPEG: the frame stays on the device, with the stream the encoder makes of it behind it)
        self.nd = self.ns if mjpeg else self.stride                           # bytes of a slot that are downloaded
        SlotRing.__init__(self, "hydra_mi-body", device, slots, self.stride, self.stride, body.video.encoder if mjpeg else None)

    def frame(self, X, d_frame, ring=None):
        """Queue the readout of the raw frame at device address d_frame at state X (a frame of `ring`, if given)."""
        s, d = self._take()
        try:
            b = self.b
            b._own_labels()                         # (the slot holds the sums of this readout's L labels)
            b._keep(X, None, None)
            row = len(b._rows) - 1
            b.r.body_warp_dev(X, d_frame, d + self.ns if self.nv else None, self.ch, d, d + 8 * b.T if b.L else None, self._stream)
            if ring is not None:
                ring.fence_after(lambda st: b.r.body_fence(st))
            if self._mj is not None:
                b.video.encoder.encode_dev(d + self.ns, d + self.stride, self._mj.cap, self._mj.size_word(s), self._stream)
            self._download(s, self.nd)
        except Exception:
            self._give_back()
            raise
        self._submit((s, row))

    def _written(self, item):
        s, row = item
        b, base = self.b, self._pinned(s)
        blk = np.ctypeslib.as_array(ctypes.cast(base, ctypes.POINTER(ctypes.c_uint64)), shape=(b.T + b.L,)).copy()
        b._rows[row][1] = blk[:b.T]
        b._rows[row][2] = blk[b.T:] if b.L else None
        if self._mj is not None:
            self._mj.finish(s, self._dev[s].ptr + self.stride, b.video)
        elif self.nv:
            b.video.write_ptr(base + self.ns)
