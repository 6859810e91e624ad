"""Measurement model of the mesh tracker on MI355X.

Host mirror of the reference's ``renderer.Renderer`` (reference
renderer.py:197-737) for the part that is on the hot path: the four off-screen
renders of the textured mesh and the reductions against the observed frame
that the reference splits between OpenGL (renderer.py:310-325) and the CUDA
kernels of ``CUDAGL`` / ``CUDAGL_multi`` (cuda.py, cuda_multi.py).  Here both
live in libhydra_mi.so (csrc/ekf.hip): a software rasteriser and fused
perturb-and-reduce kernels; nothing is rendered on a CPU and there is no
fallback.  The views of the reference canvas (raw, overlay, texture, mask, flowx,
flowy; renderer.py:436-475, 595-628) and its force plot are composed on the device
as well (``view``, ``screenshot``, ``view_forces``); the on-screen canvas and its
key bindings are not part of this build.

Same method names and argument meaning as the reference:
``update_vertex_buffer``, ``render``, ``initjacobian``, ``jz``, ``jz_multi``,
``j``, ``j_multi``, ``error``, ``update_frame``, ``get_flow``; plus ``measure``,
the fused form of ``KFState.update`` (kalman.py:437-449).

``FlowStream`` reads the ``<path>_%03d_x.mat`` / ``_y.mat`` files the flow tool
writes (reference renderer.py:807-874).
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import matio


class ChainedPredictionFailed(RuntimeError):
    """hm_update_run, chained to a state prediction on the device (hm_chain_project), found that the prediction's inner
    solve had given up: nothing was updated; predict on the host and update again."""


class Renderer:
    def __init__(self, distmesh, vel, flow, nx, im1, cuda, eps_Z, eps_J, eps_M, labels=None, labels_hess=None,
                 Q=None, showtracking=False, force=None, multi=True, device=0):
        if not cuda:
            raise NotImplementedError(
                "cuda=False: this build has no CPU measurement path (the reference's NumPy twin, "
                "cuda.py:929-1010, is restated under oracle/ as test infrastructure only)")
        self._h = None
        self.Q = Q
        self.cuda = cuda
        self.force = force
        self.labels, self.labels_hess = labels, labels_hess
        self.tri = np.ascontiguousarray(distmesh.t, np.int32)
        self.n = int(distmesh.p.shape[0])
        im1 = np.asarray(im1)
        tex = im1 if im1.ndim == 2 else im1[:, :, 0]      # the r8 target keeps channel 0 (cuda.py:931)
        self.ny, self.nx = int(tex.shape[0]), int(tex.shape[1])
        if int(nx) != self.ny:
            raise ValueError("nx=%d does not match the frame (%d rows)" % (nx, self.ny))
        uv = np.ascontiguousarray(distmesh.p, np.float32)  # texture coordinates = initial vertices (renderer.py:579)
        L = _lib.lib()
        h = _lib.c_vp()
        _lib.check(L.hm_ctx_create(int(device), self.nx, self.ny, self.n, int(self.tri.shape[0]), _lib.ptr(self.tri),
                                   _lib.ptr(uv), eps_Z, eps_J, eps_M, ctypes.byref(h)), "hm_ctx_create")
        self._h = h
        self.uv = uv                            # body coordinates of the readout (body.py)
        self._body_L, self._body_serial = 0, 0  # the label image of the readout in place (body_set_labels)
        self._worker = None                     # a state-prediction worker attached to this handle (attach_worker)
        _lib.register(self, 2)
        _lib.check(L.hm_set_texture(self._h, _lib.ptr(np.ascontiguousarray(tex, np.uint8))), "hm_set_texture")
        self.vertices = np.array(distmesh.p, np.float64)
        self.velocities = np.array(vel, np.float64).reshape(self.vertices.shape)
        self._obs = None
        self._palette = None
        for kv in os.environ.get("HYDRA_MI_TUNE", "").split(","):          # experiments: "key=value,..." for hm_ctx_tune
            if "=" in kv:
                k, v = kv.split("=")
                _lib.check(L.hm_ctx_tune(h, k.strip().encode(), int(v)), "hm_ctx_tune")
        self.frame_in_place = False             # set by KalmanFilter.compute() while the frame it uploaded is current
        self._cov_serial = 0                    # names the covariance resident on the device (DeviceCovariance)
        self.current_frame = tex
        self.current_flowx, self.current_flowy = flow[:, :, 0], flow[:, :, 1]

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if self._h is not None:
            if self._worker is not None:        # the worker keeps a pointer to this handle: back to its host thread first
                try:
                    _lib.lib().hm_ms_worker_attach(self._worker, None)
                finally:
                    self._worker = None
            _lib.lib().hm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ----------------------------------------------------------------------------
    def update_vertex_buffer(self, vertices, velocities, multi_idx=-1, hess=False):
        """reference renderer.py:503-556: the vertex buffer and the label palette of the mask render
        (multi_idx: the partition whose labels colour the triangles, -1: none; hess: the pair partitions).
        The palette only matters to jz_multi / j_multi."""
        self.vertices = np.asarray(vertices, np.float64).reshape(-1, 2)
        self.velocities = np.asarray(velocities, np.float64).reshape(-1, 2)
        table = self.labels_hess if hess else self.labels
        if multi_idx is None or multi_idx < 0 or table is None:
            self._palette = None                                      # every triangle (255, 255, 255): no label
        else:
            self._palette = np.ascontiguousarray(np.asarray(table)[:, multi_idx], np.int32)

    def _X(self, state=None):
        if state is not None:
            return np.ascontiguousarray(np.asarray(state.X, np.float64).reshape(-1))
        return np.ascontiguousarray(np.concatenate((self.vertices.reshape(-1), self.velocities.reshape(-1))))

    def render(self):
        """The four renders of the current vertex buffer -> (im u8, fx f32, fy f32, m u8)."""
        n = self.nx * self.ny
        im = np.empty((self.ny, self.nx), np.uint8)
        m = np.empty_like(im)
        fx = np.empty((self.ny, self.nx), np.float32)
        fy = np.empty_like(fx)
        _lib.check(_lib.lib().hm_render(self._h, _lib.ptr(self._X()), _lib.ptr(im), _lib.ptr(fx), _lib.ptr(fy),
                                        _lib.ptr(m)), "hm_render")
        self.last_render = (im, fx, fy, m)
        return self.last_render

    def get_flow(self):
        """reference renderer.py:666-672."""
        _, fx, fy, _ = self.render()
        return fx, fy

    # -- views (reference renderer.py:436-475, 595-628) --------------------------------------------
    def _view_palette(self):
        """the mask view's face palette: hessfacecolors[:, :, 1] (renderer.py:624-628, 453), i.e. labels_hess[:, 1];
        -1 (255, 255) for every triangle when there is no such column"""
        lh = self.labels_hess
        if lh is None or np.ndim(lh) != 2 or np.shape(lh)[1] < 2:
            return None
        return np.ascontiguousarray(np.asarray(lh)[:, 1], np.int32)

    def view(self, X=None, which="overlay"):
        """The view `which` (raw, overlay, texture, mask, flowx, flowy) at state X (default: the vertex buffer)
        -> (H, W, 3) uint8, B G R (hm_view).  The overlay's red channel is the observed frame in place."""
        from .videoio import VIEWS
        x = self._X() if X is None else np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        if x.shape[0] != 4 * self.n:
            raise ValueError("state of %d entries for a mesh of %d vertices" % (x.shape[0], self.n))
        out = np.empty((self.ny, self.nx, 3), np.uint8)
        pal = self._view_palette() if which == "mask" else None
        _lib.check(_lib.lib().hm_view(self._h, _lib.ptr(x), VIEWS[which], _lib.ptr(pal), _lib.ptr(out)), "hm_view")
        return out

    def view_dev(self, X, which, d_out, stream=None):
        """hm_view_dev: queue the view into device memory d_out (W*H*3 bytes, 4-byte aligned); `stream` waits for it on
        the device."""
        from .videoio import VIEWS
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        pal = self._view_palette() if which == "mask" else None
        _lib.check(_lib.lib().hm_view_dev(self._h, _lib.ptr(x), VIEWS[which], _lib.ptr(pal), ctypes.c_void_p(int(d_out)),
                                          stream), "hm_view_dev")

    def view_forces(self, X, orig, pred, tv, fv, mv):
        """The force plot of reference kalman.py:638-674 at state X (hm_view_forces): the overlay halved, then the
        arrows orig -> pred (white), pred -> pred + 10 tv / fv / mv (blue, green, red).  Vectors: state-sized or
        2N; the first 2N entries (the vertex coordinates) are used."""
        n2 = 2 * self.n
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        f = [np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)[:n2]) for a in (orig, pred, tv, fv, mv)]
        if x.shape[0] != 4 * self.n or any(a.shape[0] != n2 for a in f):
            raise ValueError("view_forces: states of 4N and vectors of at least 2N entries (N=%d)" % self.n)
        out = np.empty((self.ny, self.nx, 3), np.uint8)
        _lib.check(_lib.lib().hm_view_forces(self._h, _lib.ptr(x), *[_lib.ptr(a) for a in f], _lib.ptr(out)),
                   "hm_view_forces")
        return out

    # -- the cell view (hm_view_set_cells, hm_view_cells*; hydra_mi.cellview) ------------------------------
    def view_set_cells(self, labels, weights=None, colours=None):
        """The cells of the cell view, in body coordinates: labels (n_layers, H, W) or (H, W) int32, -1: none (None
        clears them); weights: the same shape, uint16 (None: 65535 everywhere); colours (L, 3) uint8, B G R, one per
        label.  They stay until set again."""
        self._cells_L = 0
        if labels is None:
            _lib.check(_lib.lib().hm_view_set_cells(self._h, 0, None, None, 0, None), "hm_view_set_cells")
            return
        lab = np.ascontiguousarray(labels, np.int32)
        lab = lab[None] if lab.ndim == 2 else lab
        if lab.ndim != 3 or lab.shape[1:] != (self.ny, self.nx):
            raise ValueError("label planes of shape %r for %dx%d frames" % (lab.shape, self.nx, self.ny))
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.uint16).reshape(lab.shape)
        col = np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
        _lib.check(_lib.lib().hm_view_set_cells(self._h, int(lab.shape[0]), _lib.ptr(lab), _lib.ptr(w), int(col.shape[0]),
                                                _lib.ptr(col)), "hm_view_set_cells")
        self._cells_L = int(col.shape[0])

    def _view_cells_args(self, X, levels, outline, wire, points, point_colours, point_radius):
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        if x.shape[0] < 2 * self.n:
            raise ValueError("state of %d entries for a mesh of %d vertices" % (x.shape[0], self.n))
        lv = None
        if levels is not None:
            lv = np.ascontiguousarray(levels, np.uint8).reshape(-1)
            if lv.shape[0] != getattr(self, "_cells_L", 0):    # (the library reads L bytes there)
                raise ValueError("%d levels for %d cells" % (lv.shape[0], getattr(self, "_cells_L", 0)))
        pts = pc = None
        P = 0
        if points is not None and np.size(points):
            pts = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
            P = int(pts.shape[0])
            pc = np.ascontiguousarray(point_colours, np.uint8).reshape(-1, 3)
            if pc.shape[0] != P:
                raise ValueError("%d colours for %d points" % (pc.shape[0], P))
        flags = (1 if outline else 0) | (2 if wire else 0)
        return x, lv, flags, P, pts, pc, int(point_radius)

    def view_cells(self, X, frame, levels=None, outline=True, wire=False, points=None, point_colours=None, point_radius=2):
        """hm_view_cells: the cells set by view_set_cells and the markers `points` (P, 2) image coordinates, colours
        (P, 3) B G R) painted onto the gray frame (H, W) uint8 at state X -> (H, W, 3) uint8, B G R.  levels: (L,) uint8,
        the activity of every cell in this frame (None: 255)."""
        x, lv, flags, P, pts, pc, rad = self._view_cells_args(X, levels, outline, wire, points, point_colours, point_radius)
        f = self._plane(frame, np.uint8, "frame")
        out = np.empty((self.ny, self.nx, 3), np.uint8)
        _lib.check(_lib.lib().hm_view_cells(self._h, _lib.ptr(x), _lib.ptr(f), _lib.ptr(lv), flags, P, _lib.ptr(pts), _lib.ptr(pc),
                                            rad, _lib.ptr(out)), "hm_view_cells")
        return out

    def view_cells_dev(self, X, d_frame, d_out, levels=None, outline=True, wire=False, points=None, point_colours=None,
                       point_radius=2, stream=None):
        """hm_view_cells_dev: the same queued on the handle's stream, frame (W*H bytes) and output (W*H*3 bytes) device
        addresses; it does not wait, and the host arrays may be overwritten at once; `stream` waits for it on the device."""
        x, lv, flags, P, pts, pc, rad = self._view_cells_args(X, levels, outline, wire, points, point_colours, point_radius)
        _lib.check(_lib.lib().hm_view_cells_dev(self._h, _lib.ptr(x), ctypes.c_void_p(int(d_frame)), _lib.ptr(lv), flags, P,
                                                _lib.ptr(pts), _lib.ptr(pc), rad, ctypes.c_void_p(int(d_out)), stream),
                   "hm_view_cells_dev")

    # -- the body-frame readout (hm_body_*; hydra_mi.body) ------------------------------------------------
    def _plane(self, a, dtype, what):
        """-> `a` as a contiguous (H, W) array of dtype; `what` names it in the refusal"""
        a = np.ascontiguousarray(a, dtype)
        if a.shape != (self.ny, self.nx):
            raise ValueError("%s of shape %r for %dx%d frames" % (what, a.shape, self.nx, self.ny))
        return a

    def _rec_n(self, k0, n):
        """-> the number of frames of a range k0, n of the record (n None: all from k0)"""
        return self.body_rec_count() - int(k0) if n is None else int(n)

    def body_map(self):
        """-> (triangle per pixel (H, W) int32, -1 outside the mesh; pixels per triangle (T,) uint32) at X = uv."""
        tri = np.empty((self.ny, self.nx), np.int32)
        cnt = np.empty(self.tri.shape[0], np.uint32)
        _lib.check(_lib.lib().hm_body_map(self._h, _lib.ptr(tri), _lib.ptr(cnt)), "hm_body_map")
        return tri, cnt

    def body_set_labels(self, labels, L):
        """The label image (H, W) int32 of the label sums (-1: none; None clears) -> map pixels per label (L,) uint32.
        The handle holds one label image: this replaces the one set before (body_labels names the one in place)."""
        self._body_L = 0                          # (a failed call leaves no label count that could outgrow a buffer)
        self._body_serial += 1
        if labels is None:
            _lib.check(_lib.lib().hm_body_set_labels(self._h, None, 0, None), "hm_body_set_labels")
            return np.zeros(0, np.uint32)
        lab = self._plane(labels, np.int32, "label image")
        cnt = np.empty(int(L), np.uint32)
        _lib.check(_lib.lib().hm_body_set_labels(self._h, _lib.ptr(lab), int(L), _lib.ptr(cnt)), "hm_body_set_labels")
        self._body_L = int(L)
        return cnt

    @property
    def body_labels(self):
        """(labels L of the label image in place, 0: none; serial number of the body_set_labels call that set it)"""
        return self._body_L, self._body_serial

    def body_warp(self, X, frame):
        """hm_body_warp: frame (H, W) uint8 pulled back through the mesh at state X -> (registered (H, W) uint8, sums per
        triangle (T,) uint64, sums per label (L,) uint64 of the label image in place, or None when there is none)."""
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        if x.shape[0] < 2 * self.n:
            raise ValueError("state of %d entries for a mesh of %d vertices" % (x.shape[0], self.n))
        f = self._plane(frame, np.uint8, "frame")
        out = np.empty((self.ny, self.nx), np.uint8)
        ts = np.empty(self.tri.shape[0], np.uint64)
        ls = np.empty(self._body_L, np.uint64) if self._body_L else None    # (the library writes L values there)
        _lib.check(_lib.lib().hm_body_warp(self._h, _lib.ptr(x), _lib.ptr(f), _lib.ptr(out), _lib.ptr(ts), _lib.ptr(ls)),
                   "hm_body_warp")
        return out, ts, ls

    def body_warp_dev(self, X, d_frame, d_out, channels, d_tri_sums, d_label_sums, stream=None):
        """hm_body_warp_dev: device addresses (None: NULL); d_label_sums holds body_labels[0] values; `stream` waits for the
        warp on the device."""
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        v = lambda a: None if a is None else ctypes.c_void_p(int(a))
        _lib.check(_lib.lib().hm_body_warp_dev(self._h, _lib.ptr(x), v(d_frame), v(d_out), int(channels), v(d_tri_sums),
                                               v(d_label_sums), stream), "hm_body_warp_dev")

    def body_fence(self, stream):
        """hm_body_fence: `stream` waits on the device for the last warp queued."""
        _lib.check(_lib.lib().hm_body_fence(self._h, stream), "hm_body_fence")

    # -- the deformation readout (hm_strain_*, hm_view_strain*; hydra_mi.strain) ------------------------------
    STRAIN_WHICH = {"J": 0, "l1": 1, "l2": 2}

    def _states(self, states):
        """-> `states` as a contiguous (frames, 4N) float64 array (one state: one row)"""
        x = np.ascontiguousarray(states, np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x.reshape(x.shape[0], -1)
        if x.shape[1] != 4 * self.n:
            raise ValueError("states of %d entries for a mesh of %d vertices" % (x.shape[1], self.n))
        return x

    def strain_tri(self, states):
        """hm_strain_tri: states (frames, 4N) -> (frames, T, 7) float64: J, l1, l2, c2, s2, rc, rs per frame and triangle."""
        x = self._states(states)
        out = np.empty((x.shape[0], self.tri.shape[0], 7), np.float64)
        _lib.check(_lib.lib().hm_strain_tri(self._h, int(x.shape[0]), _lib.ptr(x), _lib.ptr(out)), "hm_strain_tri")
        return out

    def strain_labels(self, states, labels, L):
        """hm_strain_labels: the mean J, l1, l2 over the body-map pixels of every label -> ((frames, L, 3) float64, map
        pixels per label (L,) uint32).  labels: (H, W) int32 in body coordinates, -1: none; None: the label image in
        place (body_set_labels), whose L is passed."""
        x = self._states(states)
        lab = None if labels is None else self._plane(labels, np.int32, "label image")
        out = np.empty((x.shape[0], max(int(L), 0), 3), np.float64)
        cnt = np.empty(max(int(L), 0), np.uint32)
        _lib.check(_lib.lib().hm_strain_labels(self._h, int(x.shape[0]), _lib.ptr(x), _lib.ptr(lab), int(L), _lib.ptr(out),
                                               _lib.ptr(cnt)), "hm_strain_labels")
        return out, cnt

    def _view_strain_args(self, X, which, lut, wire):
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        if x.shape[0] < 2 * self.n:
            raise ValueError("state of %d entries for a mesh of %d vertices" % (x.shape[0], self.n))
        t = None
        if lut is not None:
            t = np.ascontiguousarray(lut, np.uint8)
            if t.shape != (256, 3):
                raise ValueError("a colour table of shape %r (256 x 3, B G R)" % (t.shape,))
        return x, self.STRAIN_WHICH.get(which, which), t, 2 if wire else 0

    def view_strain(self, X, frame, which="J", gain=256.0, alpha=128, lut=None, wire=False):
        """hm_view_strain: J, l1 or l2 of the triangle under every pixel painted onto the gray frame (H, W) uint8 at state X
        -> (H, W, 3) uint8, B G R: level = clamp(128 + rint(gain (value - 1)), 0, 255), colour lut[level] (256 x 3, B G R),
        blended at alpha / 255."""
        x, w, t, flags = self._view_strain_args(X, which, lut, wire)
        f = self._plane(frame, np.uint8, "frame")
        out = np.empty((self.ny, self.nx, 3), np.uint8)
        _lib.check(_lib.lib().hm_view_strain(self._h, _lib.ptr(x), _lib.ptr(f), int(w), float(gain), int(alpha), _lib.ptr(t),
                                             flags, _lib.ptr(out)), "hm_view_strain")
        return out

    def view_strain_dev(self, X, d_frame, d_out, which="J", gain=256.0, alpha=128, lut=None, wire=False, stream=None):
        """hm_view_strain_dev: the same queued on the handle's stream, frame (W*H bytes) and output (W*H*3 bytes) device
        addresses; it does not wait, and X and the table may be overwritten at once; `stream` waits for it on the device."""
        x, w, t, flags = self._view_strain_args(X, which, lut, wire)
        _lib.check(_lib.lib().hm_view_strain_dev(self._h, _lib.ptr(x), ctypes.c_void_p(int(d_frame)), int(w), float(gain),
                                                 int(alpha), _lib.ptr(t), flags, ctypes.c_void_p(int(d_out)), stream),
                   "hm_view_strain_dev")

    # -- statistics of the registered video (hm_body_stats_*; hydra_mi.body.BodyReadout(stats=True)) -------
    SCORES = {"corr": 0, "std": 1, "range": 2}

    def body_stats_begin(self):
        """hm_body_stats_begin: every body_warp / body_warp_dev from now on adds its registered frame; again: restart."""
        _lib.check(_lib.lib().hm_body_stats_begin(self._h), "hm_body_stats_begin")

    def body_stats_end(self):
        """hm_body_stats_end: stop accumulating and free the sums (harmless when not begun)."""
        _lib.check(_lib.lib().hm_body_stats_end(self._h), "hm_body_stats_end")

    def body_stats_count(self):
        """-> frames added since body_stats_begin"""
        n = ctypes.c_int(0)
        _lib.check(_lib.lib().hm_body_stats_count(self._h, ctypes.byref(n)), "hm_body_stats_count")
        return n.value

    def body_stats_fetch(self):
        """-> (s1 (H, W) uint32, s2 (H, W) uint32, cross (4, H, W) uint32: right, down-right, down, down-left,
        vmax (H, W) uint8) of the frames added so far; zeros outside the map."""
        H, W = self.ny, self.nx
        s1, s2 = np.empty((H, W), np.uint32), np.empty((H, W), np.uint32)
        cross, vmax = np.empty((4, H, W), np.uint32), np.empty((H, W), np.uint8)
        _lib.check(_lib.lib().hm_body_stats_fetch(self._h, _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(cross), _lib.ptr(vmax)),
                   "hm_body_stats_fetch")
        return s1, s2, cross, vmax

    def body_stats_images(self):
        """-> (mean, std, corr (H, W) float64, NaN outside the map; max (H, W) uint8) of the frames added so far."""
        H, W = self.ny, self.nx
        mean, std, corr = (np.empty((H, W), np.float64) for _ in range(3))
        vmax = np.empty((H, W), np.uint8)
        _lib.check(_lib.lib().hm_body_stats_images(self._h, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(corr), _lib.ptr(vmax)),
                   "hm_body_stats_images")
        return mean, std, corr, vmax

    def body_stats_peaks(self, score="corr", radius=6, min_score=-np.inf, cap=None):
        """hm_body_stats_peaks: the local maxima of a score image ("corr", "std", "range" = max - mean, or 0, 1, 2)
        within (2 radius + 1)^2 windows -> (raster indices (P,) int32, scores (P,) float64, number found); score
        descending, the first `cap` of them (None: all)."""
        which = self.SCORES[score] if isinstance(score, str) else int(score)
        cap = self.nx * self.ny if cap is None else int(cap)
        idx, sc = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.float64)
        n = ctypes.c_int(0)
        _lib.check(_lib.lib().hm_body_stats_peaks(self._h, which, int(radius), float(min_score), cap, _lib.ptr(idx),
                                                  _lib.ptr(sc), ctypes.byref(n)), "hm_body_stats_peaks")
        k = min(n.value, cap)
        return idx[:k].copy(), sc[:k].copy(), n.value

    # -- the registered video kept on the device (hm_body_rec_*; hydra_mi.body.BodyReadout(keep=True), hydra_mi.roi) --
    def body_rec_begin(self, max_bytes=8 << 30):
        """hm_body_rec_begin: every body_warp / body_warp_dev from now on appends its registered frame to a record in device
        memory of at most max_bytes; again: start over."""
        _lib.check(_lib.lib().hm_body_rec_begin(self._h, int(max_bytes)), "hm_body_rec_begin")

    def body_rec_end(self):
        """hm_body_rec_end: stop recording and free the record (harmless when not begun)."""
        _lib.check(_lib.lib().hm_body_rec_end(self._h), "hm_body_rec_end")

    def body_rec_count(self):
        """-> frames recorded since body_rec_begin"""
        n = ctypes.c_int(0)
        _lib.check(_lib.lib().hm_body_rec_count(self._h, ctypes.byref(n)), "hm_body_rec_count")
        return n.value

    def body_rec_fetch(self, k0=0, n=None):
        """-> recorded frames k0 .. k0 + n - 1 (default: all from k0) as (n, H, W) uint8"""
        n = self._rec_n(k0, n)
        out = np.empty((max(n, 0), self.ny, self.nx), np.uint8)
        _lib.check(_lib.lib().hm_body_rec_fetch(self._h, int(k0), n, _lib.ptr(out)), "hm_body_rec_fetch")
        return out

    def body_rec_label_sums(self, labels, L):
        """hm_body_rec_label_sums: a label image (H, W) int32 given now -> (F, L) uint64, the sums per label of every
        recorded frame."""
        lab = self._plane(labels, np.int32, "label image")
        out = np.empty((self.body_rec_count(), int(L)), np.uint64)
        _lib.check(_lib.lib().hm_body_rec_label_sums(self._h, _lib.ptr(lab), int(L), _lib.ptr(out)), "hm_body_rec_label_sums")
        return out

    def body_rec_seed_sums(self, seeds, r_disc, r_in, r_out, R):
        """hm_body_rec_seed_sums: seeds (P, 2) integer (column, row) map pixels -> dict: n_T, n_G (P,) uint32; T, G (F, P)
        uint64 disc and ring sums; U (F, P) int64 = n_G T - n_T G; w1, w2 (P, 2R+1, 2R+1) uint64 and c (same, int64):
        sums of v, v^2 and v U per window pixel; u1, u2 (P,) int64: sums of U and U^2."""
        sd = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
        P, F, S = sd.shape[0], self.body_rec_count(), 2 * int(R) + 1
        o = dict(n_T=np.empty(P, np.uint32), n_G=np.empty(P, np.uint32), T=np.empty((F, P), np.uint64),
                 G=np.empty((F, P), np.uint64), U=np.empty((F, P), np.int64), w1=np.empty((P, S, S), np.uint64),
                 w2=np.empty((P, S, S), np.uint64), c=np.empty((P, S, S), np.int64), u1=np.empty(P, np.int64),
                 u2=np.empty(P, np.int64))
        _lib.check(_lib.lib().hm_body_rec_seed_sums(self._h, P, _lib.ptr(sd), float(r_disc), float(r_in), float(r_out), int(R),
                                                    *[_lib.ptr(o[k]) for k in ("n_T", "n_G", "T", "G", "U", "w1", "w2", "c",
                                                                               "u1", "u2")]), "hm_body_rec_seed_sums")
        return o

    def body_rec_weighted_sums(self, seeds, weights, R):
        """hm_body_rec_weighted_sums: weights (P, 2R+1, 2R+1) uint16 round the seeds -> (F, P) uint64 sums of weight x
        value of every recorded frame."""
        sd = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
        S = 2 * int(R) + 1
        w = np.ascontiguousarray(weights, np.uint16)
        if w.shape != (sd.shape[0], S, S):
            raise ValueError("weights of shape %r for %d seeds and windows of %d x %d" % (w.shape, sd.shape[0], S, S))
        out = np.empty((self.body_rec_count(), sd.shape[0]), np.uint64)
        _lib.check(_lib.lib().hm_body_rec_weighted_sums(self._h, sd.shape[0], _lib.ptr(sd), int(R), _lib.ptr(w), _lib.ptr(out)),
                   "hm_body_rec_weighted_sums")
        return out

    def body_rec_trace_products(self, seeds, q, R):
        """hm_body_rec_trace_products: one int32 trace per seed, q (F, P) -> (P, 2R+1, 2R+1) int64, the sum over the
        recorded frames of every window pixel times the seed's trace (0 off the frame and outside the map)."""
        sd = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
        S, F = 2 * int(R) + 1, self.body_rec_count()
        q = np.asarray(q)
        if q.dtype != np.int32 or q.ndim != 2 or q.shape[1] != sd.shape[0] or (F and q.shape[0] != F):   # (F 0: the call says why)
            raise ValueError("traces %s of shape %r for %d frames and %d seeds (need int32)" % (q.dtype, q.shape, F, sd.shape[0]))
        q = np.ascontiguousarray(q)
        out = np.empty((sd.shape[0], S, S), np.int64)
        _lib.check(_lib.lib().hm_body_rec_trace_products(self._h, sd.shape[0], _lib.ptr(sd), int(R), _lib.ptr(q), _lib.ptr(out)),
                   "hm_body_rec_trace_products")
        return out

    def body_rec_trace_maps(self, q, want=("c", "w1", "w2")):
        """hm_body_rec_trace_maps: L int32 traces, q (F, L) with |q| <= 32767 -> dict of those in `want`: c (L, H, W) int64,
        the sum over the recorded frames of every pixel times every trace; w1, w2 (H, W) uint64, the sums of every pixel
        and of its square (0 outside the map)."""
        F = self.body_rec_count()
        q = np.asarray(q)
        if q.dtype != np.int32 or q.ndim != 2 or (F and q.shape[0] != F):          # (F 0: the call says why)
            raise ValueError("traces %s of shape %r for %d frames (need int32, frames x traces)" % (q.dtype, q.shape, F))
        q = np.ascontiguousarray(q)
        L, H, W = q.shape[1], self.ny, self.nx
        o = {}
        if "c" in want:
            o["c"] = np.empty((min(max(L, 0), 1024), H, W), np.int64)               # (L out of range: the call says so)
        for key in ("w1", "w2"):
            if key in want:
                o[key] = np.empty((H, W), np.uint64)
        _lib.check(_lib.lib().hm_body_rec_trace_maps(self._h, L, _lib.ptr(q), *[_lib.ptr(o[k]) if k in o else None
                                                                                 for k in ("c", "w1", "w2")]),
                   "hm_body_rec_trace_maps")
        return o

    def body_rec_trace_null(self, q, vb, want=("tmax", "tmin", "ge", "le")):
        """hm_body_rec_trace_null: q (F, L) int32 with |q| <= 32767, column 0 the observed trace and the others its
        surrogates, vb (L,) float64 = F u2 - u1^2 of every column -> dict of those in `want`: tmax, tmin (L,) float64, the
        largest and smallest correlation of every column over the map; ge, le (H, W) uint32, per pixel the surrogates
        whose numerator is >= and <= the observed one (0 outside the map)."""
        F = self.body_rec_count()
        q = np.asarray(q)
        if q.dtype != np.int32 or q.ndim != 2 or (F and q.shape[0] != F):          # (F 0: the call says why)
            raise ValueError("traces %s of shape %r for %d frames (need int32, frames x traces)" % (q.dtype, q.shape, F))
        q = np.ascontiguousarray(q)
        L, H, W = q.shape[1], self.ny, self.nx
        vb = np.ascontiguousarray(vb, np.float64)
        if vb.shape != (L,):
            raise ValueError("vb of shape %r for %d traces" % (vb.shape, L))
        o = {}
        for key in ("tmax", "tmin"):
            if key in want:
                o[key] = np.empty(max(L, 0), np.float64)
        for key in ("ge", "le"):
            if key in want:
                o[key] = np.empty((H, W), np.uint32)
        _lib.check(_lib.lib().hm_body_rec_trace_null(self._h, L, _lib.ptr(q), _lib.ptr(vb),
                                                     *[_lib.ptr(o[k]) if k in o else None for k in ("tmax", "tmin", "ge", "le")]),
                   "hm_body_rec_trace_null")
        return o

    def body_rec_gram(self, k0=0, n=None, stride=1, want=("G", "s1")):
        """hm_body_rec_gram: the frames k0 + i stride, i < n (default: as many as the record holds from k0) -> dict of those
        in `want`: G (n, n) int64, the sum over the pixels of the product of every two of the frames; s1 (n,) uint64, the
        sum of every frame."""
        k0, stride = int(k0), int(stride)
        if n is None:
            F = self.body_rec_count()
            n = (F - 1 - k0) // stride + 1 if stride >= 1 and 0 <= k0 < F else 1          # (out of range: the call says why)
        n = int(n)
        m = min(max(n, 1), 8192)                                                       # (n out of range: the call says so)
        o = {}
        if "G" in want:
            o["G"] = np.empty((m, m), np.int64)
        if "s1" in want:
            o["s1"] = np.empty(m, np.uint64)
        _lib.check(_lib.lib().hm_body_rec_gram(self._h, k0, n, stride, *[_lib.ptr(o[k]) if k in o else None for k in ("G", "s1")]),
                   "hm_body_rec_gram")
        return o

    # -- residual motion of the record (hm_body_rec_match / _frame_sums / _shift / _warp / _field_sums; hydra_mi.stabilize) --
    def body_rec_patches(self, B):
        """-> (patches per row, patch rows) of the grid of B x B patches over the record's box (the bounding box of the
        body map)"""
        box = getattr(self, "_body_rec_box", None)
        if box is None:                                          # (the map is the mesh at X = uv: fixed for the handle)
            m = self.body_map()[0] >= 0
            rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
            box = (int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1) if m.any() else (1, 1)
            self._body_rec_box = box
        B = int(B)
        return (box[0] + B - 1) // B, (box[1] + B - 1) // B

    def body_rec_match(self, template, B, S, k0=0, n=None, want=("A", "V1", "V2")):
        """hm_body_rec_match: template (H, W) uint8 in body coordinates -> dict: n_core (patches,) uint32 and, of A, V1,
        V2, those in `want` as (n, patches, (2S+1)^2) uint32: the sums over every patch's core of v(p + d) t(p),
        v(p + d) and v(p + d)^2 for the frames k0 .. k0 + n - 1 (default: all from k0)."""
        t = self._plane(template, np.uint8, "template")
        B, S = int(B), int(S)
        if not (4 <= B <= 64 and 0 <= S <= 8):                   # (the call says so with its numbers; no grid to size for)
            _lib.check(_lib.lib().hm_body_rec_match(self._h, int(k0), 0, B, S, _lib.ptr(t), None, None, None, None),
                       "hm_body_rec_match")
        n = self._rec_n(k0, n)
        npx, npy = self.body_rec_patches(B)
        o = dict(n_core=np.empty(npx * npy, np.uint32))
        for key in want:
            o[key] = np.empty((max(n, 0), npx * npy, (2 * S + 1) ** 2), np.uint32)
        _lib.check(_lib.lib().hm_body_rec_match(self._h, int(k0), n, B, S, _lib.ptr(t), _lib.ptr(o["n_core"]),
                                                *[_lib.ptr(o.get(key)) for key in ("A", "V1", "V2")]), "hm_body_rec_match")
        return o

    def _body_shifts(self, shifts, B, who):
        sh = np.asarray(shifts)
        if sh.dtype != np.int8 or sh.ndim != 3 or sh.shape[2] != 2:
            raise ValueError("%s: shifts %s of shape %r (need int8, (frames, patches, 2))" % (who, sh.dtype, sh.shape))
        if 4 <= int(B) <= 64:
            npx, npy = self.body_rec_patches(B)
            if sh.shape[1] != npx * npy:
                raise ValueError("%s: shifts for %d patches, the grid of %d px patches has %d" % (who, sh.shape[1], int(B),
                                                                                                  npx * npy))
        return np.ascontiguousarray(sh)

    def body_rec_frame_sums(self, shifts=None, B=16, k0=0, n=None):
        """hm_body_rec_frame_sums: -> (H, W) uint32, the sum over the frames k0 .. k0 + n - 1 of every map pixel taken at
        its patch's shift of that frame; shifts (n, patches, 2) int8 (dx, dy), None: no shift."""
        n = self._rec_n(k0, n)
        sh = None
        if shifts is not None:
            sh = self._body_shifts(shifts, B, "body_rec_frame_sums")
            if sh.shape[0] != n:
                raise ValueError("body_rec_frame_sums: shifts of %d frames for %d" % (sh.shape[0], n))
        out = np.empty((self.ny, self.nx), np.uint32)
        _lib.check(_lib.lib().hm_body_rec_frame_sums(self._h, int(k0), n, int(B), _lib.ptr(sh), _lib.ptr(out)),
                   "hm_body_rec_frame_sums")
        return out

    def body_rec_shift(self, shifts, B):
        """hm_body_rec_shift: rewrite the record in place, every map pixel of every frame taken at its patch's shift;
        shifts (F, patches, 2) int8 (dx, dy) for all recorded frames.  Not reversible."""
        sh = self._body_shifts(shifts, B, "body_rec_shift")
        F = self.body_rec_count()
        if F and sh.shape[0] != F:                               # (F 0: the call says why)
            raise ValueError("body_rec_shift: shifts of %d frames for a record of %d" % (sh.shape[0], F))
        _lib.check(_lib.lib().hm_body_rec_shift(self._h, int(B), _lib.ptr(sh)), "hm_body_rec_shift")

    def _body_field(self, q, valid, B, who):
        q, valid = np.asarray(q), np.asarray(valid)
        if q.dtype != np.int16 or q.ndim != 3 or q.shape[2] != 2:
            raise ValueError("%s: q %s of shape %r (need int16, (frames, patches, 2))" % (who, q.dtype, q.shape))
        if valid.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)) or valid.shape != q.shape[:2]:
            raise ValueError("%s: valid %s of shape %r for q of shape %r (need uint8 or bool, (frames, patches))" % (
                who, valid.dtype, valid.shape, q.shape))
        if 4 <= int(B) <= 64:
            npx, npy = self.body_rec_patches(B)
            if q.shape[1] != npx * npy:
                raise ValueError("%s: q for %d patches, the grid of %d px patches has %d" % (who, q.shape[1], int(B), npx * npy))
        return np.ascontiguousarray(q), np.ascontiguousarray(valid, np.uint8)

    def body_rec_field_sums(self, q, valid, B, k0=0, n=None):
        """hm_body_rec_field_sums: -> (H, W) uint32, the sum over the frames k0 .. k0 + n - 1 of every map pixel sampled at
        the smooth field of that frame; q (n, patches, 2) int16 (dx, dy) in 1/16 px, valid (n, patches)."""
        n = self._rec_n(k0, n)
        q, valid = self._body_field(q, valid, B, "body_rec_field_sums")
        if q.shape[0] != n:
            raise ValueError("body_rec_field_sums: q of %d frames for %d" % (q.shape[0], n))
        out = np.empty((self.ny, self.nx), np.uint32)
        _lib.check(_lib.lib().hm_body_rec_field_sums(self._h, int(k0), n, int(B), _lib.ptr(q), _lib.ptr(valid), _lib.ptr(out)),
                   "hm_body_rec_field_sums")
        return out

    def body_rec_warp(self, q, valid, B):
        """hm_body_rec_warp: rewrite the record in place, every map pixel of every frame sampled bilinearly at the smooth
        field between the patches' shifts; q (F, patches, 2) int16 (dx, dy) in 1/16 px, valid (F, patches), for all
        recorded frames.  Not reversible."""
        q, valid = self._body_field(q, valid, B, "body_rec_warp")
        F = self.body_rec_count()
        if F and q.shape[0] != F:                                # (F 0: the call says why)
            raise ValueError("body_rec_warp: q of %d frames for a record of %d" % (q.shape[0], F))
        _lib.check(_lib.lib().hm_body_rec_warp(self._h, int(B), _lib.ptr(q), _lib.ptr(valid)), "hm_body_rec_warp")

    # -- the record against the deformation of its own tissue (hm_body_rec_tri_maps / _tri_gain; hydra_mi.deform) --
    def _tri_table(self, a, dtype, who):
        """-> `a` as a contiguous (F, T) array of exactly `dtype`, one row per recorded frame and a column per triangle"""
        a = np.asarray(a)
        F, T = self.body_rec_count(), self.tri.shape[0]
        if a.dtype != dtype or a.ndim != 2 or a.shape[1] != T or (F and a.shape[0] != F):     # (F 0: the call says why)
            raise ValueError("%s: %s of shape %r for %d frames and %d triangles (need %s, frames x triangles)" % (
                who, a.dtype, a.shape, F, T, np.dtype(dtype).name))
        return np.ascontiguousarray(a)

    def body_rec_tri_maps(self, q, want=("c", "w1", "w2")):
        """hm_body_rec_tri_maps: one int32 trace per triangle, q (F, T) with |q| <= 32767 -> (c, w1, w2): c (H, W) int64, the
        sum over the recorded frames of every pixel times the trace of its own triangle; w1, w2 (H, W) uint64, the sums of
        every pixel and of its square (0 outside the map); None for one that is not in `want`."""
        q = self._tri_table(q, np.int32, "body_rec_tri_maps")
        H, W = self.ny, self.nx
        o = {"c": np.empty((H, W), np.int64) if "c" in want else None}
        for key in ("w1", "w2"):
            o[key] = np.empty((H, W), np.uint64) if key in want else None
        _lib.check(_lib.lib().hm_body_rec_tri_maps(self._h, q.shape[1], _lib.ptr(q), _lib.ptr(o["c"]), _lib.ptr(o["w1"]),
                                                   _lib.ptr(o["w2"])), "hm_body_rec_tri_maps")
        return o["c"], o["w1"], o["w2"]

    def body_rec_tri_gain(self, m):
        """hm_body_rec_tri_gain: rewrite the record in place, every map pixel of every frame times the gain of its own
        triangle in that frame, min(255, (v m + 2048) >> 12); m (F, T) uint16, 4096 the identity -> the number of values
        that were clipped at 255.  Not reversible."""
        m = self._tri_table(m, np.uint16, "body_rec_tri_gain")
        n = ctypes.c_uint64(0)
        _lib.check(_lib.lib().hm_body_rec_tri_gain(self._h, m.shape[1], _lib.ptr(m), ctypes.byref(n)), "hm_body_rec_tri_gain")
        return int(n.value)

    # -- the running baseline per pixel of the record (hm_body_rec_planes / _stats_add; hydra_mi.detrend) -----
    PLANES = {"recorded": 0, "baseline": 1, "excess": 2, "dff": 3}

    def body_rec_planes(self, what, half, q, floor=1, gain=1, k0=0, n=None):
        """hm_body_rec_planes: -> (n, H, W) uint8, the planes of kind `what` ("recorded", "baseline", "excess", "dff", or
        0..3) of the recorded frames k0 .. k0 + n - 1 (default: all from k0): the baseline is the value at rank
        q (window - 1) // 100 of the frames k - half .. k + half of the whole record, the excess what lies above it, dff
        min(255, gain excess // max(baseline, floor))."""
        what = self.PLANES[what] if isinstance(what, str) else int(what)
        n = self._rec_n(k0, n)
        out = np.empty((max(n, 0), self.ny, self.nx), np.uint8)
        _lib.check(_lib.lib().hm_body_rec_planes(self._h, int(k0), n, what, int(half), int(q), int(floor), int(gain),
                                                 _lib.ptr(out)), "hm_body_rec_planes")
        return out

    def body_rec_stats_add(self, what, half, q, floor=1, gain=1):
        """hm_body_rec_stats_add: add every recorded frame's plane of kind `what` (as body_rec_planes) to the statistics
        begun with body_stats_begin, as if each had just been warped."""
        what = self.PLANES[what] if isinstance(what, str) else int(what)
        _lib.check(_lib.lib().hm_body_rec_stats_add(self._h, what, int(half), int(q), int(floor), int(gain)),
                   "hm_body_rec_stats_add")

    # -- events per pixel of the record: AR(1) deconvolution of the planes (hm_body_rec_event_*; hydra_mi.events) -----
    def body_rec_event_planes(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0, k0=0, n=None):
        """hm_body_rec_event_planes: -> (n, H, W) uint8, the event bytes min(255, floor(s + 0.5)) of the recorded frames
        k0 .. k0 + n - 1 (default: all from k0): s the AR(1) deconvolution (decay g per frame, penalty lam) of every
        pixel's planes of kind `what` (as body_rec_planes) over the whole record."""
        what = self.PLANES[what] if isinstance(what, str) else int(what)
        n = self._rec_n(k0, n)
        out = np.empty((max(n, 0), self.ny, self.nx), np.uint8)
        _lib.check(_lib.lib().hm_body_rec_event_planes(self._h, int(k0), n, what, int(half), int(q), int(floor), int(gain),
                                                       float(g), float(lam), _lib.ptr(out)), "hm_body_rec_event_planes")
        return out

    def body_rec_event_stats_add(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0):
        """hm_body_rec_event_stats_add: add every recorded frame's event plane (as body_rec_event_planes) to the statistics
        begun with body_stats_begin, as if each had just been warped."""
        what = self.PLANES[what] if isinstance(what, str) else int(what)
        _lib.check(_lib.lib().hm_body_rec_event_stats_add(self._h, what, int(half), int(q), int(floor), int(gain), float(g),
                                                          float(lam)), "hm_body_rec_event_stats_add")

    def body_rec_event_sums(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0, s_min=1.0):
        """hm_body_rec_event_sums: -> (count (H, W) uint32, sum (H, W) float64): per pixel the number of frames with
        s >= s_min and the sum of s over the record (s as in body_rec_event_planes, before rounding)."""
        what = self.PLANES[what] if isinstance(what, str) else int(what)
        count, total = np.empty((self.ny, self.nx), np.uint32), np.empty((self.ny, self.nx), np.float64)
        _lib.check(_lib.lib().hm_body_rec_event_sums(self._h, what, int(half), int(q), int(floor), int(gain), float(g), float(lam),
                                                     float(s_min), _lib.ptr(count), _lib.ptr(total)), "hm_body_rec_event_sums")
        return count, total

    # -- the residual of the record under a model of the cells (hm_body_rec_residual_*; hydra_mi.residual) -----
    def _residual_args(self, who, labels, weights, traces, blank):
        lab = np.ascontiguousarray(labels, np.int32)
        lab = lab[None] if lab.ndim == 2 else lab
        if lab.ndim != 3 or lab.shape[1:] != (self.ny, self.nx):
            raise ValueError("%s: label planes of shape %r for %dx%d frames" % (who, lab.shape, self.nx, self.ny))
        w = None if weights is None else np.ascontiguousarray(weights, np.uint16)
        if w is not None and w.size != lab.size:
            raise ValueError("%s: weights of shape %r for labels of shape %r" % (who, w.shape, lab.shape))
        tr = np.ascontiguousarray(traces, np.int32)
        F = self.body_rec_count()
        if tr.ndim != 2 or (F and tr.shape[0] != F):             # (F 0: the call says why)
            raise ValueError("%s: traces of shape %r for a record of %d frames" % (who, tr.shape, F))
        bl = None if blank is None else self._plane(blank, np.uint8, "%s: a blank plane" % who)
        return lab, w, tr, bl

    def body_rec_residual_planes(self, labels, weights, traces, blank=None, offset=64, k0=0, n=None):
        """hm_body_rec_residual_planes: -> ((n, H, W) uint8, clipped): the recorded frames k0 .. k0 + n - 1 (default: all
        from k0) minus the cells' light, min(255, max(0, offset + v - ((sum_j weights[j] traces[k, labels[j]] + 2^23) >>
        24))), 0 off the map and where blank is set.  labels (n_layers, H, W) or (H, W) int32 (-1: none), weights the
        same shape uint16 (None: 65535), as view_set_cells takes them; traces (F, L) int32 for all recorded frames."""
        lab, w, tr, bl = self._residual_args("body_rec_residual_planes", labels, weights, traces, blank)
        n = self._rec_n(k0, n)
        out = np.empty((max(n, 0), self.ny, self.nx), np.uint8)
        clipped = ctypes.c_uint64(0)
        _lib.check(_lib.lib().hm_body_rec_residual_planes(self._h, int(k0), n, int(lab.shape[0]), _lib.ptr(lab), _lib.ptr(w),
                                                          int(tr.shape[1]), _lib.ptr(tr), _lib.ptr(bl), int(offset),
                                                          _lib.ptr(out), ctypes.byref(clipped)), "hm_body_rec_residual_planes")
        return out, clipped.value

    def body_rec_residual_stats_add(self, labels, weights, traces, blank=None, offset=64):
        """hm_body_rec_residual_stats_add: add every recorded frame's residual plane (as body_rec_residual_planes) to the
        statistics begun with body_stats_begin, as if each had just been warped -> clipped."""
        lab, w, tr, bl = self._residual_args("body_rec_residual_stats_add", labels, weights, traces, blank)
        clipped = ctypes.c_uint64(0)
        _lib.check(_lib.lib().hm_body_rec_residual_stats_add(self._h, int(lab.shape[0]), _lib.ptr(lab), _lib.ptr(w),
                                                             int(tr.shape[1]), _lib.ptr(tr), _lib.ptr(bl), int(offset),
                                                             ctypes.byref(clipped)), "hm_body_rec_residual_stats_add")
        return clipped.value

    def screenshot(self, saveall=True, basename="screenshot", X=None):
        """reference renderer.py:436-475: writes <basename>_<view>.png for flowx, flowy, raw, overlay, texture and mask
        at state X (default: the vertex buffer) and returns the overlay.  Unlike the reference the names carry no
        time stamp: a second call with the same basename overwrites.  saveall=False writes the overlay alone."""
        from .videoio import write_png
        views = ("flowx", "flowy", "raw", "overlay", "texture", "mask") if saveall else ("overlay",)
        overlay = None
        for v in views:
            img = self.view(X, v)
            write_png("%s_%s.png" % (basename, v), img)
            if v == "overlay":
                overlay = img
        return overlay

    # -- observation ------------------------------------------------------------------------
    def update_frame(self, y_im, y_flow, y_m):
        """reference renderer.py:656-664: the frame compute() works on.  Uploaded once."""
        self.set_observation(y_im, y_flow, y_m)

    def set_observation(self, y_im, y_flow, y_m):
        y_im = np.asarray(y_im)
        if y_im.ndim == 3:
            y_im = y_im[:, :, 0]
        a = np.ascontiguousarray(y_im, np.uint8)
        fx = np.ascontiguousarray(y_flow[:, :, 0], np.float32)
        fy = np.ascontiguousarray(y_flow[:, :, 1], np.float32)
        m = np.ascontiguousarray(y_m, np.uint8)
        if a.shape != (self.ny, self.nx) or fx.shape != a.shape or m.shape != a.shape:
            raise ValueError("observation arrays must be %dx%d" % (self.ny, self.nx))
        _lib.check(_lib.lib().hm_set_observation(self._h, _lib.ptr(a), _lib.ptr(fx), _lib.ptr(fy), _lib.ptr(m)),
                   "hm_set_observation")
        self._obs = (y_im, y_flow, y_m)

    def set_observation_dev(self, obs):
        """A DeviceObservation: frame, flow planes (e.g. what hm_brox_calc_dev just wrote) and mask
        already in device memory.  The caller keeps them alive and ordered before this call."""
        _lib.check(_lib.lib().hm_set_observation_dev(self._h, int(obs.d_y_im), int(obs.d_flowx), int(obs.d_flowy),
                                                     int(obs.d_y_m)), "hm_set_observation_dev")
        self._obs = obs

    def _masked_flag(self, y_im, y_flow, y_m):
        """Which of the two device copies of the observed flow an operator uses (0 raw, 1 mask-multiplied),
        uploading the arrays first unless they are known to be the observation in place.

        The reference's operators always work on the arrays they are given (renderer.py:485-501, 674-679).
        Host arrays are therefore uploaded on every call -- a caller may have refilled its buffers in
        place -- except inside KalmanFilter.compute(), which has just uploaded them itself
        (``frame_in_place``): there the arrays are recognised by identity and the copies are skipped."""
        o = self._obs
        if isinstance(y_im, DeviceObservation):
            if o is not y_im:
                self.set_observation_dev(y_im)
            return 1 if y_flow is y_im.masked else 0
        if self.frame_in_place and o is not None and len(o) == 3 and y_im is o[0] and y_m is o[2]:
            if y_flow is o[1]:
                return 0
            if getattr(y_flow, "_hm_masked_from", None) is o[1]:
                return 1
        raw = getattr(y_flow, "_hm_masked_from", None)
        if raw is not None:                       # a MaskedFlow: upload the flow it was made from, use the masked copy
            self.set_observation(y_im, raw, y_m)
            return 1
        self.set_observation(y_im, y_flow, y_m)
        return 0

    # -- the reference's operator interface ---------------------------------------------------
    def initjacobian(self, y_im, y_flow, y_m):
        """reference renderer.py:674-679 / cuda.py:940-950: current render becomes the reference."""
        self._masked = self._masked_flag(y_im, y_flow, y_m)
        _lib.check(_lib.lib().hm_initjacobian(self._h, _lib.ptr(self._X()), self._masked), "hm_initjacobian")

    def jz(self, state=None):
        """reference renderer.py:681-694 / cuda.py:972-980 -> (jz, [im, fx, fy, m] components)."""
        out = ctypes.c_double()
        comp = (ctypes.c_double * 4)()
        _lib.check(_lib.lib().hm_jz(self._h, _lib.ptr(self._X(state)), getattr(self, "_masked", 0),
                                    ctypes.byref(out), comp), "hm_jz")
        return out.value, np.array(comp[:])

    def _labels_now(self, who):
        if getattr(self, "_palette", None) is None:
            raise RuntimeError("%s: no label palette selected (update_vertex_buffer / KFState.refresh with the "
                               "partition index first, reference kalman.py:459, 545)" % who)
        return self._palette

    def jz_multi(self, state):
        """reference renderer.py:696-709 / cuda_multi.py:721-845 -> (hz [N,1], hzc [N,4]): the terms of jz summed
        per vertex label of the palette in place (hm_jz_multi)."""
        lab = self._labels_now("jz_multi")
        hz = np.zeros(self.n)
        hzc = np.zeros((self.n, 4))
        _lib.check(_lib.lib().hm_jz_multi(self._h, _lib.ptr(self._X(state)), getattr(self, "_masked", 0), _lib.ptr(lab),
                                          self.n, _lib.ptr(hz), _lib.ptr(hzc)), "hm_jz_multi")
        return hz.reshape(-1, 1), hzc

    def j(self, state, deltaX, i, j):
        """reference renderer.py:711-721 / cuda.py:982-1010."""
        out = ctypes.c_double()
        _lib.check(_lib.lib().hm_j(self._h, _lib.ptr(self._X(state)), float(deltaX), int(i), int(j),
                                   ctypes.byref(out)), "hm_j")
        return out.value

    def j_multi(self, state, deltaX, ee, labelidx, ee_idx=None):
        """reference renderer.py:723-737 / cuda_multi.py:979-1129 -> (h [1,|Q|], nz [|Q|] bool, hcomp [|Q|,4]): the
        terms of j for the pairs ee (|e| x 2 state indices, all perturbed at once) summed per pair label of the
        hessian palette `labelidx` (hm_j_multi)."""
        lab = np.ascontiguousarray(np.asarray(self.labels_hess)[:, labelidx], np.int32)
        ee = np.ascontiguousarray(np.asarray(ee).reshape(-1, 2), np.int32)
        nq = len(self.Q)
        h = np.zeros(nq)
        nz = np.zeros(nq)
        hc = np.zeros((nq, 4))
        _lib.check(_lib.lib().hm_j_multi(self._h, _lib.ptr(self._X(state)), float(deltaX), int(ee.shape[0]), _lib.ptr(ee),
                                         _lib.ptr(lab), nq, _lib.ptr(h), _lib.ptr(nz), _lib.ptr(hc)), "hm_j_multi")
        return h.reshape(1, -1), nz > 0, hc

    def measure(self, state, y_im, y_flow, y_m, deltaX=2.0):
        """KFState.update (kalman.py:437-449) fused: -> (Hz [4N,1], HTH [4N,4N], Hz_components [4N,4])."""
        masked = self._masked_flag(y_im, y_flow, y_m)
        n4 = 4 * self.n
        Hz = np.empty(n4)
        Hzc = np.empty((n4, 4))
        HTH = np.empty((n4, n4))
        _lib.check(_lib.lib().hm_measure(self._h, _lib.ptr(self._X(state)), float(deltaX), masked, _lib.ptr(Hz),
                                         _lib.ptr(Hzc), _lib.ptr(HTH)), "hm_measure")
        return Hz.reshape(-1, 1), HTH, Hzc

    # -- the dense update on the device (information form) --------------------------------------
    def _cov_arg(self, W, who):
        """NULL for the covariance resident on the device, else a contiguous host array."""
        if isinstance(W, DeviceCovariance):
            if not W.valid(self):
                raise RuntimeError("%s: this DeviceCovariance is no longer resident on the device" % who)
            return None
        return np.ascontiguousarray(W, np.float64)

    def _cov_result(self, fetch):
        self._cov_serial += 1
        tok = DeviceCovariance(self, self._cov_serial)
        return tok.fetch() if fetch else tok

    def tune(self, key, value):
        if -2 ** 31 <= int(value) < 2 ** 31:
            _lib.check(_lib.lib().hm_ctx_tune(self._h, key.encode(), int(value)), "hm_ctx_tune")
        else:                                                    # ("rec_ev_bytes" reaches 2^34)
            _lib.check(_lib.lib().hm_ctx_tune64(self._h, key.encode(), int(value)), "hm_ctx_tune")

    def project_mask(self, X, y_m=None):
        """KalmanFilter.projectmask (kalman.py:724-742) on the device -> (X projected, number of
        vertices that were outside).  y_m: host mask, or None for the mask of the observation in place."""
        Xp = np.array(X, np.float64).reshape(-1)
        if Xp.shape[0] != 4 * self.n:
            raise ValueError("state of %d entries for a mesh of %d vertices" % (Xp.shape[0], self.n))
        mask = None
        if y_m is not None:
            mask = np.ascontiguousarray(np.asarray(y_m) > 0.5).view(np.uint8)
            if mask.shape != (self.ny, self.nx):
                raise ValueError("mask of shape %r for frames of %r" % (mask.shape, (self.ny, self.nx)))
        moved = ctypes.c_int(0)
        _lib.check(_lib.lib().hm_project_mask(self._h, _lib.ptr(mask), _lib.ptr(Xp), ctypes.byref(moved)),
                   "hm_project_mask")
        return Xp.reshape(np.shape(X)), moved.value

    def prune_mask(self, y_m):
        """hm_prune_mask: the reference's contour pruning of a mask (imgproc.py:198-228) as project_mask applies it."""
        mask = np.ascontiguousarray(np.asarray(y_m) > 0.5).view(np.uint8)
        if mask.shape != (self.ny, self.nx):
            raise ValueError("mask of shape %r for frames of %r" % (mask.shape, (self.ny, self.nx)))
        out = np.empty_like(mask)
        _lib.check(_lib.lib().hm_prune_mask(self._h, _lib.ptr(mask), _lib.ptr(out)), "hm_prune_mask")
        return out

    def cov_fetch(self):
        n4 = 4 * self.n
        W = np.empty((n4, n4))
        _lib.check(_lib.lib().hm_cov_fetch(self._h, _lib.ptr(W)), "hm_cov_fetch")
        return W

    def cov_predict(self, W, bars, blocks, a, s, eps_F, fetch=True):
        """hm_cov_predict: F W F^T + Weps on the device.  W is a host array or the DeviceCovariance
        the last update left on the device; fetch=False returns a DeviceCovariance instead of
        copying 4N x 4N doubles back."""
        Win = self._cov_arg(W, "cov_predict")
        nb = 0 if bars is None else int(len(bars))
        b = None if nb == 0 else np.ascontiguousarray(bars, np.int32)
        blk = None if nb == 0 else np.ascontiguousarray(blocks, np.float64)
        _lib.check(_lib.lib().hm_cov_predict(self._h, _lib.ptr(Win), nb, _lib.ptr(b), _lib.ptr(blk), float(a), float(s),
                                             float(eps_F), None), "hm_cov_predict")
        return self._cov_result(fetch)

    def ms_predict(self, W, X, bars, l0, kappa, M, dt, maxiter, tol, eps_F, prefactor=True):
        """hm_ms_predict: IteratedMSKalmanFilter.predict (kalman.py:850-863) for the DeviceCovariance W in one native
        call -> (X predicted [4N,1], Newton iterations, DeviceCovariance of the predicted covariance)."""
        if self._cov_arg(W, "ms_predict") is not None:
            raise TypeError("ms_predict takes the DeviceCovariance resident on the device")
        Xp = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1)).copy()
        b = np.ascontiguousarray(bars, np.int32)
        l0 = np.ascontiguousarray(np.asarray(l0, np.float64).reshape(-1))
        its = ctypes.c_int()
        _lib.check(_lib.lib().hm_ms_predict(self._h, int(b.shape[0]), _lib.ptr(b), _lib.ptr(l0), float(kappa), float(M),
                                            float(dt), int(maxiter), float(tol), float(eps_F), _lib.ptr(Xp),
                                            ctypes.byref(its), 1 if prefactor else 0), "hm_ms_predict")
        return Xp.reshape(-1, 1), its.value, self._cov_result(False)

    def update_prefactor(self, W):
        """hm_update_prefactor: queue the factorisation / inversion of the DeviceCovariance W now (it
        does not need the predicted state); the next update_begin / update_run with W picks it up."""
        if self._cov_arg(W, "update_prefactor") is not None:
            raise TypeError("update_prefactor takes the DeviceCovariance resident on the device")
        _lib.check(_lib.lib().hm_update_prefactor(self._h), "hm_update_prefactor")

    def update_begin(self, W_prior, X0):
        """Factor the prior covariance on the device and keep inv(W), X0 there (hm_update_begin).
        A DeviceCovariance is used where it is."""
        W = self._cov_arg(W_prior, "update_begin")
        x0 = np.ascontiguousarray(np.asarray(X0, np.float64).reshape(-1))
        _lib.check(_lib.lib().hm_update_begin(self._h, _lib.ptr(W), _lib.ptr(x0)), "hm_update_begin")
        if W is not None:
            self._cov_serial += 1

    def update_run(self, W_prior, X0, y_im, y_flow, y_m, max_iter, reltol, deltaX=2.0, fetch=False, tail=True):
        """hm_update_run: the whole iterated update (kalman.py:774-831) ->
        (X kept [4N,1], info dict, errs [niter,4], Hz_components [4N,4], gains [3,4N], covariance).
        tail=False: the call does not wait for the kernels that form the Hz components and the gains (None in their place);
        update_tail() fetches them, until the next update_run."""
        masked = self._masked_flag(y_im, y_flow, y_m)
        W = self._cov_arg(W_prior, "update_run")
        n4 = 4 * self.n
        X = np.ascontiguousarray(np.asarray(X0, np.float64).reshape(-1)).copy()
        info = (ctypes.c_int * 4)()
        errs = np.zeros((max(int(max_iter), 1), 4))
        Hzc = np.empty((n4, 4)) if tail else None
        gains = np.empty((3, n4)) if tail else None
        rc = _lib.lib().hm_update_run(self._h, _lib.ptr(W), _lib.ptr(X), float(deltaX), masked, int(max_iter),
                                      float(reltol), info, _lib.ptr(errs), _lib.ptr(Hzc), _lib.ptr(gains), None)
        if rc == 2:                                 # a chained run whose state prediction gave up: the caller predicts on the host
            raise ChainedPredictionFailed()         # (nothing was updated: the predicted covariance is still the resident one)
        self._cov_serial += 1
        if rc == _lib.HM_ERR_NUMERIC:
            raise FloatingPointError(_lib.lib().hm_last_error().decode())
        _lib.check(rc, "hm_update_run")
        out = dict(niter=info[0], accepted=info[1], reverted=bool(info[2]), converged=bool(info[3]))
        return X.reshape(-1, 1), out, errs[:info[0]], Hzc, gains, self._cov_result(fetch)

    def arm_newton(self, worker, bars, l0, kappa, M, dt, maxiter, tol):
        """hm_update_arm_newton: the next update_run starts hm_ms_newton on `worker` with the state it ends with, as
        soon as that state is known."""
        bars = np.ascontiguousarray(bars, np.int32)
        l0 = np.ascontiguousarray(l0, np.float64)
        _lib.check(_lib.lib().hm_update_arm_newton(self._h, worker, int(bars.shape[0]), _lib.ptr(bars), _lib.ptr(l0),
                                                   float(kappa), float(M), float(dt), int(maxiter), float(tol)),
                   "hm_update_arm_newton")

    def attach_worker(self, worker, on=True):
        """hm_ms_worker_attach: the state predictions started on `worker` run as a launch on this renderer's device."""
        _lib.check(_lib.lib().hm_ms_worker_attach(worker, self._h if on else None), "hm_ms_worker_attach")
        self._worker = worker if on else None

    def detach_worker(self, worker):
        """(the worker is about to be destroyed)"""
        if self._worker is not None and self._h is not None:
            _lib.lib().hm_ms_worker_attach(worker, None)
        self._worker = None

    def chain_project(self):
        """hm_chain_project: projectmask of the state prediction in flight queued behind it, its result the prior mean
        of the next update_run (whose X0 is then ignored) -- True when queued, False when there is nothing to chain."""
        rc = _lib.lib().hm_chain_project(self._h)
        if rc == 1:
            return False
        _lib.check(rc, "hm_chain_project")
        return True

    def update_tail(self):
        """hm_update_tail -> (Hz components [4N,4], gains [3,4N]) of the last update_run(tail=False)."""
        n4 = 4 * self.n
        Hzc, gains = np.empty((n4, 4)), np.empty((3, n4))
        _lib.check(_lib.lib().hm_update_tail(self._h, _lib.ptr(Hzc), _lib.ptr(gains)), "hm_update_tail")
        return Hzc, gains

    def arm_mask(self, d_mask):
        """hm_update_arm_mask: the next update_run queues the outline of this mask (device address: the NEXT frame's) when
        its state is final."""
        _lib.check(_lib.lib().hm_update_arm_mask(self._h, ctypes.c_void_p(int(d_mask))), "hm_update_arm_mask")

    def prepare_mask(self, d_mask):
        """hm_prepare_mask: pruning + outline of the NEXT observation's mask (device address) queued a frame ahead.
        None discards the preparation (before the memory of the prepared mask is given another mask)."""
        p = None if d_mask is None else ctypes.c_void_p(int(d_mask))
        _lib.check(_lib.lib().hm_prepare_mask(self._h, p), "hm_prepare_mask")

    def chain_states(self):
        """hm_chain_states -> (predicted state, projected state, Newton iterations, vertices moved) of the last chained
        update_run."""
        n4 = 4 * self.n
        pred, proj = np.empty(n4), np.empty(n4)
        its, moved = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.lib().hm_chain_states(self._h, _lib.ptr(pred), _lib.ptr(proj), ctypes.byref(its), ctypes.byref(moved)),
                   "hm_chain_states")
        return pred, proj, its.value, moved.value

    def arm_cov(self, eps_F):
        """hm_update_arm_cov: the next update_run (armed with arm_newton as well) also queues the covariance half of the
        next frame's prediction -- cov_predict at the state it ends with, then update_prefactor -- behind its own last
        launches; predict_take makes them current."""
        _lib.check(_lib.lib().hm_update_arm_cov(self._h, float(eps_F)), "hm_update_arm_cov")

    def predict_take(self, W, X, bars, l0, kappa, a, s, eps_F):
        """hm_predict_take: the DeviceCovariance of the prediction update_run queued ahead from the resident covariance W,
        if it was made from exactly these inputs (its factorisation for the next update is queued as well, as after
        update_prefactor) -- else None, and the caller calls cov_predict / update_prefactor itself."""
        if not (isinstance(W, DeviceCovariance) and W.valid(self)):
            return None
        x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        b = np.ascontiguousarray(bars, np.int32)
        l0 = np.ascontiguousarray(np.asarray(l0, np.float64).reshape(-1))
        rc = _lib.lib().hm_predict_take(self._h, _lib.ptr(x), int(b.shape[0]), _lib.ptr(b), _lib.ptr(l0), float(kappa),
                                        float(a), float(s), float(eps_F))
        if rc == 1:
            return None
        _lib.check(rc, "hm_predict_take")
        return self._cov_result(False)

    def update_step(self, state, y_im, y_flow, y_m, deltaX=2.0, want_error=True):
        """hm_update_step: measurement at state.X, the solve and (want_error) Renderer.error of the new
        iterate X0 + step -> (step [4N,1], Hz_components [4N,4], (e_im, e_fx, e_fy, e_m) or None)."""
        masked = self._masked_flag(y_im, y_flow, y_m)
        n4 = 4 * self.n
        step = np.empty(n4)
        Hzc = np.empty((n4, 4))
        err = (ctypes.c_double * 4)()
        _lib.check(_lib.lib().hm_update_step(self._h, _lib.ptr(self._X(state)), float(deltaX), masked,
                                             _lib.ptr(step), _lib.ptr(Hzc), err if want_error else None),
                   "hm_update_step")
        e = (int(err[0]), err[1], err[2], int(err[3])) if want_error else None
        return step.reshape(-1, 1), Hzc, e

    def update_cov(self, which=0, fetch=True):
        """hm_update_cov: covariance of the last step (0), of the one before (1) or the prior (-1)."""
        _lib.check(_lib.lib().hm_update_cov(self._h, int(which), None), "hm_update_cov")
        return self._cov_result(fetch)

    def error(self, state, y_im, y_flow, y_m, want_flow=True):
        """reference renderer.py:485-501 -> (e_im, e_fx, e_fy, e_m, fx, fy).

        want_flow=False skips the device-to-host copy of the two rendered flow planes (the IEKF
        loop only looks at the four sums); fx, fy are then None."""
        masked = self._masked_flag(y_im, y_flow, y_m)
        err = (ctypes.c_double * 4)()
        fx = fy = None
        if not want_flow and not masked:
            # the state an update_run has just kept: the sums came out of the render of its last iterate
            rc = _lib.lib().hm_update_last_error(self._h, _lib.ptr(self._X(state)), err)
            if rc == 0:
                return int(err[0]), err[1], err[2], int(err[3]), None, None
            if rc < 0:
                _lib.check(rc, "hm_update_last_error")
        if want_flow:
            fx = np.empty((self.ny, self.nx), np.float32)
            fy = np.empty_like(fx)
        _lib.check(_lib.lib().hm_error(self._h, _lib.ptr(self._X(state)), masked, err, _lib.ptr(fx), _lib.ptr(fy)),
                   "hm_error")
        if want_flow:      # the reference returns read_pixels arrays of shape (ny, nx, 1)
            fx, fy = fx[:, :, None], fy[:, :, None]
        return int(err[0]), err[1], err[2], int(err[3]), fx, fy


class DeviceCovariance:
    """A 4N x 4N covariance that lives on the device: what the last cov_predict / update_cov /
    update_run of one Renderer left there.  fetch() copies it to the host; it stops being valid
    when that renderer produces the next one."""

    def __init__(self, renderer, serial):
        self._renderer, self._serial = renderer, serial

    def valid(self, renderer=None):
        r = self._renderer
        return (renderer is None or renderer is r) and r._cov_serial == self._serial

    def fetch(self):
        if not self.valid():
            raise RuntimeError("this DeviceCovariance is no longer resident on the device")
        return self._renderer.cov_fetch()


class DeviceObservation:
    """One observed frame held in device memory (addresses as integers): u8 frame, f32 flow x / y,
    u8 mask in {0,1}, all W*H row-major.  ``raw`` and ``masked`` are the tokens to pass as y_flow."""

    class _Token:
        def __init__(self, name):
            self.name = name

    def __init__(self, d_y_im, d_flowx, d_flowy, d_y_m, y_m_host=None, next_mask=None):
        self.d_y_im, self.d_flowx, self.d_flowy, self.d_y_m = d_y_im, d_flowx, d_flowy, d_y_m
        self.y_m_host = y_m_host
        self.next_mask = next_mask      # device address of the NEXT frame's mask when it is resident already (hm_prepare_mask)
        self.raw = DeviceObservation._Token("raw")
        self.masked = DeviceObservation._Token("masked")


class MaskedFlow(np.ndarray):
    """y_m * y_flow (kalman.py:679-682) that remembers the raw flow it was made from, so the
    renderer can use the device-side product instead of uploading the frame a second time."""

    def __new__(cls, y_flow, y_m):
        out = np.dstack((y_m * y_flow[:, :, 0], y_m * y_flow[:, :, 1])).astype(np.float32).view(cls)
        out._hm_masked_from = y_flow
        return out

    def __array_finalize__(self, obj):
        self._hm_masked_from = getattr(obj, "_hm_masked_from", None)


class FlowStream:
    """reference renderer.py:807-874: flow frames <path>_%03d_x.mat / _y.mat."""

    def __init__(self, path):
        self.path = path
        self.frame = 0

    def _names(self):
        return (self.path + "_%03d_x.mat" % self.frame, self.path + "_%03d_y.mat" % self.frame)

    def peek(self):
        fn_x, fn_y = self._names()
        try:
            self.flowx = matio.read_mat(fn_x)
            self.flowy = matio.read_mat(fn_y)
        except IOError:
            return False, None
        return True, np.dstack((self.flowx, self.flowy)).astype(np.float32)

    def read(self):
        ret, flow = self.peek()
        self.frame += 1
        return ret, flow

    def isOpened(self):
        fn_x, fn_y = self._names()
        return os.path.isfile(fn_x) and os.path.isfile(fn_y)
