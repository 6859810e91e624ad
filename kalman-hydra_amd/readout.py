"""The readout half of ``renderer.Renderer``, the Python side of csrc/readout.hip: the views, the body-frame readout, the
strain readout and the statistics of the registered video (the kept record is in ``record.Record``).  ``Readout`` is a
class of methods that ``Renderer`` inherits: it reads the handle ``_h`` and what ``Renderer.__init__`` sets.
"""
import ctypes

import numpy as np

from . import _lib
from .videoio import VIEWS, write_png


class Readout:
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
            if lv.shape[0] != self._cells_L:                   # (the library reads L bytes there)
                raise ValueError("%d levels for %d cells" % (lv.shape[0], self._cells_L))
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

    def screenshot(self, saveall=True, basename="screenshot", X=None):
        """reference renderer.py:436-475: writes <basename>_<view>.png for flowx, flowy, raw, overlay, texture and mask
        at state X (default: the vertex buffer) and returns the overlay.  Unlike the reference the names carry no
        time stamp: a second call with the same basename overwrites.  saveall=False writes the overlay alone."""
        views = ("flowx", "flowy", "raw", "overlay", "texture", "mask") if saveall else ("overlay",)
        overlay = None
        for v in views:
            img = self.view(X, v)
            write_png("%s_%s.png" % (basename, v), img)
            if v == "overlay":
                overlay = img
        return overlay
