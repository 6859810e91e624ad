"""The kept record of ``renderer.Renderer``: the registered video a BodyReadout(keep=True) holds on the device and what is
computed from it there (hm_body_rec_*, the Python side of csrc/record.hip).  ``Record`` is a class of methods that
``Renderer`` inherits beside ``readout.Readout``: it reads the handle ``_h`` and what ``Renderer.__init__`` sets.
"""
import ctypes

import numpy as np

from . import _lib


class Record:
    def _rec_n(self, k0, n):
        """-> the number of frames of a range k0, n of the record (n None: all from k0)"""
        return self.body_rec_count() - int(k0) if n is None else int(n)

    def _rec_out(self, k0, n):
        """-> (n, the (n, H, W) uint8 block that takes the planes of the recorded frames k0 .. k0 + n - 1; n None: all
        from k0)"""
        n = self._rec_n(k0, n)
        return n, np.empty((max(n, 0), self.ny, self.nx), np.uint8)

    def _kind(self, what):
        """-> the number of a plane kind, given by name (PLANES) or number"""
        return self.PLANES[what] if isinstance(what, str) else int(what)

    def _traces(self, q, message, columns=None):
        """-> q as a contiguous (F, L) int32 array, one row per recorded frame (and `columns` columns, if given);
        message % (dtype, shape, F[, columns]) refuses anything else"""
        F = self.body_rec_count()
        q = np.asarray(q)
        if (q.dtype != np.int32 or q.ndim != 2 or (columns is not None and q.shape[1] != columns)
                or (F and q.shape[0] != F)):                                       # (F 0: the call says why)
            raise ValueError(message % ((q.dtype, q.shape, F) + (() if columns is None else (columns,))))
        return np.ascontiguousarray(q)

    @staticmethod
    def _wanted(want, **arrays):
        """-> {key: an empty array of its (shape, dtype)} for the keys that are in `want`"""
        return {key: np.empty(*a) for key, a in arrays.items() if key in want}

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
        n, out = self._rec_out(k0, n)
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
        S = 2 * int(R) + 1
        q = self._traces(q, "traces %s of shape %r for %d frames and %d seeds (need int32)", sd.shape[0])
        out = np.empty((sd.shape[0], S, S), np.int64)
        _lib.check(_lib.lib().hm_body_rec_trace_products(self._h, sd.shape[0], _lib.ptr(sd), int(R), _lib.ptr(q), _lib.ptr(out)),
                   "hm_body_rec_trace_products")
        return out

    def body_rec_trace_maps(self, q, want=("c", "w1", "w2")):
        """hm_body_rec_trace_maps: L int32 traces, q (F, L) with |q| <= 32767 -> dict of those in `want`: c (L, H, W) int64,
        the sum over the recorded frames of every pixel times every trace; w1, w2 (H, W) uint64, the sums of every pixel
        and of its square (0 outside the map)."""
        q = self._traces(q, "traces %s of shape %r for %d frames (need int32, frames x traces)")
        L, H, W = q.shape[1], self.ny, self.nx
        o = self._wanted(want, c=((min(max(L, 0), 1024), H, W), np.int64),          # (L out of range: the call says so)
                         w1=((H, W), np.uint64), w2=((H, W), np.uint64))
        _lib.check(_lib.lib().hm_body_rec_trace_maps(self._h, L, _lib.ptr(q), *[_lib.ptr(o.get(k)) for k in ("c", "w1", "w2")]),
                   "hm_body_rec_trace_maps")
        return o

    def body_rec_trace_null(self, q, vb, want=("tmax", "tmin", "ge", "le")):
        """hm_body_rec_trace_null: q (F, L) int32 with |q| <= 32767, column 0 the observed trace and the others its
        surrogates, vb (L,) float64 = F u2 - u1^2 of every column -> dict of those in `want`: tmax, tmin (L,) float64, the
        largest and smallest correlation of every column over the map; ge, le (H, W) uint32, per pixel the surrogates
        whose numerator is >= and <= the observed one (0 outside the map)."""
        q = self._traces(q, "traces %s of shape %r for %d frames (need int32, frames x traces)")
        L, H, W = q.shape[1], self.ny, self.nx
        vb = np.ascontiguousarray(vb, np.float64)
        if vb.shape != (L,):
            raise ValueError("vb of shape %r for %d traces" % (vb.shape, L))
        o = self._wanted(want, tmax=(max(L, 0), np.float64), tmin=(max(L, 0), np.float64), ge=((H, W), np.uint32),
                         le=((H, W), np.uint32))
        _lib.check(_lib.lib().hm_body_rec_trace_null(self._h, L, _lib.ptr(q), _lib.ptr(vb),
                                                     *[_lib.ptr(o.get(k)) for k in ("tmax", "tmin", "ge", "le")]),
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
        o = self._wanted(want, G=((m, m), np.int64), s1=(m, np.uint64))
        _lib.check(_lib.lib().hm_body_rec_gram(self._h, k0, n, stride, *[_lib.ptr(o.get(k)) for k in ("G", "s1")]),
                   "hm_body_rec_gram")
        return o

    # -- residual motion of the record (hm_body_rec_match / _frame_sums / _shift / _warp / _field_sums; hydra_mi.stabilize) --
    def body_rec_patches(self, B):
        """-> (patches per row, patch rows) of the grid of B x B patches over the record's box (the bounding box of the
        body map)"""
        box = self._body_rec_box
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
        c, w1, w2 = (self._wanted(want, c=((H, W), np.int64), w1=((H, W), np.uint64), w2=((H, W), np.uint64)).get(k)
                     for k in ("c", "w1", "w2"))
        _lib.check(_lib.lib().hm_body_rec_tri_maps(self._h, q.shape[1], _lib.ptr(q), _lib.ptr(c), _lib.ptr(w1), _lib.ptr(w2)),
                   "hm_body_rec_tri_maps")
        return c, w1, w2

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
        what = self._kind(what)
        n, out = self._rec_out(k0, n)
        _lib.check(_lib.lib().hm_body_rec_planes(self._h, int(k0), n, what, int(half), int(q), int(floor), int(gain),
                                                 _lib.ptr(out)), "hm_body_rec_planes")
        return out

    def body_rec_stats_add(self, what, half, q, floor=1, gain=1):
        """hm_body_rec_stats_add: add every recorded frame's plane of kind `what` (as body_rec_planes) to the statistics
        begun with body_stats_begin, as if each had just been warped."""
        what = self._kind(what)
        _lib.check(_lib.lib().hm_body_rec_stats_add(self._h, what, int(half), int(q), int(floor), int(gain)),
                   "hm_body_rec_stats_add")

    # -- events per pixel of the record: AR(1) deconvolution of the planes (hm_body_rec_event_*; hydra_mi.events) -----
    def body_rec_event_planes(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0, k0=0, n=None):
        """hm_body_rec_event_planes: -> (n, H, W) uint8, the event bytes min(255, floor(s + 0.5)) of the recorded frames
        k0 .. k0 + n - 1 (default: all from k0): s the AR(1) deconvolution (decay g per frame, penalty lam) of every
        pixel's planes of kind `what` (as body_rec_planes) over the whole record."""
        what = self._kind(what)
        n, out = self._rec_out(k0, n)
        _lib.check(_lib.lib().hm_body_rec_event_planes(self._h, int(k0), n, what, int(half), int(q), int(floor), int(gain),
                                                       float(g), float(lam), _lib.ptr(out)), "hm_body_rec_event_planes")
        return out

    def body_rec_event_stats_add(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0):
        """hm_body_rec_event_stats_add: add every recorded frame's event plane (as body_rec_event_planes) to the statistics
        begun with body_stats_begin, as if each had just been warped."""
        what = self._kind(what)
        _lib.check(_lib.lib().hm_body_rec_event_stats_add(self._h, what, int(half), int(q), int(floor), int(gain), float(g),
                                                          float(lam)), "hm_body_rec_event_stats_add")

    def body_rec_event_sums(self, what, half, q, floor=1, gain=1, g=0.9, lam=0.0, s_min=1.0):
        """hm_body_rec_event_sums: -> (count (H, W) uint32, sum (H, W) float64): per pixel the number of frames with
        s >= s_min and the sum of s over the record (s as in body_rec_event_planes, before rounding)."""
        what = self._kind(what)
        count, total = np.empty((self.ny, self.nx), np.uint32), np.empty((self.ny, self.nx), np.float64)
        _lib.check(_lib.lib().hm_body_rec_event_sums(self._h, what, int(half), int(q), int(floor), int(gain), float(g), float(lam),
                                                     float(s_min), _lib.ptr(count), _lib.ptr(total)), "hm_body_rec_event_sums")
        return count, total

    # -- activity waves: latency per event and pixel, its sums, the local fits' sums (hm_body_rec_waves; hydra_mi.waves) -----
    WAVE_OUTPUTS = ("n_bin", "lat", "rise", "why", "cnt", "sum_lat", "sum_lat2", "fit")

    def body_rec_wave_nodes(self, step):
        """hm_body_rec_wave_nodes: -> (nx, ny, c0, r0): the grid of fit nodes of body_rec_waves, node (i, j) at column
        c0 + i step, row r0 + j step of the frame, row-major."""
        v = [ctypes.c_int(0) for _ in range(4)]
        _lib.check(_lib.lib().hm_body_rec_wave_nodes(self._h, int(step), *[ctypes.byref(x) for x in v]), "hm_body_rec_wave_nodes")
        return tuple(int(x.value) for x in v)

    def body_rec_waves(self, triggers, what, half, q, floor=1, gain=1, b=2, pre=8, lead=8, post=24, min_rise=8, step=8, Rf=6,
                       want=WAVE_OUTPUTS):
        """hm_body_rec_waves: per trigger frame (int32, E of them) and pixel the latency at which the binned plane of kind
        `what` (as body_rec_planes) crosses half of its rise, in 1/256 frame relative to the trigger -> a dict of the
        outputs named in `want`: n_bin (H, W) uint16; lat, rise (E, H, W) int32 and why (E, H, W) uint8 (lat is INT32_MIN
        where why >= 2); cnt (H, W) uint32, sum_lat, sum_lat2 (H, W) int64 over the events with why <= 1; fit
        (E, nodes, 9) int64: n, sum dx, dy, dx^2, dx dy, dy^2, Lat, dx Lat, dy Lat over the valid pixels within Rf of a node."""
        what = self._kind(what)
        t = np.ascontiguousarray(triggers, np.int32).reshape(-1)
        E, H, W = int(t.size), self.ny, self.nx
        shapes = dict(n_bin=((H, W), np.uint16), lat=((E, H, W), np.int32), rise=((E, H, W), np.int32), why=((E, H, W), np.uint8),
                      cnt=((H, W), np.uint32), sum_lat=((H, W), np.int64), sum_lat2=((H, W), np.int64))
        if "fit" in want and E:
            nx, ny = self.body_rec_wave_nodes(step)[:2]
            shapes["fit"] = ((E, nx * ny, 9), np.int64)
        out = self._wanted(want, **shapes)
        _lib.check(_lib.lib().hm_body_rec_waves(self._h, E, _lib.ptr(t), what, int(half), int(q), int(floor), int(gain), int(b),
                                                int(pre), int(lead), int(post), int(min_rise), int(step), int(Rf),
                                                *[_lib.ptr(out.get(k)) for k in self.WAVE_OUTPUTS]), "hm_body_rec_waves")
        return out

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
        n, out = self._rec_out(k0, n)
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
