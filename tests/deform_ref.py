"""NumPy restatement of the record against the deformation of its own tissue (include/hydra_mi.h: hm_body_rec_tri_maps,
hm_body_rec_tri_gain), a stand-in for the readout so that hydra_mi.deform runs without a device, and the planted video
under a planted contraction that the recovery tests run on.

`regs` is the registered video (F, H, W) uint8, `tri_of` the body map (H, W), the triangle of every pixel and -1 off the
map.  A pixel off the map counts 0 whatever `regs` holds there, as in the record.  All sums are exact integers.
"""
import numpy as np

import body_ref
import roi_ref
import strain_ref

QMAX = 32767


def _record(regs, tri_of):
    tri_of = np.asarray(tri_of)
    return np.where((tri_of >= 0)[None], np.asarray(regs), 0).astype(np.uint8), tri_of


def tri_maps(regs, tri_of, q):
    """q (F, T) whole numbers, |q| <= 32767 -> (c (H, W) int64 = sum_k v_k(p) q[k, t(p)], w1 (H, W) uint64 = sum_k v_k(p),
    w2 (H, W) uint64 = sum_k v_k(p)^2), 0 off the map"""
    v, tri_of = _record(regs, tri_of)
    q = np.asarray(q).astype(np.int64)
    assert q.shape[0] == v.shape[0] and np.abs(q).max(initial=0) <= QMAX
    m = tri_of >= 0
    t = np.where(m, tri_of, 0)
    v = v.astype(np.int64)
    c = np.where(m, (v * q[:, t]).sum(0), 0)
    return c.astype(np.int64), v.sum(0).astype(np.uint64), (v * v).sum(0).astype(np.uint64)


def tri_gain(regs, tri_of, m):
    """m (F, T) 0..65535 -> ((F, H, W) uint8: min(255, (v_k(p) m[k, t(p)] + 2048) >> 12) on the map, 0 off it; the number
    of values whose unclamped result exceeded 255)"""
    v, tri_of = _record(regs, tri_of)
    m = np.asarray(m).astype(np.int64)
    assert m.shape[0] == v.shape[0] and m.min(initial=0) >= 0 and m.max(initial=0) <= 65535
    on = tri_of >= 0
    t = np.where(on, tri_of, 0)
    r = np.where(on[None], (v.astype(np.int64) * m[:, t] + 2048) >> 12, 0)
    return np.minimum(r, 255).astype(np.uint8), int((r > 255).sum())


def overflow_bound(F):
    """F x F x 255 x 32767 as a Python integer: every sum and the host's F c - w1 u1 are exact in int64 below 2^63"""
    return int(F) * int(F) * 255 * QMAX


class RefBody:
    """What hydra_mi.deform asks of a BodyReadout(keep=True) and of its renderer, answered by the restatements: the record
    is `regs` with 0 off the map.  The deformation comes from the mesh (uv, tri) through strain_ref.strain_tri, or is
    handed over as it is (J (F, T): the states are then not looked at)."""

    def __init__(self, regs, tri_of, uv=None, tri=None, J=None):
        self.keep = True
        self.r = self
        self.regs, tri_of = _record(regs, tri_of)
        self.tri_of_pixel = tri_of.astype(np.int32)
        self.J = None if J is None else np.asarray(J, np.float64)
        if J is None:
            H, W = tri_of.shape
            self.uv = np.asarray(uv, np.float32)
            self.tri = np.asarray(tri, np.int64)
            self.ids = body_ref.body_map(uv, tri, W, H)[3]
        else:
            T = self.J.shape[1]
            self.uv = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32)       # area0 of every triangle: 1 / 2
            self.tri = np.tile(np.array([[0, 1, 2]], np.int64), (T, 1))

    def body_rec_count(self):
        return self.regs.shape[0]

    def body_rec_fetch(self, k0=0, n=None):
        n = self.regs.shape[0] - k0 if n is None else n
        return self.regs[k0:k0 + n].copy()

    def body_rec_label_sums(self, labels, L):
        return roi_ref.label_sums(self.regs, self.tri_of_pixel >= 0, labels, L)

    def body_rec_tri_maps(self, q, want=("c", "w1", "w2")):
        out = tri_maps(self.regs, self.tri_of_pixel, q)
        return tuple(o if k in want else None for k, o in zip(("c", "w1", "w2"), out))

    def body_rec_tri_gain(self, m):
        self.regs, clipped = tri_gain(self.regs, self.tri_of_pixel, m)
        return clipped

    def strain_tri(self, states):
        if self.J is not None:
            out = np.ones(self.J.shape + (7,))
            out[:, :, 0] = self.J
            return out
        return strain_ref.strain_tri(states, self.uv, self.ids)


# ---- the planted video under a planted contraction -------------------------------------------------------------------
GRID = (9, 9, 2.0, 2.0, 15.5, 15.5)     # strain_ref.grid_mesh: 128 triangles of about 16 px that cover roi_ref.planted_map()
J_LO, J_HI = 0.55, 1.05
PERIOD = 75


def planted_triangles(seed=0):
    """-> (p, t, tri_of (H, W) int64): the grid mesh and its body map in the planted video's frame"""
    p, t = strain_ref.grid_mesh(*GRID, seed=seed)
    tri_of = body_ref.body_map(p, t, roi_ref.PLANTED["W"], roi_ref.PLANTED["H"])[0]
    assert (tri_of[roi_ref.planted_map()] >= 0).all()
    return p, t, tri_of


def planted_J(seed, T, F=None):
    """J (F, T): one slow wave for the whole animal, 1 - a_t (1 - cos(2 pi k / 75)) / 2 with a per-triangle amplitude a_t in
    0.25..0.42, plus noise of +-0.015, kept within 0.55..1.05"""
    F = roi_ref.PLANTED["F"] if F is None else F
    rng = np.random.default_rng((seed, 2000))
    amp = rng.uniform(0.25, 0.42, T)
    wave = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(F) / PERIOD))
    J = 1.0 - amp[None, :] * wave[:, None] + rng.uniform(-0.015, 0.015, (F, T))
    return np.clip(J, J_LO, J_HI)


def contracting_video(seed, gamma0, J=None):
    """roi_ref.planted_video(seed) in the body frame with every map pixel's byte made clip(rint(v J^-gamma0), 0, 255), J of
    the pixel's triangle (planted_J, or the one given, for the frames it has) -> dict: video, clean (F, H, W) uint8; centres (12, 2);
    activity (12, F); J (F, T); tri_of (H, W); p, t the mesh; saturated: the share of map values that reached 255."""
    clean, cs, act, _ = roi_ref.planted_video(seed)
    p, t, tri_of = planted_triangles()
    J = planted_J(seed, len(t), clean.shape[0]) if J is None else np.asarray(J, np.float64)
    clean, act = clean[:J.shape[0]], act[:, :J.shape[0]]
    on = tri_of >= 0
    tt = np.where(on, tri_of, 0)
    gain = np.where(on[None], J[:, tt] ** -np.float64(gamma0), 1.0)
    raw = np.rint(clean.astype(np.float64) * gain)
    video = np.clip(raw, 0, 255).astype(np.uint8)
    return {"video": video, "clean": clean, "centres": cs, "activity": act, "J": J, "tri_of": tri_of, "p": p, "t": t,
            "saturated": float((raw[:, on] >= 255).mean())}


def contracting_states(seed, p, F=None):
    """States (F, 4N) of the grid mesh under a contraction towards its centre that comes and goes with the planted wave,
    stronger near the centre, with a little noise per vertex: what a tracker would hand over.  Their J
    (strain_ref.strain_tri) stays within 0.55..1.05."""
    F = roi_ref.PLANTED["F"] if F is None else F
    p = np.asarray(p, np.float64)
    rng = np.random.default_rng((seed, 3000))
    c = p.mean(0)
    d = p - c
    w = np.exp(-(d * d).sum(1) / (2.0 * 60.0 ** 2))
    wave = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(F) / PERIOD))
    out = np.zeros((F, 4 * len(p)))
    for k in range(F):
        x = c + d * (1.0 - 0.17 * wave[k] * w)[:, None] + rng.normal(0.0, 0.03, p.shape)
        out[k, :2 * len(p)] = x.reshape(-1)
    return out


# ---- the figures of the recovery test ----------------------------------------------------------------------------------
def disc_traces(regs, tri_of, centres, radius=3.0):
    """(K, F): the mean of every frame over the map pixels within `radius` of each centre"""
    v, tri_of = _record(regs, tri_of)
    out = []
    for c in centres:
        disc = roi_ref.disc_and_ring(tri_of >= 0, c, radius, 0.0, 0.0)[0]
        out.append(v[:, disc].mean(1))
    return np.array(out)


def _r(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def figures(regs, tri_of, centres, activity, J):
    """-> (mean, min of r(disc trace, planted activity) over the cells; mean |r(disc trace, J of the centre's triangle)|)"""
    tr = disc_traces(regs, tri_of, centres)
    ra = [_r(tr[i], activity[i]) for i in range(len(centres))]
    rj = [abs(_r(tr[i], J[:, tri_of[c[1], c[0]]])) for i, c in enumerate(centres)]
    return float(np.mean(ra)), float(np.min(ra)), float(np.mean(rj))
