"""CPU checks of tests/border_cases.py: every scene's body map has the property its table states, and the scenes see what
the interior scenes of tests/bodystats_cases.py cannot.  Three rules of the readout are restated here a second time in a
"forgetful" form -- the neighbour products by linear index without the column test, the box <-> plane copy that takes
c0 + pitch <= W for granted, the patch window that wraps across row ends.  On the interior scenes every forgetful form
equals the restatement (so a kernel that forgot the rule passes every test built on them); on the border scenes it
differs (so the tests of tests/test_readout_borders_gpu.py would fail it)."""
import numpy as np
import pytest

import body_ref
import bodystats_cases
import bodystats_ref
import border_cases as cases
import stab_ref

CANARY = 0xA5


def _map(name):
    dm = cases.make_mesh(name)
    W, H = cases.size(name)
    return dm, body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)


def _regs(scene):
    """the registered frames of a scene by the restatement -> (map as a mask, (F, H, W) uint8)"""
    dm, Xs, frames, f0 = scene
    H, W = f0.shape
    tri_of, l1, l2, ids = body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)
    return tri_of >= 0, np.array([body_ref.warp(X, f, tri_of, l1, l2, ids) for X, f in zip(Xs, frames)])


_CACHE = {}


def _scene_regs(kind, name):
    if (kind, name) not in _CACHE:
        _CACHE[kind, name] = _regs((cases if kind == "border" else bodystats_cases).scene(name))
    return _CACHE[kind, name]


# ---- the table ---------------------------------------------------------------------------------------------------------
#: name -> (vertices, triangles, map pixels, c0, r0, bw, bh, pitch, fs); None: not stated
TABLE = {
    "full33x17": (48, 72, 561, 0, 0, 33, 17, 36, 624),
    "disk_over": (46, 70, 804, 0, 0, 37, 23, 40, 928),
    "corner": (None, None, 266, 18, 9, 19, 14, 20, 288),
    "col0": (14, 12, 16, 0, 0, 1, 16, 4, 64),
    "lastcol": (None, None, 16, 15, 0, 1, 16, 4, 64),
    "pixel": (4, 2, 1, 7, 7, 1, 1, 4, 16),
    "empty": (10, 8, 0, 0, 0, 1, 1, 4, 16),
}


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_map_is_what_the_table_says(name):
    dm, (tri_of, l1, l2, ids) = _map(name)
    W, H = cases.size(name)
    m = tri_of >= 0
    nv, nt, npx, c0, r0, bw, bh, pitch, fs = TABLE[name]
    assert nv is None or (dm.size(), dm.t.shape[0]) == (nv, nt)
    assert int(m.sum()) == npx
    assert cases.box_of(m) == dict(c0=c0, r0=r0, bw=bw, bh=bh, pitch=pitch, fs=fs)
    g = stab_ref.patch_grid(m, 4)                               # the restatements' box is the same box
    assert (g["c0"], g["r0"], g["bw"], g["bh"]) == (c0, r0, bw, bh)
    if name == "full33x17":
        assert m.all() and (bw, bh) == (W, H) and pitch > W
    if name == "disk_over":
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and not m.all()
        assert not m[0, 0] and not m[0, -1] and not m[-1, 0] and not m[-1, -1]      # the corners are off the disk
    if name == "corner":
        assert m[-1].any() and m[:, -1].any() and not m[0].any() and not m[:, 0].any()
        assert c0 + bw == W and r0 + bh == H and c0 + pitch > W
    if name == "col0":
        assert m[:, 0].all() and not m[:, 1:].any()
    if name == "lastcol":
        assert m[:, -1].all() and not m[:, :-1].any()
        assert c0 + pitch > W and (r0 + bh - 1) * W + c0 + pitch > H * W           # padding beyond the row, beyond the plane
    if name == "pixel":
        assert m[7, 7] and np.argwhere(m).tolist() == [[7, 7]]
    if name == "empty":
        assert not m.any()


@pytest.mark.parametrize("name", cases.NAMES)
def test_scenes_have_three_states_and_frames_without_a_zero_on_the_border(name):
    dm, Xs, frames, f0 = cases.scene(name)
    W, H = cases.size(name)
    assert len(Xs) == len(frames) == 3 and f0 is frames[0]
    rest = np.asarray(dm.p, np.float64).reshape(-1)
    N = dm.size()
    assert np.array_equal(Xs[0][:2 * N], rest) and Xs[0][2 * N:].any()
    for X, s in zip(Xs[1:], (0.7, 2.5)):
        d = X[:2 * N] - rest
        assert X.shape == (4 * N,) and d.any() and np.abs(d).max() <= 6 * s
    for f in frames:
        assert f.shape == (H, W) and f.dtype == np.uint8
        assert f[0].all() and f[-1].all() and f[:, 0].all() and f[:, -1].all()
    again = cases.scene(name)
    assert all(np.array_equal(a, b) for a, b in zip(Xs + frames, again[1] + again[2]))


def test_the_first_and_last_column_of_full33x17_carry_values_on_adjacent_rows():
    """What the forgetful neighbour products need to show: a value in the last column of a row and one in the first column
    of the next, in the same frame."""
    m, regs = _scene_regs("border", "full33x17")
    assert (regs[:, :-1, -1].astype(np.int64) * regs[:, 1:, 0]).any()
    m, regs = _scene_regs("border", "disk_over")
    assert (regs[:, :-1, -1].astype(np.int64) * regs[:, 1:, 0]).any()


# ---- rule 1: the neighbour products ---------------------------------------------------------------------------------
def _cross_forgetful(regs, inmap):
    """bodystats_ref.accumulate's cross sums with the neighbour of pixel p taken at the linear index p + d_col + W d_row,
    on the plane and in the map, wherever that index is inside the plane: no test of the column"""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    v = np.asarray(regs).astype(np.int64).reshape(len(regs), H * W)
    mf = m.reshape(-1)
    p = np.arange(H * W)
    cross = np.zeros((4, H * W), np.int64)
    for d, (dc, dr) in enumerate(bodystats_ref.FORWARD):
        q = p + dc + W * dr
        ok = (q >= 0) & (q < H * W)
        qc = np.clip(q, 0, H * W - 1)
        both = mf & ok & mf[qc]
        cross[d] = np.where(both, (v * v[:, qc]).sum(0), 0)
    return cross.reshape(4, H, W)


# ---- rule 2: the record's box and the plane ----------------------------------------------------------------------------
def _to_box(reg, inmap, forgetful):
    """One registered frame into the record's box (rows of `pitch` bytes).  The rule: a box row holds the map's values in
    its first bw bytes and zeros in its padding.  Forgetful: `pitch` bytes a row from the linear address (r0 + y) W + c0,
    whatever lies there (behind the plane: CANARY)."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    b = cases.box_of(m)
    c0, r0, bw, bh, pitch = (b[k] for k in ("c0", "r0", "bw", "bh", "pitch"))
    src = np.concatenate((np.where(m, reg, 0).astype(np.uint8).reshape(-1), np.full(pitch, CANARY, np.uint8)))
    n = pitch if forgetful else bw
    box = np.zeros((bh, pitch), np.uint8)
    for y in range(bh):
        at = (r0 + y) * W + c0
        box[y, :n] = src[at:at + n]
    return box


def _to_plane(box, inmap, forgetful):
    """A box frame (padding zero, as the rule leaves it) back into a plane -> the plane and `pitch` bytes of what lies behind
    it.  The rule: bw bytes a row.  Forgetful: `pitch` bytes a row to the linear address (r0 + y) W + c0, the rows last to
    first (a copy by independent threads may take any order)."""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    b = cases.box_of(m)
    c0, r0, bw, bh, pitch = (b[k] for k in ("c0", "r0", "bw", "bh", "pitch"))
    n = pitch if forgetful else bw
    plane = np.concatenate((np.zeros(H * W, np.uint8), np.full(pitch, CANARY, np.uint8)))
    for y in reversed(range(bh)):
        at = (r0 + y) * W + c0
        plane[at:at + n] = box[y, :n]
    return plane


def _box_and_plane(reg, m, forgetful):
    return _to_box(reg, m, forgetful), _to_plane(_to_box(reg, m, False), m, forgetful)


def _same_roundtrip(regs, m):
    return all(all(np.array_equal(a, b) for a, b in zip(_box_and_plane(reg, m, True), _box_and_plane(reg, m, False)))
               for reg in regs)


def test_the_roundtrip_rule_is_the_identity_on_the_map():
    for kind, name in (("border", "full33x17"), ("border", "lastcol"), ("interior", "33x17")):
        m, regs = _scene_regs(kind, name)
        for reg in regs:
            box, plane = _box_and_plane(reg, m, False)
            assert np.array_equal(plane[:m.size].reshape(m.shape), np.where(m, reg, 0)) and (plane[m.size:] == CANARY).all()


# ---- rule 3: the patch window ------------------------------------------------------------------------------------------
def _match_forgetful(regs, inmap, B, S, template):
    """stab_ref.match with v(p + d) and the map at p + d taken at the linear index p + dx + W dy wherever that is inside the
    plane: the window wraps across the ends of rows"""
    m = np.asarray(inmap, bool)
    H, W = m.shape
    n = len(regs)
    g = stab_ref.patch_grid(m, B)
    c0, r0, bw, bh, npx, npy = (g[key] for key in ("c0", "r0", "bw", "bh", "npx", "npy"))
    n1 = 2 * S + 1
    pad = S * W + S
    v = np.zeros((n, H * W + 2 * pad), np.int32)
    v[:, pad:pad + H * W] = np.where(m[None], regs, 0).reshape(n, -1)
    mf = np.zeros(H * W + 2 * pad, bool)
    mf[pad:pad + H * W] = m.reshape(-1)
    cm = m.reshape(-1).copy()
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            cm &= mf[pad + dy * W + dx:pad + dy * W + dx + H * W]
    core = np.zeros((npy * B, npx * B), np.int32)
    core[:bh, :bw] = cm.reshape(H, W)[r0:r0 + bh, c0:c0 + bw]
    t = np.zeros((npy * B, npx * B), np.int32)
    t[:bh, :bw] = np.asarray(template)[r0:r0 + bh, c0:c0 + bw]
    t *= core

    def per_patch(x):
        return x.reshape(n, npy, B, npx, B).sum((2, 4), dtype=np.int64).reshape(n, npy * npx)

    out = dict(n_core=core.reshape(npy, B, npx, B).sum((1, 3)).reshape(-1).astype(np.uint32))
    A, V1, V2 = (np.zeros((n, npy * npx, n1 * n1), np.int64) for _ in range(3))
    x = np.zeros((n, npy * B, npx * B), np.int32)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            s = (dy + S) * n1 + dx + S
            at = pad + dy * W + dx
            x[:, :bh, :bw] = v[:, at:at + H * W].reshape(n, H, W)[:, r0:r0 + bh, c0:c0 + bw]
            xc = x * core
            A[:, :, s], V1[:, :, s], V2[:, :, s] = per_patch(x * t), per_patch(xc), per_patch(xc * x)
    out.update(A=A.astype(np.uint32), V1=V1.astype(np.uint32), V2=V2.astype(np.uint32))
    return out


MATCH_GRIDS = ((7, 1), (16, 3))


def _same_match(regs, m, B, S):
    H, W = m.shape
    t = np.random.default_rng(B).integers(1, 256, (H, W), dtype=np.uint8)
    a, b = _match_forgetful(regs, m, B, S, t), stab_ref.match(regs, m, B, S, t)
    return all(np.array_equal(a[k], b[k]) for k in ("n_core", "A", "V1", "V2"))


# ---- differs here, equal there -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33x17", "96x160"])
def test_on_the_interior_scenes_every_forgetful_rule_equals_the_restatement(name):
    m, regs = _scene_regs("interior", name)
    assert regs[:, m].any() and not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()
    assert np.array_equal(_cross_forgetful(regs, m), bodystats_ref.accumulate(regs, m)[2])
    assert _same_roundtrip(regs, m)
    for B, S in MATCH_GRIDS:
        assert stab_ref.match(regs, m, B, S, regs[0])["n_core"].any()           # (cores exist: the sums are not all zero)
        assert _same_match(regs, m, B, S)


@pytest.mark.parametrize("name", ["full33x17", "disk_over"])
def test_on_the_border_scenes_every_forgetful_rule_differs_from_the_restatement(name):
    m, regs = _scene_regs("border", name)
    assert not np.array_equal(_cross_forgetful(regs, m), bodystats_ref.accumulate(regs, m)[2])
    assert not _same_roundtrip(regs, m)
    for reg in regs:                                            # in every frame, in the box and in the plane
        (fb, fp), (rb, rp) = _box_and_plane(reg, m, True), _box_and_plane(reg, m, False)
        assert not np.array_equal(fb, rb) and not np.array_equal(fp, rp)
    # (the sums run over a patch's core, so a wrapped window shows where it makes a core pixel of a border pixel: with
    # S = 1 on both maps; with S = 3 on the full frame alone -- the polygon of disk_over holds too few rows of the last
    # column for 7 of them to line up with a window on the first)
    for B, S in MATCH_GRIDS if name == "full33x17" else MATCH_GRIDS[:1]:
        assert not _same_match(regs, m, B, S)


@pytest.mark.parametrize("name", ["corner", "lastcol"])
def test_a_box_that_ends_at_the_last_column_shows_the_forgotten_pitch(name):
    m, regs = _scene_regs("border", name)
    assert not _same_roundtrip(regs, m)
