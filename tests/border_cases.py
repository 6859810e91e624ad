"""Scenes whose body map touches the frame's border, for the tests of the body-frame readout: the shape of
tests/bodystats_cases.py (scene(name) -> (mesh, states, frames, frame 0); the filter is bodystats_cases.make_filter), with
the mesh reaching over the frame so that the record's box starts at column 0 or row 0, ends at the last column or the last
row, is 1 pixel wide, is a single pixel, or does not exist.

  name        frame W x H  mesh                                     the map (tests/test_border_cases_cpu.py asserts it)
  full33x17   33 x 17      box_mesh(-1.0, -1.5, 34.0, 18.5, 5.0)    all 561 pixels: the box is the frame, pitch 36 > W
  disk_over   37 x 23      disk_mesh(18.0, 11.0, 19.0, 6.0)         804 of 851 pixels, on all four borders, no rectangle
  corner      37 x 23      box_mesh(18.0, 9.0, 40.0, 30.0, 5.0)     reaches the last column and the last row only
  col0        16 x 16      box_mesh(-0.4, -1.0, 0.9, 17.0, 3.0)     column 0, rows 0..15: bw 1, pitch 4
  lastcol     16 x 16      box_mesh(15.2, -1.0, 17.0, 17.0, 3.0)    column 15, rows 0..15: the padding of every row lies
                                                                    beyond the row, on row 15 beyond the plane
  pixel       16 x 16      square4_mesh(7.2, 8.1)                   the pixel (row 7, column 7) alone: a record frame of 16 bytes
  empty       16 x 16      box_mesh(5.6, 2.0, 6.4, 14.0, 3.0)       no pixel centre is covered

Three states per scene: rest + N(0, s) for s = 0, 0.7, 2.5 px, velocities random, all seeded by the name.  Frames are
random uint8 with no zero on the frame's first and last row and column, so a clamped texel is never a stand-in for "off the
frame".  The handle accepts every one of these meshes as it is (tests/test_readout_borders_gpu.py builds a filter on each);
no mesh had to be swapped.
"""
import zlib

import numpy as np

NAMES = ["full33x17", "disk_over", "corner", "col0", "lastcol", "pixel", "empty"]
N_FRAMES = 3
#: name -> (W, H, mesh builder, its arguments)
CASES = {
    "full33x17": (33, 17, "box_mesh", (-1.0, -1.5, 34.0, 18.5, 5.0)),
    "disk_over": (37, 23, "disk_mesh", (18.0, 11.0, 19.0, 6.0)),
    "corner": (37, 23, "box_mesh", (18.0, 9.0, 40.0, 30.0, 5.0)),
    "col0": (16, 16, "box_mesh", (-0.4, -1.0, 0.9, 17.0, 3.0)),
    "lastcol": (16, 16, "box_mesh", (15.2, -1.0, 17.0, 17.0, 3.0)),
    "pixel": (16, 16, "square4_mesh", (7.2, 8.1)),
    "empty": (16, 16, "box_mesh", (5.6, 2.0, 6.4, 14.0, 3.0)),
}


def seed_of(name):
    return zlib.crc32(name.encode())


def size(name):
    """-> (W, H)"""
    return CASES[name][:2]


def make_mesh(name):
    from hydra_mi import mesh
    _, _, builder, args = CASES[name]
    return getattr(mesh, builder)(*args)


def random_frames(rng, n, H, W):
    """n random frames (n, H, W) uint8 whose first and last row and column hold no zero"""
    f = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    for edge in (f[:, 0, :], f[:, -1, :], f[:, :, 0], f[:, :, -1]):
        np.maximum(edge, 1, out=edge)
    return f


def scene(name):
    """-> (mesh, states, frames, frame 0)"""
    W, H = size(name)
    dm = make_mesh(name)
    rng = np.random.default_rng(seed_of(name))
    frames = list(random_frames(rng, N_FRAMES, H, W))
    N = dm.size()
    Xs = []
    for s in (0.0, 0.7, 2.5):
        X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, s, 2 * N), rng.normal(0, 1, 2 * N)))
        Xs.append(X)
    return dm, Xs, frames, frames[0]


def record_pairs(name, F=7):
    """-> F (state, frame) pairs to record: the scene's states in turn, a fresh random frame each"""
    W, H = size(name)
    Xs = scene(name)[1]
    frames = random_frames(np.random.default_rng(seed_of(name) + 1), F, H, W)
    return [(Xs[k % len(Xs)], frames[k]) for k in range(F)]


def box_of(inmap):
    """The record's box of a map (a mask): c0, r0, bw, bh, pitch (rows padded to 4 bytes) and fs (a frame padded to 16
    bytes); the box of an empty map is one pixel at (0, 0) (include/hydra_mi.h: hm_body_rec_begin)"""
    m = np.asarray(inmap, bool)
    if not m.any():
        c0 = r0 = 0
        bw = bh = 1
    else:
        cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
        c0, r0 = int(cols[0]), int(rows[0])
        bw, bh = int(cols[-1]) - c0 + 1, int(rows[-1]) - r0 + 1
    pitch = (bw + 3) & ~3
    return dict(c0=c0, r0=r0, bw=bw, bh=bh, pitch=pitch, fs=(pitch * bh + 15) & ~15)
