"""NumPy and Python-integer restatement of the full-depth traces (include/hydra_mi.h, "Full-depth traces").

The body map and the positions come from tests/body_ref.py, which restates them for the 8-bit warp; this file restates what
is new: the bilinear sample of unsigned 16-bit texels with a 16-bit result, the byte swap, and the column sums in Python
integers.  NumPy evaluates a * b + c as two rounded operations, as the library (-ffp-contract=off) does.
"""
import numpy as np

import body_ref

COORD_MAX = 1048576.0


def swap_bytes(a):
    """Every 16-bit value with its two bytes exchanged, written out: (v >> 8) | ((v & 255) << 8)"""
    v = np.asarray(a).astype(np.uint32)
    return ((v >> 8) | ((v & 255) << 8)).astype(np.uint16)


def sample16(x, y, frame):
    """The value at position (x, y) (scalars or arrays; NaN and beyond +-2^20: 0) of `frame` (H, W) uint16: bilinear at
    (x - 0.5, y - 0.5), texels clamped to the frame, rint half to even -> uint16"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint16
    H, W = frame.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x >= -COORD_MAX) & (x <= COORD_MAX) & (y >= -COORD_MAX) & (y <= COORD_MAX)
    u = np.where(ok, x, 0.5) - 0.5
    v = np.where(ok, y, 0.5) - 0.5
    fc, fr = np.floor(u), np.floor(v)
    a, b = u - fc, v - fr
    c0, r0 = fc.astype(np.int64), fr.astype(np.int64)
    ca, cb = np.clip(c0, 0, W - 1), np.clip(c0 + 1, 0, W - 1)
    ra, rb = np.clip(r0, 0, H - 1), np.clip(r0 + 1, 0, H - 1)
    f = frame.astype(np.float64)
    val = (1.0 - b) * ((1.0 - a) * f[ra, ca] + a * f[ra, cb]) + b * ((1.0 - a) * f[rb, ca] + a * f[rb, cb])
    return np.where(ok, np.rint(val), 0.0).astype(np.uint16)


def warp16(X, frame, tri_of, l1, l2, ids, swap=0):
    """The registered plane (H, W) uint16 of `frame` (H, W) uint16 as it lies in memory; swap = 1: its bytes are exchanged
    first."""
    frame = np.asarray(frame)
    if swap:
        frame = swap_bytes(frame)
    x, y = body_ref.positions(X, tri_of, l1, l2, ids)
    out = sample16(x, y, frame)
    return np.where(tri_of >= 0, out, 0).astype(np.uint16)


def column_sums(plane, col_ptr, pix, wt):
    """sums[s] = sum over e in column s of wt[e] plane[pix[e]], in Python integers -> a list of C integers"""
    flat = np.asarray(plane).reshape(-1).tolist()
    pix, wt = np.asarray(pix).tolist(), np.asarray(wt).tolist()
    ptr = np.asarray(col_ptr).tolist()
    return [sum(wt[e] * flat[pix[e]] for e in range(ptr[s], ptr[s + 1])) for s in range(len(ptr) - 1)]


def run(Xs, frames, tri_of, l1, l2, ids, col_ptr=None, pix=None, wt=None, swap=0):
    """Every frame at its state -> (sums (F, C) uint64 or None, planes (F, H, W) uint16)"""
    planes = np.stack([warp16(X, f, tri_of, l1, l2, ids, swap) for X, f in zip(Xs, frames)])
    sums = None
    if col_ptr is not None:
        rows = [column_sums(p, col_ptr, pix, wt) for p in planes]
        assert all(v < 2 ** 64 for r in rows for v in r)
        sums = np.array(rows, dtype=np.uint64).reshape(len(rows), len(col_ptr) - 1)
    return sums, planes
