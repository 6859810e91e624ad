"""The full-depth traces on the device (`pytest -m gpu`), bit for bit against tests/deeptrace_ref.py: the planes of
k_body_warp16 on every scene of tests/border_cases.py (runs of 1, max_run and max_run + 1 frames, both byte orders, states
with a vertex that is not finite or beyond 2^20, guard bytes) and against the 8-bit warp; the sums of k_deep_cols (C = 1 and
4096, columns of 1, 63, 64, 65 and 257 entries, a pixel in three columns, entries off the map, a state per frame); the
64-bit widths and the split of a long column; the second pass against the kept record end to end; what the depth buys; the
refusals; the CLI."""
import ctypes
import os
import sys

import numpy as np
import pytest

import body_ref
import bodystats_cases
import border_cases as bc
import deeptrace_ref as ref
import demix_ref
import roi_ref

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
MAX_RUN = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Rig:
    def __init__(self, name):
        self.dm, self.Xs, _, f0 = bc.scene(name)
        self.W, self.H = bc.size(name)
        self.kf = bodystats_cases.make_filter(self.dm, f0)
        self.r = self.kf.state.renderer
        self.map = body_ref.body_map(np.asarray(self.dm.p, np.float32), self.dm.t, self.W, self.H)

    def states(self, F, spoil=True):
        """F states, a different one for every frame: the scene's three in turn, each moved a little further; with spoil
        frame 1 has a vertex that is not finite and frame 2 one beyond 2^20"""
        N = self.dm.size()
        out = []
        for k in range(F):
            X = self.Xs[k % 3].copy()
            X[:2 * N] += 0.37 * (k // 3)
            out.append(X)
        if spoil and F > 1:
            out[1][0] = np.nan
        if spoil and F > 2:
            out[2][2 * N - 1] = -2.0e6
        return np.array(out)


@pytest.fixture(scope="module")
def rigs(hm):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(name)
        return made[name]

    yield get
    for rig in made.values():
        rig.kf.close()


def _handle(W, H, run=MAX_RUN):
    from hydra_mi import deepio
    return deepio._Handle(W, H, run, 0)


def _set_columns(h, r, col_ptr, pix, wt):
    from hydra_mi import _lib
    col_ptr = np.ascontiguousarray(col_ptr, np.int64)
    pix = np.ascontiguousarray(pix, np.int32)
    wt = np.ascontiguousarray(wt, np.uint16)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    return _lib.lib().hm_deep_body_set_columns(h._h, r._h, len(col_ptr) - 1, _lib.ptr(col_ptr), _lib.ptr(pad(pix)), _lib.ptr(pad(wt)))


def _run(h, r, block, swap, X, C=0, planes=False):
    """hm_deep_body_run with guard bytes round both outputs -> (rc, sums or None, planes or None)"""
    from hydra_mi import _lib
    block = np.ascontiguousarray(block)
    X = np.ascontiguousarray(X, np.float64)
    F, n = block.shape[0], block.shape[1] * block.shape[2]
    sbuf = np.full(GUARD + 8 * F * C + GUARD, FILL, np.uint8)
    pbuf = np.full(GUARD + 2 * F * n + GUARD, FILL, np.uint8)
    sp = ctypes.c_void_p(sbuf.ctypes.data + GUARD) if C else None
    pp = ctypes.c_void_p(pbuf.ctypes.data + GUARD) if planes else None
    rc = _lib.lib().hm_deep_body_run(h._h, r._h, F, _lib.ptr(block.view(np.uint16)), int(swap), _lib.ptr(X), sp, pp)
    for buf in (sbuf, pbuf):
        assert (buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all()
    if not C:
        assert (sbuf == FILL).all()
    if not planes:
        assert (pbuf == FILL).all()
    sums = sbuf[GUARD:-GUARD].view(np.uint64).reshape(F, C).copy() if C else None
    pl = pbuf[GUARD:-GUARD].view(np.uint16).reshape(block.shape).copy() if planes else None
    return rc, sums, pl


def _err():
    from hydra_mi import _lib
    return _lib.lib().hm_last_error().decode()


# ---- planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.NAMES)
def test_planes_equal_the_restatement(rigs, name):
    g = rigs(name)
    rng = np.random.default_rng(bc.seed_of(name) + 11)
    h = _handle(g.W, g.H)
    try:
        for F in (1, MAX_RUN, MAX_RUN + 1):
            video = rng.integers(0, 65536, (F, g.H, g.W)).astype(np.uint16)
            X = g.states(F)
            want = ref.run(X, video, *g.map)[1]
            if F > 1 and (g.map[0] >= 0).any():                     # the spoilt vertices give 0 where they reach, and nothing else
                clean = ref.run(g.states(F, spoil=False), video, *g.map)[1]
                uses0 = (g.map[3][np.where(g.map[0] >= 0, g.map[0], 0)] == 0).any(-1) & (g.map[0] >= 0)
                assert (want[1][uses0] == 0).all() and np.array_equal(want[1][~uses0], clean[1][~uses0])
            for swap in (0, 1):
                rc, _, got = _run(h, g.r, video.byteswap() if swap else video, swap, X, planes=True)
                assert rc == 0, _err()
                assert np.array_equal(got, want), (F, swap)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["full33x17", "disk_over"])
def test_planes_of_8_bit_values_equal_the_old_kernel(rigs, name):
    g = rigs(name)
    F = MAX_RUN + 2
    f8 = bc.random_frames(np.random.default_rng(5), F, g.H, g.W)
    X = g.states(F)
    h = _handle(g.W, g.H)
    try:
        rc, _, got = _run(h, g.r, f8.astype(np.uint16), 0, X, planes=True)
        assert rc == 0, _err()
    finally:
        h.close()
    old = np.array([g.r.body_warp(X[k], f8[k])[0] for k in range(F)])
    assert got.max() <= 255 and np.array_equal(got.astype(np.uint8), old)


# ---- sums --------------------------------------------------------------------------------------------------------------
def _test_columns(g, rng, C):
    """columns of 1, 63, 64, 65 and 257 entries among C (the rest empty), drawn from all pixels -- on and off the map, with
    repeats --, pixel `three` in three of them"""
    n = g.W * g.H
    on = np.flatnonzero(g.map[0].reshape(-1) >= 0)
    three = int(on[len(on) // 2]) if len(on) else n // 2
    lengths = np.zeros(C, np.int64)
    where = [0] if C == 1 else [0, 7, 2000, 2001, C - 1]
    for s, ln in zip(where, [257] if C == 1 else [1, 63, 64, 65, 257]):
        lengths[s] = ln
    ptr = np.concatenate(([0], np.cumsum(lengths)))
    pix = rng.integers(0, n, int(ptr[-1])).astype(np.int32)
    for s in where[-3:]:
        pix[ptr[s]] = three
    wt = rng.integers(0, 65536, pix.shape[0]).astype(np.uint16)
    wt[::17] = 65535
    return ptr, pix, wt


@pytest.mark.parametrize("name,C", [("disk_over", 4096), ("disk_over", 1), ("full33x17", 4096), ("pixel", 4096), ("empty", 1)])
def test_sums_equal_the_restatement(rigs, name, C):
    g = rigs(name)
    rng = np.random.default_rng(bc.seed_of(name) + C)
    F = MAX_RUN + 1
    video = rng.integers(0, 65536, (F, g.H, g.W)).astype(np.uint16)
    video[0] = 65535
    X = g.states(F, spoil=False)                                     # a different state for every frame of a run
    ptr, pix, wt = _test_columns(g, rng, C)
    if name == "disk_over":
        assert (g.map[0].reshape(-1)[pix] < 0).any()                 # entries off the map
    want_s, want_p = ref.run(X, video, *g.map, ptr, pix, wt)
    assert len({want_p[k].tobytes() for k in range(F)}) == F or not (g.map[0] >= 0).any()
    h = _handle(g.W, g.H)
    try:
        assert _set_columns(h, g.r, ptr, pix, wt) == 0, _err()
        rc, got, _ = _run(h, g.r, video, 0, X, C=C)
        assert rc == 0, _err()
        assert np.array_equal(got, want_s)
        rc, got, pl = _run(h, g.r, video.byteswap(), 1, X, C=C, planes=True)      # both outputs at once, swapped bytes
        assert rc == 0, _err()
        assert np.array_equal(got, want_s) and np.array_equal(pl, want_p)
    finally:
        h.close()


# ---- the widths --------------------------------------------------------------------------------------------------------
def test_products_and_reduction_are_64_bit(rigs):
    g = rigs("full33x17")
    N = g.dm.size()
    rest = np.concatenate((np.asarray(g.dm.p, np.float64).reshape(-1), np.zeros(2 * N)))[None]
    video = np.full((1, g.H, g.W), 65535, np.uint16)
    h = _handle(g.W, g.H)
    try:
        assert _set_columns(h, g.r, [0, 2], [40, 300], [65535, 65535]) == 0, _err()
        rc, got, _ = _run(h, g.r, video, 0, rest, C=1)
        assert rc == 0, _err()
        assert got.tolist() == [[2 * 4294836225]]
        assert got.tolist() == ref.run(rest, video, *g.map, [0, 2], [40, 300], [65535, 65535])[0].tolist()
    finally:
        h.close()


def test_a_long_column_passes_2_32_and_splits_to_the_same_bytes(hm):
    from hydra_mi import mesh
    W = H = 300
    dm = mesh.box_mesh(-1.0, -1.0, 301.0, 301.0, 40.0)
    N = dm.size()
    rng = np.random.default_rng(12)
    kf = bodystats_cases.make_filter(dm, np.zeros((H, W), np.uint8))
    r = kf.state.renderer
    h = _handle(W, H)
    try:
        assert (r.body_map()[0] >= 0).all()                          # a whole-frame map
        rest = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * N)))
        moved = rest.copy()
        moved[:2 * N] += rng.normal(0, 1.5, 2 * N)
        X = np.array([rest, moved])
        video = np.stack([np.full((H, W), 65535, np.uint16), rng.integers(0, 65536, (H, W)).astype(np.uint16)])
        n = W * H
        ptr, pix, wt = [0, n, n + 70], np.concatenate((np.arange(n), np.arange(70))), np.ones(n + 70, np.uint16)
        m = body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)
        want = ref.run(X, video, *m, ptr, pix, wt)[0]
        assert int(want[0, 0]) == 90000 * 65535 > 2 ** 32
        assert _set_columns(h, r, ptr, pix, wt) == 0, _err()
        seen = []
        for value in (64, 1000, 1024):                               # the smallest, a mid value that does not divide, the default
            r.tune("deep_col_entries", value)
            rc, got, _ = _run(h, r, video, 0, X, C=2)
            assert rc == 0, _err()
            seen.append(got.tobytes())
            assert np.array_equal(got, want), value
        assert seen[0] == seen[1] == seen[2]
        from hydra_mi import _lib
        for bad in (63, 2 ** 30 + 1):
            assert _lib.lib().hm_ctx_tune(r._h, b"deep_col_entries", bad) == -1 and "deep_col_entries" in _err()
    finally:
        h.close()
        kf.close()


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_second_pass_equals_the_kept_record_after_tracking(hm):
    """A 16-bit video with values <= 255 tracked through DeepSource with the window 0..255 (make_lut is the identity
    there): the ROI and ring columns read from the 16-bit frames equal hm_body_rec_label_sums and
    hm_body_rec_weighted_sums of the kept record, and deep_dff equals dff."""
    from hydra_mi import body, deepio, deeptrace, kalman, mesh, roi, synth
    from hydra_mi.pipeline import FlowEKFPipeline
    n, F = 96, 8
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    deep = video.astype(np.uint16)
    lut = deepio.make_lut(0, 255)
    assert np.array_equal(lut[:256], np.arange(256))
    kf = kalman.IteratedMSKalmanFilter(mesh.disk_mesh(c[0], c[1], rad - 1.0, 12.0), video[0], np.zeros((n, n, 2), np.float32),
                                       True, nI=3)
    src = deepio.DeepSource(deep, lut, 0, 255, 0, frames=video)
    pipe = FlowEKFPipeline(kf, src, flow_batch=2)
    b = body.BodyReadout(kf, keep=True)
    states = []
    try:
        pipe.run(on_frame=lambda k, e: states.append(kf.state.X.reshape(-1).copy()), body=b)
    finally:
        pipe.close()
        src.close()
    try:
        r = kf.state.renderer
        assert len(states) == F - 1 == r.body_rec_count()
        pts = np.array([[c[0], c[1]], [c[0] + 11.0, c[1] + 2.0], [c[0] - 4.0, c[1] - 13.0]]) + 0.5
        e = roi.extract(b, pts, r_disc=3.0)
        seeds, P = e["seeds"], 3
        w, ring_counts, Rg = roi.ring_weights(e["roi_labels"], b.tri_of_pixel >= 0, seeds, 6.0, 8.5)
        cols = deeptrace.columns(e["roi_labels"], P, [(seeds, w, Rg)])
        sums = deeptrace.run(b, deep, states, cols)
        assert np.array_equal(sums[:, :P], r.body_rec_label_sums(e["roi_labels"], P))
        assert np.array_equal(sums[:, P:], r.body_rec_weighted_sums(seeds, w, Rg))
        assert sums[:, :P].min() > 0
        got = deeptrace.extract(b, deep, states, e)
        assert np.array_equal(_bits(got["deep_dff"]), _bits(e["dff"]))
        assert np.array_equal(_bits(got["deep_F_roi"]), _bits(e["F_roi"])) and np.array_equal(_bits(got["deep_F_np"]), _bits(e["F_np"]))
        # the host path gives the same bytes
        assert np.array_equal(deeptrace.run(b, deep, states, cols, device=None), sums)
    finally:
        kf.close()


def test_demixed_traces_of_8_bit_values_equal_the_last_round(hm):
    """values that fit 8 bits: deep_demix_c is demix.extract's C, the traces step on the same whole numbers"""
    from hydra_mi import body, deeptrace, demix, mesh
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, _ = demix_ref.paired_scene(4, 4, dm.p)
    kf = bodystats_cases.make_filter(dm, frames[0])
    try:
        b = body.BodyReadout(kf, keep=True)
        for X, f in zip(states, frames):
            b.registered(X, f)
        e = demix.extract(b, cs + 0.5, iters=2, alpha=1.0)
        got = deeptrace.extract(b, np.asarray(frames).astype(np.uint16), states, e, demixed=e, alpha=1.0, first=0)
        assert np.array_equal(_bits(got["deep_demix_c"]), _bits(e["C"]))
        assert np.array_equal(_bits(got["deep_dff"]), _bits(e["dff"]))
    finally:
        kf.close()


def test_depth_is_kept_where_8_bits_clip(hm):
    """One flat cell on a 12-bit scene whose brightness rises through the window's hi: the 8-bit F_roi is flat from there
    on, deep_F_roi keeps rising.  8 frames."""
    from hydra_mi import body, deepio, deeptrace, mesh, roi
    H = W = 48
    F, lo, hi = 8, 0, 2040
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W]
    cell = (xx - 24) ** 2 + (yy - 22) ** 2 <= 9
    # (a background that does not change: its pixels have no variance, so none of them joins the ROI by chance)
    video = np.repeat((400 + rng.integers(0, 200, (1, H, W))).astype(np.uint16), F, axis=0)
    level = [900, 1300, 1700, 2100, 2500, 2900, 3300, 3700]           # above hi from frame 3 on
    for k in range(F):
        video[k][cell] = level[k]
    mapped = deepio.map_video(video, deepio.make_lut(lo, hi), lo, hi, device=0)[0]
    dm = mesh.box_mesh(4.0, 4.0, 44.0, 44.0, 10.0)
    N = dm.size()
    # the state the map was taken at: the vertices snapped to 1/256 px, so that every body pixel lands on its own centre and
    # the cell's border pixels take nothing from the background
    snapped = np.rint(np.asarray(dm.p, np.float32).astype(np.float64) * 256.0) / 256.0
    rest = np.concatenate((snapped.reshape(-1), np.zeros(2 * N)))
    kf = bodystats_cases.make_filter(dm, mapped[0])
    try:
        b = body.BodyReadout(kf, keep=True)
        for f in mapped:
            b.registered(rest, f)
        e = roi.extract(b, np.array([[24.5, 22.5]]), thr=0.9)
        assert np.array_equal(e["roi_labels"] == 0, cell)
        got = deeptrace.extract(b, video, [rest] * F, e, first=0)
        assert (e["F_roi"][3:, 0] == 255.0).all()                    # clipped flat
        assert got["deep_F_roi"][:, 0].tolist() == [float(v) for v in level]
        assert (np.diff(got["deep_F_roi"][:, 0]) > 0).all()
        assert got["deep_dff"][7, 0] > got["deep_dff"][3, 0] and e["dff"][7, 0] == e["dff"][3, 0]
        off = deeptrace.extract(b, video, [rest] * F, e, offset=400.0, first=0)
        assert off["deep_F_roi"][:, 0].tolist() == [float(v - 400) for v in level]
    finally:
        kf.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_numbers_and_leave_the_handles_working(rigs):
    from hydra_mi import _lib
    L = _lib.lib()
    g = rigs("full33x17")
    n = g.W * g.H
    video = np.random.default_rng(3).integers(0, 65536, (2, g.H, g.W)).astype(np.uint16)
    X = g.states(2, spoil=False)
    h = _handle(g.W, g.H)
    other = _handle(16, 16)
    try:
        rc, _, _ = _run(h, g.r, video, 0, X, C=1)                    # sums before any columns
        assert rc == _lib.HM_ERR_STATE and "no columns" in _err()
        rc, _, pl = _run(h, g.r, video, 0, X, planes=True)           # planes alone work without columns
        want = ref.run(X, video, *g.map)[1]
        assert rc == 0 and np.array_equal(pl, want)
        one, w1 = np.zeros(1, np.int32), np.ones(1, np.uint16)
        for C, words in ((0, "0 columns outside 1..4096"), (4097, "4097 columns outside 1..4096")):
            ptr = np.zeros(C + 1, np.int64)
            assert L.hm_deep_body_set_columns(h._h, g.r._h, C, _lib.ptr(ptr), _lib.ptr(one), _lib.ptr(w1)) == -1
            assert words in _err()
        assert _set_columns(h, g.r, [0, 3, 2, 4], [1, 2, 3, 4], [1, 1, 1, 1]) == -1
        assert "column 1" in _err() and "2 after 3" in _err()
        assert _set_columns(h, g.r, [1, 2], [1, 2], [1, 1]) == -1 and "col_ptr[0] = 1" in _err()
        assert _set_columns(h, g.r, [0, 1, 3], [5, 6, n], [1, 1, 1]) == -1
        assert "entry 2" in _err() and "pixel %d" % n in _err()
        assert _set_columns(h, g.r, [0, 1], [-1], [1]) == -1 and "entry 0" in _err() and "pixel -1" in _err()
        # handles of two sizes: both are named
        assert _set_columns(other, g.r, [0, 1], [5], [1]) == -1
        assert "16x16" in _err() and "33x17" in _err()
        rc, _, _ = _run(other, g.r, np.zeros((1, 16, 16), np.uint16), 0, X[:1], planes=True)
        assert rc == -1 and "16x16" in _err() and "33x17" in _err()
        # the run's own arguments
        assert L.hm_deep_body_run(h._h, g.r._h, 0, _lib.ptr(video), 0, _lib.ptr(X), None, _lib.ptr(np.zeros_like(video))) == -1
        assert "0 frames" in _err()
        assert L.hm_deep_body_run(h._h, g.r._h, 2, _lib.ptr(video), 0, _lib.ptr(X), None, None) == -1
        assert "neither sums nor planes" in _err()
        # after all that: columns set, used, cleared
        ptr, pix, wt = [0, 2, 2, 5], [3, 3, 0, 1, 3], [65535, 65535, 1, 10, 2]
        assert _set_columns(h, g.r, ptr, pix, wt) == 0, _err()
        rc, got, pl = _run(h, g.r, video, 0, X, C=3, planes=True)
        assert rc == 0 and np.array_equal(pl, want) and np.array_equal(got, ref.run(X, video, *g.map, ptr, pix, wt)[0])
        assert L.hm_deep_body_set_columns(h._h, g.r._h, 0, None, None, None) == 0          # cleared
        rc, _, _ = _run(h, g.r, video, 0, X, C=3)
        assert rc == _lib.HM_ERR_STATE
        assert np.array_equal(g.r.body_warp(X[0], (video[0] >> 8).astype(np.uint8))[0],
                              body_ref.warp(X[0], (video[0] >> 8).astype(np.uint8), *g.map))   # the filter handle too
    finally:
        h.close()
        other.close()


def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the library uses (tests/test_handle_lifetime_gpu.py)"""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    assert path is not None, "the HIP runtime is not loaded"
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_the_deep_handle_gives_back_what_the_pass_allocated(hm):
    """Every buffer, stream and event of the pass belongs to the deep handle: 8 handles made, used and closed in turn on one
    filter leave the free device memory where it was.  A cycle allocates three blocks of 4 MiB (two copies of a run, the
    planes) and more; a handle that kept one of them would cost 28 MiB over the 7 cycles compared, the slack is 8."""
    from hydra_mi import mesh
    W = H = 512
    dm = mesh.box_mesh(40.0, 40.0, 470.0, 470.0, 60.0)
    N = dm.size()
    kf = bodystats_cases.make_filter(dm, np.zeros((H, W), np.uint8))
    try:
        r = kf.state.renderer
        X = np.repeat(np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * N)))[None], 9, axis=0)
        video = np.random.default_rng(2).integers(0, 65536, (9, H, W)).astype(np.uint16)
        free, first = [], None
        for _ in range(8):
            h = _handle(W, H, 8)
            try:
                assert _set_columns(h, r, [0, 3], [5, 70000, 200000], [1, 2, 3]) == 0, _err()
                rc, got, pl = _run(h, r, video, 0, X, C=1, planes=True)
                assert rc == 0, _err()
            finally:
                h.close()
            first = got if first is None else first
            assert np.array_equal(got, first)
            free.append(_free_device_memory())
        assert free[0] - free[-1] <= 8 << 20, "free device memory after each cycle (MiB): %s" % [f >> 20 for f in free]
    finally:
        kf.close()


# ---- the command line --------------------------------------------------------------------------------------------------
def test_cli_writes_the_deep_arrays(hm, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from hydra_mi import synth
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_kalmanfilter as cli
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    deep = (16 * video.astype(np.int64) + 100).astype(np.uint16)
    monkeypatch.chdir(tmp_path)
    ims = [Image.fromarray(p) for p in deep]
    ims[0].save("v.tif", format="TIFF", save_all=True, append_images=ims[1:])
    with open("pts.csv", "w") as f:
        f.write("a,%r,%r\nb,%r,%r\n" % (c[0] + 0.5, c[1] + 0.5, c[0] + 12.5, c[1] - 3.5))
    argv = ["v.tif", "none", "out.npz", "-s", "14", "--points", "pts.csv", "--rois", "--depth-range", "100,4180"]
    assert cli.main(argv + ["--deep-traces", "--deep-offset", "100"]) == 0
    assert "Full-depth traces: 2 cells over 4 frames" in capsys.readouterr().out
    z = np.load("out.npz")
    for key in ("deep_F_roi", "deep_F_np", "deep_dff"):
        assert z[key].shape == (F - 1, 2) and z[key].dtype == np.float64, key
    assert float(z["deep_offset"]) == 100.0 and "deep_demix_c" not in z.files
    # the window 100..4180 is 16 levels to one and maps 16 v + 100 to v.  Per pixel the full-depth value is
    # rint(16 b + 100) and the 8-bit one rint(b), b the same bilinear sample: they differ by at most (0.5 + 16 x 0.5) / 16
    assert np.isfinite(z["deep_F_roi"]).all() and np.abs(z["deep_F_roi"] / 16.0 - z["roi_F"]).max() <= 8.5 / 16.0
    # the points alone, no ROIs: their discs read from the 16-bit frames, by the same bound against the 8-bit point_means
    alone = ["v.tif", "none", "pts.npz", "-s", "14", "--points", "pts.csv", "--depth-range", "100,4180"]
    assert cli.main(alone + ["--deep-traces", "--deep-offset", "100"]) == 0
    assert "Full-depth traces: the discs of 2 points over 4 frames" in capsys.readouterr().out
    zp = np.load("pts.npz")
    assert zp["deep_point_means"].shape == (F - 1, 2) and "deep_F_roi" not in zp.files and float(zp["deep_offset"]) == 100.0
    assert np.abs(zp["deep_point_means"] / 16.0 - zp["point_means"]).max() <= 8.5 / 16.0
    assert "deep_point_means" not in z.files
    with pytest.raises(SystemExit):
        cli.main(argv + ["--deep-traces", "--stabilize"])
    assert "--stabilize rewrites" in capsys.readouterr().err
