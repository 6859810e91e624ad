"""The body-frame readout with the animal on the frame's border (`pytest -m gpu`): every hm_body_* call family on the
scenes of tests/border_cases.py -- a map that is the whole frame, a disk over all four borders, a map in the last corner,
maps of one column at column 0 and at the last column, of one pixel and of none -- against the restatement the family
already has (tests/*_ref.py) and nothing new, and one record of 2100 frames.  Every comparison is np.array_equal, or
equality of the bits where the restatement returns floats.  What these scenes reach that the interior ones cannot is shown
on the CPU by tests/test_border_cases_cpu.py.

Every family runs on every scene.  On `empty` a call that takes seeds has nothing to take: every seed is refused, which is
what is asserted there; all other calls run on its record of one-pixel frames and equal the restatement on an empty map
(zeros; NaN where a statistic has no pixel).  One filter per scene serves the whole module; every test starts its own
record (7 frames in chunks of 2, runs of 3 frames per workgroup, so runs cross chunks) and leaves none."""
import time

import numpy as np
import pytest

import body_ref
import bodystats_cases
import bodystats_ref
import border_cases as cases
import deform_ref
import demix_ref
import detrend_ref
import events_ref
import network_null_ref
import network_ref
import pca_ref
import residual_ref
import roi_ref
import stab_ref
import stabfield_ref

pytestmark = pytest.mark.gpu
F = 7
GRIDS = ((4, 0), (7, 1), (16, 3), (64, 8))
DET = dict(half=3, q=20, floor=16, gain=255)            # tests/test_events_gpu.py
G, LAM, SMIN = 0.9, 2.5, 4.0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Rig:
    """A filter on a scene, its map and its record by the restatement"""

    def __init__(self, name):
        self.name = name
        self.dm, self.Xs, self.frames, f0 = cases.scene(name)
        self.kf = bodystats_cases.make_filter(self.dm, f0)
        self.r = self.kf.state.renderer
        self.W, self.H = cases.size(name)
        self.T = self.dm.t.shape[0]
        self.map = body_ref.body_map(np.asarray(self.dm.p, np.float32), self.dm.t, self.W, self.H)
        self.tri_of = self.map[0]
        self.m = self.tri_of >= 0
        self.box = cases.box_of(self.m)
        self.pairs = cases.record_pairs(name, F)
        self.regs = np.array([body_ref.warp(X, f, *self.map) for X, f in self.pairs])
        self.r.tune("rec_tp_frames", 3)

    def fill(self):
        """(re)start the record with the 7 frames -> what the warps returned"""
        r = self.r
        r.tune("body_rec_chunk", 2)
        r.body_rec_begin()
        got = np.array([r.body_warp(X, f)[0] for X, f in self.pairs])
        r.tune("body_rec_chunk", 0)
        assert r.body_rec_count() == F
        return got

    def unchanged(self):
        assert np.array_equal(self.r.body_rec_fetch(), self.regs)

    def seeds(self):
        """the map's first and last pixel in raster order as (column, row)"""
        rows, cols = np.nonzero(self.m)
        return np.array([(cols[0], rows[0]), (cols[-1], rows[-1])], np.int32)


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


# ---- map, warp, sums -------------------------------------------------------------------------------------------------
def test_the_handle_accepts_every_mesh_as_it_is(rigs):
    """(tests/border_cases.py: no mesh had to be swapped, the smallest has 4 vertices and 2 triangles)"""
    for name in cases.NAMES:
        assert rigs(name).r.n == rigs(name).dm.size()


@pytest.mark.parametrize("name", cases.NAMES)
def test_map_and_warp(rigs, name):
    from hydra_mi import _lib
    from hydra_mi.pipeline import DeviceBuffer
    g = rigs(name)
    r, m, H, W, T = g.r, g.m, g.H, g.W, g.T
    tri, cnt = r.body_map()
    assert np.array_equal(tri, g.tri_of) and np.array_equal(cnt.astype(np.uint64), body_ref.counts(g.tri_of, T))
    if name == "empty":
        assert (tri == -1).all()
    rng = np.random.default_rng(7)
    L = 9
    labels = rng.integers(-1, L, (H, W)).astype(np.int32)
    labels[0, 0], labels[-1, -1] = L - 1, 0
    keys = body_ref.label_keys(labels, g.tri_of)
    assert np.array_equal(r.body_set_labels(labels, L).astype(np.uint64), body_ref.counts(keys, L))
    d_f, d_o, d_s = DeviceBuffer(H * W), DeviceBuffer(3 * H * W), DeviceBuffer(8 * (T + L))
    white = np.full((H, W), 255, np.uint8)
    for X, f in list(zip(g.Xs, g.frames)) + [(g.Xs[0], white)]:
        want = body_ref.warp(X, f, *g.map)
        reg, ts, ls = r.body_warp(X, f)
        assert np.array_equal(reg, want)
        assert np.array_equal(ts, body_ref.sums(want, g.tri_of, T)) and np.array_equal(ls, body_ref.sums(want, keys, L))
        d_f.upload(np.ascontiguousarray(f))
        r.body_warp_dev(X, d_f.ptr, d_o.ptr, 3, d_s.ptr, d_s.ptr + 8 * T)
        _lib.check(_lib.lib().hm_ctx_sync(r._h), "hm_ctx_sync")
        out, sums = np.empty((H, W, 3), np.uint8), np.empty(T + L, np.uint64)
        d_o.download(out)
        d_s.download(sums)
        assert np.array_equal(out, np.repeat(want[:, :, None], 3, axis=2))
        assert np.array_equal(sums[:T], ts) and np.array_equal(sums[T:], ls)
    assert (reg[m] == 255).all() and (reg[~m] == 0).all()        # the mesh at rest on a white frame: the map itself
    for b in (d_f, d_o, d_s):
        b.close()
    r.body_set_labels(None, 0)


@pytest.mark.parametrize("name", cases.NAMES)
def test_statistics_images_and_peaks(rigs, name):
    g = rigs(name)
    r, m = g.r, g.m
    r.body_stats_begin()
    regs = [r.body_warp(X, f)[0] for X, f in g.pairs[:4]]
    assert np.array_equal(np.array(regs), g.regs[:4])
    want = bodystats_ref.accumulate(g.regs[:4], m)
    assert r.body_stats_count() == 4
    for a, b in zip(r.body_stats_fetch(), want):
        assert np.array_equal(a, b)
    if name in ("full33x17", "disk_over"):
        assert want[2][3][:, 0].sum() == 0 and want[2][0][:, -1].sum() == 0      # no SW of column 0, no E of the last
        assert want[2][0][:, 0].any() and want[2][3][:, -1].any()
    imgs = bodystats_ref.images(*want, 4, m)
    got = r.body_stats_images()
    for a, b in zip(got[:3], imgs[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(got[3], imgs[3])
    assert all(np.isnan(a[~m]).all() for a in got[:3]) and (got[3][~m] == 0).all()
    for which in ("corr", "std", "range"):
        score = bodystats_ref.score_image(which, *imgs)
        for radius in (1, 3, 16):
            for min_score in (-np.inf,) + ((float(np.median(score[m])),) if m.any() else (0.0,)):
                wi, ws = bodystats_ref.peaks_fast(score, m, radius, min_score)
                gi, gs, n = r.body_stats_peaks(which, radius, min_score)
                assert n == len(wi), (which, radius, min_score)
                assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws)), (which, radius, min_score)
                if name == "empty":
                    assert n == 0
    if name == "empty":
        assert all(np.isnan(a).all() for a in got[:3])
    r.body_stats_end()


# ---- the record --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_record_fetch_label_seed_weighted_sums_and_trace_products(rigs, name):
    g = rigs(name)
    r, m, H, W = g.r, g.m, g.H, g.W
    assert np.array_equal(g.fill(), g.regs)
    assert np.array_equal(r.body_rec_fetch(), g.regs) and np.array_equal(r.body_rec_fetch(1, 4), g.regs[1:5])
    assert np.array_equal(r.body_rec_fetch(F - 1, 1), g.regs[F - 1:]) and r.body_rec_fetch(F, 0).shape[0] == 0
    assert not g.regs[:, ~m].any()
    assert g.regs[:, m].any() == (name != "empty")
    if name in ("full33x17", "disk_over"):
        assert g.regs[:, :, 0].any() and g.regs[:, :, -1].any() and g.regs[:, 0].any() and g.regs[:, -1].any()
    rng = np.random.default_rng(11)
    labels = rng.integers(-1, 3, (H, W)).astype(np.int32)
    ls = r.body_rec_label_sums(labels, 3)
    assert ls.dtype == np.uint64 and np.array_equal(ls, roi_ref.label_sums(g.regs, m, labels, 3))
    if name == "empty":
        assert not ls.any()
        g.unchanged()
        for seed in ((0, 0), (7, 7), (15, 15)):
            sd = np.array([seed], np.int32)
            for call in (lambda: r.body_rec_seed_sums(sd, 3.0, 6.0, 8.5, 4),
                         lambda: r.body_rec_weighted_sums(sd, np.ones((1, 9, 9), np.uint16), 4),
                         lambda: r.body_rec_trace_products(sd, np.ones((F, 1), np.int32), 4)):
                with pytest.raises(RuntimeError, match=r"code -1.*seed 0 \(column %d, row %d\) is not a pixel of the body map" % seed):
                    call()
        g.unchanged()
        r.body_rec_end()
        return
    g.unchanged()
    seeds = g.seeds()
    P = len(seeds)
    if name == "full33x17":
        assert seeds.tolist() == [[0, 0], [W - 1, H - 1]]          # the frame's corners
    for (rd, ri, ro, R) in ((3.0, 6.0, 8.5, 4), (1.0, 0.0, 2.0, 16)):
        got, want = r.body_rec_seed_sums(seeds, rd, ri, ro, R), roi_ref.seed_sums(g.regs, m, seeds, rd, ri, ro, R)
        for key in ("n_T", "n_G", "T", "G", "U", "w1", "w2", "c", "u1", "u2"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, R)
        g.unchanged()
    for R in (4, 32):
        S = 2 * R + 1
        w = rng.integers(0, 65536, (P, S, S)).astype(np.uint16)
        w[0] = 65535
        assert np.array_equal(r.body_rec_weighted_sums(seeds, w, R), roi_ref.weighted_sums(g.regs, m, seeds, w, R)), R
        g.unchanged()
    for R in (4, 16):
        q = rng.integers(-2 ** 31, 2 ** 31, (F, P)).astype(np.int32)
        assert np.array_equal(r.body_rec_trace_products(seeds, q, R), demix_ref.trace_products(g.regs, m, seeds, q, R)), R
    g.unchanged()
    r.body_rec_end()


# ---- stabilising -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_match_frame_sums_shift_field_sums_and_warp(rigs, name):
    g = rigs(name)
    r, m, H, W, regs = g.r, g.m, g.H, g.W, g.regs
    rng = np.random.default_rng(13)
    g.fill()
    for B, S in GRIDS:
        grid = stab_ref.patch_grid(m, B)
        npatch = grid["npx"] * grid["npy"]
        assert r.body_rec_patches(B) == (grid["npx"], grid["npy"])
        noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
        got, want = r.body_rec_match(noise, B, S), stab_ref.match(regs, m, B, S, noise)
        for key in ("n_core", "A", "V1", "V2"):
            assert got[key].dtype == np.uint32 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (key, B, S)
        sub = r.body_rec_match(regs[2], B, S, 1, F - 2)
        assert all(np.array_equal(sub[key], v) for key, v in stab_ref.match(regs, m, B, S, regs[2], 1, F - 2).items())
        g.unchanged()
        sh = rng.integers(-16, 17, (F, npatch, 2)).astype(np.int8)
        sh[0, 0], sh[F - 1, npatch - 1] = (16, -16), (-16, 16)
        assert np.array_equal(r.body_rec_frame_sums(sh, B), stab_ref.frame_sums(regs, m, B, sh))
        assert np.array_equal(r.body_rec_frame_sums(), regs.astype(np.uint32).sum(0))
        g.unchanged()
        r.body_rec_shift(sh, B)
        assert np.array_equal(r.body_rec_fetch(), stab_ref.shift(regs, m, B, sh)), (B, S)
        small = rng.integers(-1, 2, (F, npatch, 2)).astype(np.int8)
        g.fill()
        r.body_rec_shift(small, B)
        want = stab_ref.shift(regs, m, B, small)
        assert np.array_equal(r.body_rec_fetch(), want), (B, S)
        if name in ("full33x17", "disk_over", "corner"):
            assert (want != regs).any() and want.any()
        g.fill()
        q = rng.integers(-256, 257, (F, npatch, 2)).astype(np.int16)
        q[0, 0], q[F - 1, npatch - 1] = (256, -256), (-256, 256)
        valid = (rng.random((F, npatch)) < 0.8).astype(np.uint8)
        valid[0, 0] = valid[F - 1, npatch - 1] = 1
        assert np.array_equal(r.body_rec_field_sums(q, valid, B), stabfield_ref.field_sums(regs, m, B, q, valid)), (B, S)
        g.unchanged()
        r.body_rec_warp(q, valid, B)
        assert np.array_equal(r.body_rec_fetch(), stabfield_ref.warp(regs, m, B, q, valid)), (B, S)
        q //= 16                                                  # within a pixel: values stay on the map
        g.fill()
        r.body_rec_warp(q, valid, B)
        want = stabfield_ref.warp(regs, m, B, q, valid)
        assert np.array_equal(r.body_rec_fetch(), want), (B, S)
        if name in ("full33x17", "disk_over", "corner"):
            assert (want != regs).any() and want.any()
        g.fill()
    r.body_rec_end()


# ---- planes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_baseline_event_and_residual_planes(rigs, name):
    g = rigs(name)
    r, m, H, W, regs = g.r, g.m, g.H, g.W, g.regs
    g.fill()
    want = {(what, half, q): detrend_ref.planes(regs, m, what, half, q, 16, 255)
            for what in range(4) for half, q in ((0, 10), (2, 50), (F + 3, 10))}
    for run in (1, 3):
        r.tune("rec_bl_frames", run)
        for key, w in want.items():
            assert np.array_equal(r.body_rec_planes(key[0], key[1], key[2], 16, 255), w), (run, key)
        g.unchanged()
        assert np.array_equal(r.body_rec_planes(3, 2, 50, 16, 255, 1, F - 2), want[3, 2, 50][1:F - 1]), run
    r.tune("rec_bl_frames", 256)
    g.unchanged()
    b = g.box
    box = (b["r0"], b["r0"] + b["bh"], b["c0"], b["c0"] + b["bw"])
    E, n, S = events_ref.video(detrend_ref.planes(regs, m, 0, **DET), box, G, LAM, SMIN)
    assert np.array_equal(r.body_rec_event_planes(0, g=G, lam=LAM, **DET), E)
    cnt, tot = r.body_rec_event_sums(0, g=G, lam=LAM, s_min=SMIN, **DET)
    assert np.array_equal(cnt, n) and np.array_equal(_bits(tot), _bits(S))
    if name in ("full33x17", "disk_over", "corner"):
        assert E.any()
    g.unchanged()
    rng = np.random.default_rng(17)
    L = 3
    lab = rng.integers(-1, L, (2, H, W)).astype(np.int32)
    lab[:, 0, 0], lab[:, -1, -1] = (0, 1), (2, 0)
    wt = rng.integers(0, 65536, lab.shape).astype(np.uint16)
    tr = rng.integers(-450 * 256, 450 * 256, (F, L)).astype(np.int32)
    blank = ((rng.random((H, W)) < 0.1) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    for weights, bl, offset in ((wt, None, 64), (None, blank, 0), (wt, blank, 255)):
        got, w = r.body_rec_residual_planes(lab, weights, tr, bl, offset), residual_ref.planes(regs, m, lab, weights, tr, bl, offset)
        assert np.array_equal(got[0], w[0]) and got[1] == w[1], offset
    p, c = r.body_rec_residual_planes(lab, wt, tr, blank, 64, 1, F - 2)
    w = residual_ref.planes(regs[1:F - 1], m, lab, wt, tr[1:F - 1], blank, 64)
    assert np.array_equal(p, w[0]) and c == w[1]
    g.unchanged()
    r.body_rec_end()


# ---- maps ----------------------------------------------------------------------------------------------------------------
def _q(rng, n, L):
    q = rng.integers(-32767, 32768, (n, L)).astype(np.int32)
    q[rng.random((n, L)) < 0.15] = 0
    q[0, 0], q[-1, -1] = 32767, -32767
    return np.ascontiguousarray(q)


@pytest.mark.parametrize("name", cases.NAMES)
def test_trace_maps_trace_null_tri_maps_tri_gain_and_gram(rigs, name):
    g = rigs(name)
    r, m, H, W, T, regs = g.r, g.m, g.H, g.W, g.T, g.regs
    rng = np.random.default_rng(19)
    g.fill()
    q = _q(rng, F, 9)
    got, want = r.body_rec_trace_maps(q), network_ref.trace_maps(regs, m, q)
    assert got["c"].shape == (9, H, W)
    for key, w in zip(("c", "w1", "w2"), want):
        assert got[key].dtype == w.dtype and np.array_equal(got[key], w), key
    g.unchanged()
    q = _q(rng, F, 10)
    vb = np.array([network_null_ref.vb_of(q[:, s]) for s in range(10)])
    got = r.body_rec_trace_null(q, vb)
    if name == "empty":
        # (no pixel: the header's "NaN for a map without a pixel"; the restatement's maximum over nothing does not exist)
        assert np.isnan(got["tmax"]).all() and np.isnan(got["tmin"]).all() and got["tmax"].shape == (10,)
        assert not got["ge"].any() and not got["le"].any()
    else:
        want = network_null_ref.trace_null_np(regs, m, q, vb)
        for key in ("tmax", "tmin", "ge", "le"):
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    g.unchanged()
    qt = _q(rng, F, T)
    got, want = r.body_rec_tri_maps(qt), deform_ref.tri_maps(regs, g.tri_of, qt)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    g.unchanged()
    got, want = r.body_rec_gram(), pca_ref.gram(regs)
    assert got["G"].dtype == np.int64 and np.array_equal(got["G"], want[0]) and np.array_equal(got["s1"], want[1])
    got, want = r.body_rec_gram(1, stride=2), pca_ref.gram(regs[1::2])
    assert got["G"].shape == (3, 3) and np.array_equal(got["G"], want[0]) and np.array_equal(got["s1"], want[1])
    got, want = r.body_rec_gram(0, 4, 2), pca_ref.gram(regs[0::2])
    assert np.array_equal(got["G"], want[0]) and np.array_equal(got["s1"], want[1])
    if name == "empty":
        assert not got["G"].any() and not got["s1"].any()
    g.unchanged()
    assert r.body_rec_tri_gain(np.full((F, T), 4096, np.uint16)) == 0
    g.unchanged()
    gains = rng.integers(0, 65536, (F, T)).astype(np.uint16)
    gains[rng.random((F, T)) < 0.5] = 4097
    want, clipped = deform_ref.tri_gain(regs, g.tri_of, gains)
    assert r.body_rec_tri_gain(gains) == clipped
    assert np.array_equal(r.body_rec_fetch(), want)
    if name == "empty":
        assert clipped == 0 and not want.any()          # no triangle has a pixel: nothing to gain
    r.body_rec_end()


# ---- one long record -----------------------------------------------------------------------------------------------------
LONG = 2100
#: the frames whose baseline planes are compared with detrend_ref.planes: windows clipped at the start, the first clipped at
#: neither end and all 52 of full length (frames 1024 .. 1075), windows clipped at the end.  The restatement takes 2 ms a
#: frame and kind (np.partition of the window); all 2100 would take 8 s.  The device computes all 2100 frames in one call.
LONG_SLICES = ((0, 40), (1000, 100), (2060, 40))


def test_one_long_record(hm):
    """Scene "16" with the mesh at rest, 2100 frames in chunks of the default size: frames 1024 and above are the second
    trip of k_rec_label_sums' y-grid and of k_rec_gram_fix' rows; a window of 2 x 1024 + 1 frames is full at frames
    1024 .. 1075, and pixel (7, 7), held at 200, puts all 2049 of its values into one bin."""
    dm, _, _, f0 = bodystats_cases.scene("16")
    kf = bodystats_cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    p = np.asarray(dm.p, np.float32).astype(np.float64)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * p.shape[0])))
    frames = np.random.default_rng(LONG).integers(0, 256, (LONG, 16, 16), dtype=np.uint8)
    frames[:, 6:9, 6:9] = 200
    frames[:, 7, 8], frames[:, 8, 7] = 0, 255
    t0 = time.perf_counter()
    r.body_rec_begin()
    for f in frames:
        r.body_warp(rest, f)
    regs = r.body_rec_fetch()
    print("recording %d frames: %.2f s" % (LONG, time.perf_counter() - t0))
    assert np.array_equal(regs, np.where(m[None], frames, 0)) and m[7, 7] and m[7, 8] and m[8, 7]
    labels = np.random.default_rng(1).integers(-1, 3, (16, 16)).astype(np.int32)
    assert np.array_equal(r.body_rec_label_sums(labels, 3), roi_ref.label_sums(regs, m, labels, 3))
    got, want = r.body_rec_gram(0, LONG), pca_ref.gram(regs)
    assert np.array_equal(got["G"], want[0]) and np.array_equal(got["s1"], want[1])
    got, want = r.body_rec_gram(0, 1030, 2), pca_ref.gram(regs[0::2][:1030])
    assert np.array_equal(got["G"], want[0]) and np.array_equal(got["s1"], want[1])
    for what in (1, 3):
        first = None
        for run in (7, 1 << 20):
            r.tune("rec_bl_frames", run)
            got = r.body_rec_planes(what, 1024, 50, 16, 255)
            for k0, n in LONG_SLICES:
                assert np.array_equal(got[k0:k0 + n], detrend_ref.planes(regs, m, what, 1024, 50, 16, 255, k0, n)), (what, run, k0)
            first = got if first is None else first
            assert got.tobytes() == first.tobytes()                # every frame: the same bytes for both run lengths
        assert (got[:, 7, 7] == (200 if what == 1 else 0)).all() and not got[:, ~m].any()
        if what == 1:
            assert (got[:, 8, 7] == 255).all() and not got[:, 7, 8].any()
    r.tune("rec_bl_frames", 256)
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()
