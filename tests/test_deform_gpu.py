"""The record against the deformation of its own tissue on the device (`pytest -m gpu`): hm_body_rec_tri_maps and
hm_body_rec_tri_gain equal to the NumPy restatement (tests/deform_ref.py) in every bit and byte on records of real warps
through the small meshes of tests/test_strain_gpu.py, for every run length and chunking; the refusals; hydra_mi.deform
through the product on the planted video under a contraction, with the filter untouched; and the command line."""
import os
import sys

import numpy as np
import pytest

import body_ref
import deform_ref as ref
import strain_ref
from test_strain_gpu import _mesh, _renderer, _states

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLIVER = np.array([[47.2, 30.3], [49.4, 30.9], [48.1, 32.2]])        # a triangle of two pixels beside the grid


def _case(name):
    """-> (p, t, W, H): the single triangle in 64 x 48 (T = 1), the 24-triangle grid in 56 x 40, and that grid with a
    triangle of fewer than 4 pixels beside it (T = 25)"""
    if name == "1x1":
        _, p, t = _mesh("1x1")
        return p, t, 64, 48
    p, t = strain_ref.grid_mesh(5, 4, 6.3, 5.1, 9.0, 8.0, seed=4)
    if name == "sliver":
        p, t = np.vstack((p, SLIVER)), np.vstack((t, [[len(p), len(p) + 1, len(p) + 2]]))
    return p, t, 56, 40


def _frames(F, W, H, rng):
    """random frames in blocks of 5 x 5 px, of which three in ten are all 255 and two in ten all 0: both survive the
    bilinear warp"""
    out = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    kind = np.kron(rng.random((F, -(-H // 5), -(-W // 5))), np.ones((5, 5)))[:, :H, :W]
    out[kind < 0.3] = 255
    out[kind > 0.8] = 0
    return out


def _record(name, F, chunk=0, seed=0):
    """F random frames warped through the mesh at the states of test_strain_gpu's generator, recorded in chunks of `chunk`
    frames (0: the default) -> (renderer, map (H, W), recorded frames as fetched)"""
    p, t, W, H = _case(name)
    r = _renderer(p, t, W, H)
    rng = np.random.default_rng((seed, F, len(t)))
    states, frames = _states(p, F, rng, noise=0.2), _frames(F, W, H, rng)
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for X, f in zip(states, frames):
        r.body_warp(X, f)
    r.tune("body_rec_chunk", 0)
    tri_of = r.body_map()[0]
    assert np.array_equal(tri_of, body_ref.body_map(p, t, W, H)[0])
    regs = r.body_rec_fetch()
    m = tri_of >= 0
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    assert (int(cols[-1] - cols[0]) + 1) % 4                                  # the last dword of a box row is partial
    assert not m[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()            # pixels of the box that are off the map
    assert regs.shape == (F, H, W) and not regs[:, ~m].any()
    if F > 1:
        assert (regs[:, m] == 255).any() and (regs[:, m] == 0).any()
    if name == "sliver":
        assert 0 < np.bincount(tri_of[m], minlength=len(t)).min() < 4         # a triangle of fewer than 4 pixels
    return r, tri_of, regs


def _q(rng, F, T):
    q = rng.integers(-32767, 32768, (F, T)).astype(np.int32)
    q[rng.random((F, T)) < 0.2] = 32767
    q[rng.random((F, T)) < 0.2] = -32767
    q[rng.random((F, T)) < 0.1] = 0
    q[0, 0], q[-1, -1] = 32767, -32767
    return np.ascontiguousarray(q)


def _gains(rng, F, T):
    m = rng.integers(0, 65536, (F, T)).astype(np.uint16)
    pick = np.array([0, 1, 4095, 4096, 4097, 65535], np.uint16)
    some = rng.random((F, T)) < 0.6
    m[some] = pick[rng.integers(0, len(pick), int(some.sum()))]
    m.reshape(-1)[:min(len(pick), m.size)] = pick[:m.size]
    m[-1, -1] = 65535
    return np.ascontiguousarray(m)


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.uint64 and got[2].dtype == np.uint64
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", ["1x1", "grid", "sliver"])
def test_tri_maps_equal_the_restatement(hm, name):
    for F, chunk in ((1, 0), (5, 0), (5, 3)):                                  # one chunk, and chunks of 3 + 2 frames
        r, tri_of, regs = _record(name, F, chunk)
        T = int(tri_of.max()) + 1
        q = _q(np.random.default_rng(F + chunk), F, T)
        want = ref.tri_maps(regs, tri_of, q)
        assert want[0][tri_of >= 0].any() and not want[0][tri_of < 0].any()
        first = None
        for run in (1, 3, 64):                                                 # F runs, runs of 3 + 2, one run (the default)
            r.tune("rec_tm_frames", run)
            got = r.body_rec_tri_maps(q)
            assert got[0].shape == tri_of.shape and _same(got, want), (F, chunk, run)
            first = got if first is None else first
            assert all(g.tobytes() == f.tobytes() for g, f in zip(got, first))
        for drop in range(3):                                                  # every output NULL in turn
            keep = tuple(k for i, k in enumerate(("c", "w1", "w2")) if i != drop)
            got = r.body_rec_tri_maps(q, want=keep)
            assert got[drop] is None and all(np.array_equal(got[i], want[i]) for i in range(3) if i != drop), (F, chunk, drop)
        assert r.body_rec_tri_maps(q, want=()) == (None, None, None)
        assert np.array_equal(r.body_rec_fetch(), regs)                        # the record as it was
        r.close()


def test_tri_maps_tune_key(hm):
    r, tri_of, regs = _record("grid", 1)
    for bad in (0, 257):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_tm_frames must be in 1\.\.256"):
            r.tune("rec_tm_frames", bad)
    r.tune("rec_tm_frames", 256)
    q = _q(np.random.default_rng(2), 1, 24)
    assert _same(r.body_rec_tri_maps(q), ref.tri_maps(regs, tri_of, q))
    r.close()


@pytest.mark.parametrize("name", ["1x1", "grid", "sliver"])
def test_tri_gain_equals_the_restatement(hm, name):
    # a lane rewrites 8 consecutive frames of a chunk: 11 = 8 + 3 in one chunk, and chunks of 9 (8 + 1) and 2 frames
    for F, chunk in ((1, 0), (11, 0), (11, 9)):
        r, tri_of, regs = _record(name, F, chunk)
        T = int(tri_of.max()) + 1
        rng = np.random.default_rng(F + chunk)
        assert r.body_rec_tri_gain(np.full((F, T), 4096, np.uint16)) == 0
        assert np.array_equal(r.body_rec_fetch(), regs)                        # the identity: every byte as it was
        m = _gains(rng, F, T)
        want, clipped = ref.tri_gain(regs, tri_of, m)
        if F > 1:
            assert clipped > 0 and (want != regs).any()
        r.tune("rec_scratch_bytes", 1)                                         # (the call takes no scratch: the key changes nothing)
        assert r.body_rec_tri_gain(m) == clipped
        r.tune("rec_scratch_bytes", 16 << 20)
        got = r.body_rec_fetch()
        assert np.array_equal(got, want), (F, chunk, np.argwhere(got != want)[:5])
        assert not got[:, tri_of < 0].any()
        q = _q(rng, F, T)
        assert _same(r.body_rec_tri_maps(q), ref.tri_maps(want, tri_of, q))    # the maps see the rewritten record
        # again on what is there, and down to nothing
        m2 = _gains(rng, F, T)
        want2, clipped2 = ref.tri_gain(want, tri_of, m2)
        assert r.body_rec_tri_gain(m2) == clipped2 and np.array_equal(r.body_rec_fetch(), want2)
        assert r.body_rec_tri_gain(np.zeros((F, T), np.uint16)) == 0 and not r.body_rec_fetch().any()
        r.close()


def test_refusals_leave_the_record_usable(hm):
    from hydra_mi import _lib
    F = 5
    r, tri_of, regs = _record("grid", F, 3)
    T = 24
    L, p = _lib.lib(), _lib.ptr
    rng = np.random.default_rng(9)
    q, m = _q(rng, F, T), _gains(rng, F, T)
    want = ref.tri_maps(regs, tri_of, q)
    c, w1, w2 = np.empty(tri_of.shape, np.int64), np.empty(tri_of.shape, np.uint64), np.empty(tri_of.shape, np.uint64)
    n = np.zeros(1, np.uint64)

    def still_good():
        assert _same(r.body_rec_tri_maps(q), want) and np.array_equal(r.body_rec_fetch(), regs)

    for bad in (T - 1, T + 1):
        assert L.hm_body_rec_tri_maps(r._h, bad, p(q), p(c), p(w1), p(w2)) == -1
        assert b"%d triangles given, the mesh has %d" % (bad, T) in L.hm_last_error()
        assert L.hm_body_rec_tri_gain(r._h, bad, p(m), p(n)) == -1
        assert b"%d triangles given, the mesh has %d" % (bad, T) in L.hm_last_error()
        still_good()
    for v in (32768, -32768):
        bad = q.copy()
        bad[3, 7] = v
        bad[4, 0] = v                                                          # (the first offender in the call's order is named)
        with pytest.raises(RuntimeError, match=r"code -1.*q %d \(frame 3, triangle 7\) outside -32767\.\.32767" % v):
            r.body_rec_tri_maps(bad)
        still_good()
    assert L.hm_body_rec_tri_maps(r._h, T, None, p(c), p(w1), p(w2)) == -1 and b"NULL handle or traces" in L.hm_last_error()
    assert L.hm_body_rec_tri_gain(r._h, T, None, p(n)) == -1 and b"NULL handle or gains" in L.hm_last_error()
    assert L.hm_body_rec_tri_maps(None, T, p(q), p(c), p(w1), p(w2)) == -1
    assert L.hm_body_rec_tri_gain(None, T, p(m), p(n)) == -1
    still_good()
    for wrong in (q.astype(np.int64), q[:4], q[:, :23], q.reshape(-1)):
        with pytest.raises(ValueError, match="need int32, frames x triangles"):
            r.body_rec_tri_maps(wrong)
    for wrong in (m.astype(np.int32), m[:4], m[:, :23]):
        with pytest.raises(ValueError, match="need uint16, frames x triangles"):
            r.body_rec_tri_gain(wrong)
    still_good()
    # a good gain without a count, through the C ABI
    assert L.hm_body_rec_tri_gain(r._h, T, p(m), None) == 0
    now = ref.tri_gain(regs, tri_of, m)[0]
    assert np.array_equal(r.body_rec_fetch(), now)
    # no frame recorded, and before begin: code -3 with the call's name; the record then takes frames and works
    pp, _, W, H = _case("grid")
    X = _states(pp, 1, rng, noise=0.2)[0]
    for state in ("no frame", "no record"):
        if state == "no frame":
            r.body_rec_begin()
            why = "no frame recorded"
        else:
            r.body_rec_end()
            why = "hm_body_rec_begin first"
        assert L.hm_body_rec_tri_maps(r._h, T, p(q), p(c), p(w1), p(w2)) == -3
        assert b"hm_body_rec_tri_maps" in L.hm_last_error() and why.encode() in L.hm_last_error()
        assert L.hm_body_rec_tri_gain(r._h, T, p(m), p(n)) == -3
        assert b"hm_body_rec_tri_gain" in L.hm_last_error() and why.encode() in L.hm_last_error()
        if state == "no record":
            r.body_rec_begin()
        reg = r.body_warp(X, now[1])[0]
        assert r.body_rec_count() == 1
        assert _same(r.body_rec_tri_maps(q[:1]), ref.tri_maps(reg[None], tri_of, q[:1]))
        g1, n1 = ref.tri_gain(reg[None], tri_of, m[:1])
        assert r.body_rec_tri_gain(m[:1]) == n1 and np.array_equal(r.body_rec_fetch(), g1)
    r.close()


def test_correct_on_the_planted_scene_equals_the_restatement_and_leaves_the_filter_alone(hm):
    """The planted video under the contraction of contracting_states, recorded through the grid mesh at rest (the frames
    are in the body frame already) and corrected at the contracting states: gains and counts equal the run on the
    restatement bit for bit, the maps to 1e-12, the artifact goes, and the filter's next frame does not change by a bit."""
    import bodystats_cases as cases
    from hydra_mi import body, deform, mesh
    p, t, tri_of = ref.planted_triangles()
    F = 299
    states = ref.contracting_states(0, p, F)
    ids = body_ref.body_map(p, t, tri_of.shape[1], tri_of.shape[0])[3]
    J = strain_ref.strain_tri(states, p, ids)[:, :, 0]
    assert ref.J_LO <= J.min() and J.max() <= ref.J_HI and J.min() < 0.75
    d = ref.contracting_video(0, 1.0, J=np.concatenate((J, J[-1:])))
    assert d["saturated"] < 0.01
    video = d["video"][:F]
    N = len(p)
    rest = np.concatenate((np.asarray(p, np.float32).astype(np.float64).reshape(-1), np.zeros(2 * N)))
    nxt = d["video"][F]                                                        # the frame the filter sees next
    flow = np.zeros(video[0].shape + (2,), np.float32)
    runs = {}
    for fix in (False, True):
        kf = cases.make_filter(mesh.Mesh(p, t, 15.5), video[0])
        b = body.BodyReadout(kf, keep=True)
        assert np.array_equal(b.tri_of_pixel, tri_of)
        regs = np.array([b.registered(rest, f) for f in video])
        assert np.array_equal(regs, np.where((tri_of >= 0)[None], video, 0))
        if fix:
            got = deform.correct(b, states)
            rb = ref.RefBody(regs, tri_of, p, t)
            want = deform.correct(rb, states)
            assert np.array_equal(got["J"], J) and np.array_equal(want["J"], J)
            assert np.array_equal(got["gain"], want["gain"]) and got["gain"].dtype == np.uint16 and got["clipped"] == want["clipped"]
            assert got["gamma"] == want["gamma"] and got["fitted"] and got["fit_r2"] == want["fit_r2"]
            for key in ("r_before", "r_after"):
                assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])) and np.array_equal(np.isnan(got[key]), tri_of < 0)
                assert np.nanmax(np.abs(got[key] - want[key])) <= 1e-12
            assert np.array_equal(b.r.body_rec_fetch(), rb.regs)
            on = tri_of >= 0
            mb, ma = np.median(np.abs(got["r_before"][on])), np.median(np.abs(got["r_after"][on]))
            print("gamma %.4f (r2 %.3f), %d clipped, median |r| %.4f -> %.4f" % (got["gamma"], got["fit_r2"], got["clipped"], mb, ma))
            assert ma < mb
        e = kf.compute(nxt, flow, (nxt > 0).astype(np.uint8))
        runs[fix] = (kf.state.X.copy(), kf.niter, np.array(e[:4], np.float64), np.array(kf.state.W, np.float64).copy())
        kf.close()
    (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) = runs[False], runs[True]
    assert np.array_equal(Xa, Xb) and ia == ib and np.array_equal(ea, eb, equal_nan=True) and np.array_equal(Wa, Wb)


def test_cli_deform_correct(hm, tmp_path):
    """The 64^2 stretching disk of the strain CLI test: --deform-correct --rois --strain writes the deform_* arrays; with
    --deform-gamma 0 every gain is 4096 and every other array is that of the run without the switch, bit for bit."""
    from hydra_mi import synth
    sys.path.insert(0, ROOT)
    import run_kalmanfilter
    n, F = 64, 6
    video = synth.disk_video(n, F, "translate_leftup_stretch", 0)[0]
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    common = ["-s", "10", "--find-points", "3", "--find-radius", "4", "--find-score", "std", "--rois", "--strain"]
    out = {}
    for key, more in (("plain", []), ("zero", ["--deform-correct", "--deform-gamma", "0"]), ("fit", ["--deform-correct"])):
        fn = str(tmp_path / (key + ".npz"))
        assert run_kalmanfilter.main([vid, str(tmp_path / "noflow"), fn] + common + more) == 0
        out[key] = np.load(fn)
    new = {"deform_gamma", "deform_fit_r2", "deform_gain", "deform_clipped", "deform_r_before", "deform_r_after"}
    K, T = out["plain"]["X"].shape[0], out["plain"]["t"].shape[0]
    for key in ("zero", "fit"):
        z = out[key]
        assert set(z.files) == set(out["plain"].files) | new
        assert z["deform_gain"].shape == (K, T) and z["deform_gain"].dtype == np.uint16
        assert z["deform_r_before"].shape == (n, n) and z["deform_r_before"].dtype == np.float32
        assert z["deform_r_after"].shape == (n, n) and z["deform_r_after"].dtype == np.float32
        assert z["deform_gamma"].shape == () and z["deform_fit_r2"].shape == () and z["deform_clipped"].dtype == np.uint64
        assert 0.0 <= float(z["deform_gamma"]) <= 3.0
    z = out["zero"]
    assert (z["deform_gain"] == 4096).all() and float(z["deform_gamma"]) == 0.0 and int(z["deform_clipped"]) == 0
    assert np.array_equal(z["deform_r_before"], z["deform_r_after"], equal_nan=True)
    for key in out["plain"].files:
        assert out["plain"][key].dtype == z[key].dtype and out["plain"][key].tobytes() == z[key].tobytes(), key
    with pytest.raises(SystemExit):
        run_kalmanfilter.main([vid, str(tmp_path / "noflow"), str(tmp_path / "x.npz"), "-s", "10", "--deform-correct"])
