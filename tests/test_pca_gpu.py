"""The Gram matrix of the record's frames on the device (`pytest -m gpu`): hm_body_rec_gram equal to the int64 product of
the fetched frames for every number of frames, every subset and every run length, at the edge of its 32-bit
accumulators, its refusals, the record before and after; a slipped frame found by its score; hydra_mi.pca through the
product on the planted scene against tests/pca_ref.py, and the CLI.  Every integer comparison is an equality."""
import os
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import network_ref
import pca_ref as ref
import roi_ref
from test_network_gpu import _record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, F = 48, 64, 70
RUNS = (64, 192, 131008)                # about 29 runs with the last partial, about 10, one


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _product(frames):
    """(G, s1) of frames (n, H, W) uint8 as int64 products"""
    X = frames.reshape(len(frames), -1).astype(np.int64)
    return X @ X.T, X.sum(1).astype(np.uint64)


def _same(got, frames):
    G, s1 = _product(frames)
    assert got["G"].dtype == np.int64 and got["s1"].dtype == np.uint64
    assert got["G"].shape == G.shape and got["s1"].shape == s1.shape
    return np.array_equal(got["G"], G) and np.array_equal(got["G"], got["G"].T) and np.array_equal(got["s1"], s1)


@pytest.fixture(scope="module")
def record(hm):
    """70 frames recorded in chunks of 3: chunk seams fall inside every tile"""
    kf, r, m, regs = _record(F=F, chunk=3)
    assert len({int(v) for v in regs.reshape(F, -1).astype(np.int64).sum(1)}) > F // 2         # frames that differ
    yield kf, r, m, regs
    kf.close()


def test_gram_equals_the_product_for_every_size_and_run(record):
    kf, r, m, regs = record
    full = {}
    for run in RUNS:
        r.tune("rec_gram_bytes", run)
        # one frame; a partial tile; a full one; a second, partial tile; a third tile; a second quarter of 64 x 64, the
        # second wave's, partial (the blocks of workgroups: test_gram_across_the_blocks_of_workgroups)
        for n in (1, 7, 16, 17, 33, 70):
            got = r.body_rec_gram(0, n)
            assert _same(got, regs[:n]), (run, n)
        full[run] = got
    assert all(full[run]["G"].tobytes() == full[RUNS[0]]["G"].tobytes() for run in RUNS)
    G, s1 = _product(regs)
    assert not np.array_equal(G[:16, 16:32], G[:16, 16:32].T)             # an off-diagonal tile that a swapped C-write would show in
    # NULL outputs, the default range
    only = r.body_rec_gram(0, 33, want=("G",))
    assert sorted(only) == ["G"] and np.array_equal(only["G"], G[:33, :33])
    only = r.body_rec_gram(0, 33, want=("s1",))
    assert sorted(only) == ["s1"] and np.array_equal(only["s1"], s1[:33])
    assert r.body_rec_gram(0, 33, want=()) == {}
    assert _same(r.body_rec_gram(), regs) and _same(r.body_rec_gram(40), regs[40:]) and _same(r.body_rec_gram(1, stride=4), regs[1::4])
    assert np.array_equal(r.body_rec_fetch(), regs)                        # the record as it was


def test_gram_across_the_blocks_of_workgroups(hm):
    """A workgroup owns 128 x 128 of G and a wave a quarter of 64 x 64: 300 frames are three blocks with the last partial
    and one, (0, 2), that does not touch the diagonal; 64 and 65 are a full quarter and the first frame of a second, 128
    and 129 a full block and the first frame of a second, the first block off the diagonal; 257 starts the third."""
    kf, r, m, regs = _record(F=300, chunk=7)
    G, s1 = _product(regs)
    assert not np.array_equal(G[:128, 128:256], G[:128, 128:256].T)
    full = {}
    for run in RUNS:
        r.tune("rec_gram_bytes", run)
        for n in (64, 65, 128, 129, 257, 300):
            got = r.body_rec_gram(0, n)
            assert np.array_equal(got["G"], G[:n, :n]) and np.array_equal(got["s1"], s1[:n]), (run, n)
        full[run] = got
    assert all(full[run]["G"].tobytes() == full[RUNS[0]]["G"].tobytes() for run in RUNS)
    sub = r.body_rec_gram(2, 140, 2)
    assert np.array_equal(sub["G"], G[2::2, 2::2][:140, :140]) and np.array_equal(sub["s1"], s1[2::2][:140])
    assert np.array_equal(r.body_rec_gram(0, 300, want=("s1",))["s1"], s1)
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()


@pytest.mark.parametrize("k0,n,stride", [(3, 5, 13), (69, 1, 1), (1, 23, 3)])
def test_gram_of_a_subset(record, k0, n, stride):
    kf, r, m, regs = record
    sub = regs[k0::stride][:n]
    assert len(sub) == n
    for run in RUNS:
        r.tune("rec_gram_bytes", run)
        assert _same(r.body_rec_gram(k0, n, stride), sub), run


def test_gram_at_the_edge_of_the_accumulators(hm):
    """A box of more than 131008 bytes: a black frame is x = -128 in every byte, and its product with itself over a full run
    of 131008 bytes is 128^2 x 131008 = 2^31 - 1 048 576, the largest a 32-bit sum has to hold; one step more would wrap."""
    from hydra_mi import mesh
    Hb, Wb = 384, 400
    dm = mesh.disk_mesh(199.5, 191.5, 185.0, 60.0)
    rng = np.random.default_rng(5)
    f0 = rng.integers(0, 256, (Hb, Wb), dtype=np.uint8)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    nb = (bw + 3) // 4 * 4 * bh
    assert nb >= 131008 + 64, (bw, bh)
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * dm.size())))
    r.body_rec_begin()
    for f in (np.zeros((Hb, Wb), np.uint8), np.full((Hb, Wb), 255, np.uint8), f0):
        r.body_warp(X, f)
    regs = r.body_rec_fetch()
    assert not regs[0].any() and (regs[1][m] == 255).all() and not regs[1][~m].any()
    assert _same(r.body_rec_gram(), regs)                                   # (the handle is fresh: the key is at its default)
    r.tune("rec_gram_bytes", 131008)
    assert _same(r.body_rec_gram(), regs)
    assert r.body_rec_gram()["G"][1, 1] == 65025 * int(m.sum())
    kf.close()


def test_gram_refusals_leave_the_record_usable(hm):
    kf, r, m, regs = _record(F=9, chunk=3)

    def good():
        return _same(r.body_rec_gram(), regs) and _same(r.body_rec_gram(2, 3, 3), regs[2::3][:3])

    assert good()
    for n in (0, 8193):                                                      # on a short record: refused on the number alone
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_gram: %d frames outside 1\.\.8192" % n):
            r.body_rec_gram(0, n)
        assert good()
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_gram: stride 0 \(need >= 1\)"):
        r.body_rec_gram(0, 3, 0)
    assert good()
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_gram: first frame -1 is negative"):
        r.body_rec_gram(-1, 3)
    assert good()
    for k0, n, stride, last in ((0, 10, 1, 9), (8, 2, 1, 9), (1, 3, 4, 9), (9, 1, 1, 9), (0, 2, 2 ** 31 - 1, 2 ** 31 - 1)):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_gram: %d frames from %d in steps of %d end at frame %d of a "
                                               r"record of 9" % (n, k0, stride, last)):
            r.body_rec_gram(k0, n, stride)
        assert good()
    for bad in (0, 63, 100, 131072):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_gram_bytes must be a multiple of 64 in 64\.\.131008"):
            r.tune("rec_gram_bytes", bad)
        assert good()
    assert np.array_equal(r.body_rec_fetch(), regs)
    # no frame recorded, and before begin: the record takes frames and gives their products afterwards
    X = np.ascontiguousarray(kf.state.X, np.float64).reshape(-1)
    for state in ("no frame", "no record"):
        if state == "no frame":
            r.body_rec_begin()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_gram.*no frame recorded"):
                r.body_rec_gram(0, 1)
        else:
            r.body_rec_end()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_gram.*hm_body_rec_begin first"):
                r.body_rec_gram(0, 1)
            r.body_rec_begin()
        reg = r.body_warp(X, regs[2])[0]
        assert r.body_rec_count() == 1 and _same(r.body_rec_gram(), reg[None])
    kf.close()


def test_gram_sees_the_record_as_rewritten(hm):
    kf, r, m, regs = _record(F=11, chunk=3)
    rng = np.random.default_rng(8)
    assert _same(r.body_rec_gram(), regs) and np.array_equal(r.body_rec_fetch(), regs)      # unchanged by the call
    B = 8
    npx, npy = r.body_rec_patches(B)
    r.body_rec_shift(rng.integers(-3, 4, (11, npx * npy, 2)).astype(np.int8), B)
    shifted = r.body_rec_fetch()
    assert not np.array_equal(shifted, regs) and _same(r.body_rec_gram(), shifted)
    r.body_rec_tri_gain(rng.integers(2048, 8193, (11, r.tri.shape[0])).astype(np.uint16))
    gained = r.body_rec_fetch()
    assert not np.array_equal(gained, shifted) and _same(r.body_rec_gram(), gained)
    assert np.array_equal(r.body_rec_fetch(), gained)
    kf.close()


def test_a_slipped_frame_has_the_lowest_score(hm):
    """12 frames of one noise texture with a little noise of their own, frame 7 recorded at a state displaced by 6 px: its
    registered frame matches no other"""
    from hydra_mi import mesh, pca
    dm = mesh.disk_mesh(31.5, 23.5, 17.0, 7.0)
    rng = np.random.default_rng(12)
    tex = rng.integers(30, 226, (H, W)).astype(np.int64)
    kf = cases.make_filter(dm, tex.astype(np.uint8))
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    N = dm.size()
    rest = np.asarray(dm.p, np.float64)
    r.body_rec_begin()
    for k in range(12):
        f = np.clip(tex + rng.integers(-8, 9, (H, W)), 0, 255).astype(np.uint8)
        p = rest + np.array([6.0, 0.0]) if k == 7 else rest
        r.body_warp(np.concatenate((p.reshape(-1), np.zeros(2 * N))), f)
    regs = r.body_rec_fetch()
    o = r.body_rec_gram()
    assert _same(o, regs)
    rr = pca.frame_similarity(o["G"], o["s1"], int(m.sum()))
    assert np.array_equal(_bits(rr), _bits(ref.frame_similarity(o["G"], o["s1"], int(m.sum()))))
    score = pca.frame_score(rr)
    print("frame scores: %s" % " ".join("%.3f" % s for s in score))
    assert int(np.argmin(score)) == 7 and score[7] < 0.5 < np.delete(score, 7).min()
    kf.close()


def test_pca_on_the_planted_scene_equals_the_restatement(hm):
    """hydra_mi.pca through the product on the planted video with ensembles as the tracker sees it: gram, centre,
    components and maps equal the restatement fed the fetched frames bit for bit."""
    from hydra_mi import body, mesh, pca
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs = network_ref.planted_scene(1, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    for X, f in zip(states, frames):
        b.registered(X, f)
    regs = b.r.body_rec_fetch()
    m = b.tri_of_pixel >= 0
    assert len(regs) == 300 and not regs[:, ~m].any()
    G, s1 = pca.gram(b)
    Gr, sr = ref.gram(regs)
    assert G.dtype == np.int64 and s1.dtype == np.uint64 and np.array_equal(G, Gr) and np.array_equal(s1, sr)
    assert np.array_equal(_bits(pca.centre(G)), _bits(ref.centre(Gr)))
    lam, U, share = pca.components(G, 4)
    lam_r, U_r, share_r = ref.components(Gr, 4)
    assert np.array_equal(_bits(lam), _bits(lam_r)) and np.array_equal(_bits(U), _bits(U_r)) and np.array_equal(_bits(share), _bits(share_r))
    rho = pca.maps(b, U)
    assert rho.shape == (4,) + m.shape and np.array_equal(_bits(rho), _bits(ref.maps(regs, m, U_r)))
    p = pca.pca(b, 4, frames=True)
    rr = ref.frame_similarity(Gr, sr, int(m.sum()))
    assert sorted(p) == ["frame_r", "frame_score", "lam", "rho", "share", "temporal"]
    assert np.array_equal(_bits(p["lam"]), _bits(lam_r)) and np.array_equal(_bits(p["share"]), _bits(share_r))
    assert np.array_equal(_bits(p["temporal"]), _bits(U_r)) and np.array_equal(_bits(p["rho"]), _bits(rho))
    assert np.array_equal(_bits(p["frame_r"]), _bits(rr)) and np.array_equal(_bits(p["frame_score"]), _bits(ref.frame_score(rr)))
    assert "frame_r" not in pca.pca(b, 1)
    print("planted scene, seed 1: shares %s" % " ".join("%.4f" % s for s in share))
    assert share[0] > 0.5
    for kw in (dict(stride=2), dict(k0=1)):
        with pytest.raises(ValueError, match=r"the maps need every frame of the record \(k0 0, stride 1\)"):
            pca.pca(b, 4, **kw)
    Gs, ss = pca.gram(b, 5, 40, 7)
    assert np.array_equal(Gs, ref.gram(regs[5::7][:40])[0]) and np.array_equal(ss, ref.gram(regs[5::7][:40])[1])
    kf.close()
    kf = cases.make_filter(dm, frames[0])
    with pytest.raises(RuntimeError, match="without keep=True"):
        pca.gram(body.BodyReadout(kf))
    kf.close()


def test_cli_pca_end_to_end(hm, tmp_path, monkeypatch, capsys):
    """--pca 4 --pca-frames writes the arrays with the stated shapes and dtypes, and they are the module's: what pca.pca
    returned inside the run, which is the restatement's result on the record fetched at that moment."""
    from hydra_mi import pca, synth
    sys.path.insert(0, ROOT)
    import run_kalmanfilter
    n, Fv = 96, 14
    video = synth.disk_video(n, Fv, "translate_leftup", 0)[0]
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    monkeypatch.chdir(tmp_path)
    seen = []
    module_pca = pca.pca

    def spy(body, k, **kw):
        out = module_pca(body, k, **kw)
        seen.append((out, body.r.body_rec_fetch(), body.tri_of_pixel >= 0))
        return out

    monkeypatch.setattr(pca, "pca", spy)
    base = [vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std"]
    out = str(tmp_path / "pca.npz")
    assert run_kalmanfilter.main(base + [out] + find + ["--rois", "--pca", "4", "--pca-frames"]) == 0
    assert "PCA: 4 components of %d frames" % (Fv - 1) in capsys.readouterr().out
    z = np.load(out)
    F1 = z["X"].shape[0]
    assert F1 == Fv - 1 and len(seen) == 1
    p, regs, m = seen[0]
    assert z["pca_lambda"].shape == (4,) and z["pca_lambda"].dtype == np.float64
    assert z["pca_share"].shape == (4,) and z["pca_share"].dtype == np.float64
    assert z["pca_temporal"].shape == (F1, 4) and z["pca_temporal"].dtype == np.float64
    assert z["pca_rho"].shape == (4, n, n) and z["pca_rho"].dtype == np.float32
    assert z["pca_frame_score"].shape == (F1,) and z["pca_frame_score"].dtype == np.float64
    assert z["pca_frame_r"].shape == (F1, F1) and z["pca_frame_r"].dtype == np.float32
    assert np.array_equal(_bits(z["pca_lambda"]), _bits(p["lam"])) and np.array_equal(_bits(z["pca_share"]), _bits(p["share"]))
    assert np.array_equal(_bits(z["pca_temporal"]), _bits(p["temporal"]))
    assert z["pca_rho"].tobytes() == p["rho"].astype(np.float32).tobytes()
    assert np.array_equal(_bits(z["pca_frame_score"]), _bits(p["frame_score"]))
    assert z["pca_frame_r"].tobytes() == p["frame_r"].astype(np.float32).tobytes()
    # the module's, from the record as it stood
    Gr, sr = ref.gram(regs)
    lam_r, U_r, share_r = ref.components(Gr, 4)
    assert len(regs) == F1 and np.array_equal(_bits(p["lam"]), _bits(lam_r)) and np.array_equal(_bits(p["temporal"]), _bits(U_r))
    assert np.array_equal(_bits(p["rho"]), _bits(ref.maps(regs, m, U_r)))
    assert np.array_equal(_bits(p["frame_r"]), _bits(ref.frame_similarity(Gr, sr, int(m.sum()))))
    assert np.isnan(z["pca_rho"][:, ~m]).all() and (z["pca_share"] > 0).all() and (np.diff(z["pca_lambda"]) <= 0).all()
    # refused without a kept record, without --pca, and for more components than the centred video has
    for extra, words in ((["--pca", "4"], "--pca reads the kept record: it needs --rois or --demix"),
                         (find + ["--rois", "--pca-frames"], "--pca-frames adds the frame similarity: it needs --pca"),
                         (find + ["--rois", "--pca", "0"], "--pca needs at least one component"),
                         (find + ["--rois", "--pca", str(F1)], r"--pca: %d components of %d frames \(need 1\.\.%d\)" % (F1, F1, F1 - 1))):
        with pytest.raises(SystemExit) as e:
            run_kalmanfilter.main(base + [out] + extra)
        assert e.value.code == 2
        import re
        assert re.search(words, capsys.readouterr().err)
