"""hydra_mi.pca on the host (`pytest -m "not gpu"`): centre, frame_similarity and frame_score equal to the restatement in
loops and Python integers (tests/pca_ref.py) bit for bit, the properties of components, and the planted video with
ensembles, whose first component is the neuropil and whose next three span the ensembles nobody named."""
import numpy as np
import pytest

import pca_ref as ref
from hydra_mi import pca

#: halfway between the highest R^2 at K = 3 (0.5520, seed 2) and the lowest at K = 4 (0.9903, seed 4) of the planted video,
#: seeds 0..4 (pca_ref.planted_figures; the table is in DESIGN.md section 22 and test_planted_video_* measures it again)
R2_MID = 0.771
#: halfway between the lowest |r| of component 1 with the planted neuropil (0.9994, seed 4) and the highest of components
#: 2..4 (0.0313, seed 4)
NPIL_MID = 0.515


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _frames(seed, F=9, n=37):
    """F small random frames with 0 and 255 among them, a constant frame (3), a black one (4), a white one (5) and a
    duplicate (frame 7 is frame 1)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (F, n), dtype=np.uint8)
    v[rng.random((F, n)) < 0.1] = 0
    v[rng.random((F, n)) < 0.1] = 255
    v[3], v[4], v[5], v[7] = 77, 0, 255, v[1]
    return v


@pytest.fixture(scope="module")
def planted():
    return [ref.planted_figures(seed) for seed in range(5)]


def test_gram_restatements_agree():
    v = _frames(0)
    G, s1 = ref.gram(v)
    G2, s2 = ref.gram_loops(v)
    assert G.dtype == np.int64 and np.array_equal(G, G2) and np.array_equal(s1, s2)
    assert G[4].sum() == 0 and G[5, 5] == 65025 * v.shape[1] and np.array_equal(G[7], G[1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_centre_similarity_and_score_equal_the_restatement(seed):
    v = _frames(seed)
    G, s1 = ref.gram(v)
    Gc = pca.centre(G)
    assert Gc.dtype == np.float64 and np.array_equal(_bits(Gc), _bits(ref.centre(G)))
    assert np.abs(Gc.sum(0)).max() <= 1e-9 * np.abs(Gc).max()                   # centred: rows sum to 0 up to rounding
    r = pca.frame_similarity(G, s1, v.shape[1])
    want = ref.frame_similarity(G, s1, v.shape[1])
    assert np.array_equal(_bits(r), _bits(want))
    for k in (3, 4, 5):                                                        # the constant frames: NaN in row and column
        assert np.isnan(r[k]).all() and np.isnan(r[:, k]).all()
    live = [k for k in range(len(v)) if k not in (3, 4, 5)]
    assert not np.isnan(r[np.ix_(live, live)]).any() and r[1, 7] == 1.0 and r[1, 1] == 1.0
    X = v[live].astype(np.float64)
    assert np.allclose(r[np.ix_(live, live)], np.corrcoef(X), rtol=0, atol=1e-12)
    sc = pca.frame_score(r)
    assert np.array_equal(_bits(sc), _bits(ref.frame_score(r)))
    assert np.isnan(sc[[3, 4, 5]]).all() and not np.isnan(sc[live]).any()
    # an even and an odd number of values, a row with one value, a row with none
    rr = np.array([[1.0, 0.2, np.nan, 0.6], [0.2, 1.0, 0.4, 0.8], [np.nan, np.nan, np.nan, 0.5], [np.nan, np.nan, np.nan, 1.0]])
    got = pca.frame_score(rr)
    assert np.array_equal(_bits(got), _bits(ref.frame_score(rr)))
    assert got[0] == (0.2 + 0.6) / 2.0 and got[1] == 0.4 and got[2] == 0.5 and np.isnan(got[3])


def test_centre_refusal_names_its_numbers():
    F = 4
    G = np.full((F, F), 1 << 57, np.int64)                                     # 4 x 4^2 x 2^57 = 2^63
    with pytest.raises(ValueError, match=r"4 F\^2 max G_ii = 4 x 4\^2 x %d could pass 2\^63" % (1 << 57)):
        pca.centre(G)
    G = np.full((F, F), (1 << 57) - 1, np.int64)                               # just below: exact
    assert np.array_equal(_bits(pca.centre(G)), _bits(ref.centre(G)))
    with pytest.raises(ValueError, match="need whole numbers, frames x frames"):
        pca.centre(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="need whole numbers, frames x frames"):
        pca.centre(np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError, match=r"65025 x 12000000\^2 could pass 2\^63"):
        pca.frame_similarity(np.zeros((2, 2), np.int64), np.zeros(2, np.uint64), 12000000)


def test_components_properties():
    rng = np.random.default_rng(11)
    F, n = 24, 500
    v = rng.integers(0, 256, (F, n), dtype=np.uint8)
    v[:, :50] = (128 + 100 * np.sin(np.arange(F) / 3.0))[:, None].astype(np.uint8)        # a strong common mode
    G, _ = ref.gram(v)
    Gc = pca.centre(G)
    k = F - 1
    lam, U, share = pca.components(G, k)
    lam_r, U_r, share_r = ref.components(G, k)
    assert np.array_equal(_bits(lam), _bits(lam_r)) and np.array_equal(_bits(U), _bits(U_r)) and np.array_equal(_bits(share), _bits(share_r))
    assert lam.shape == (k,) and U.shape == (F, k) and share.shape == (k,)
    assert (np.diff(lam) <= 0).all() and (lam >= 0).all()
    eps = np.finfo(np.float64).eps
    assert np.abs(U.T @ U - np.eye(k)).max() <= 64 * F * eps
    assert np.abs(Gc @ U - U * lam[None, :]).max() <= 64 * F * eps * lam[0]
    assert np.allclose(share.sum(), 1.0, rtol=0, atol=1e-12) and share[0] > 2.0 * share[1]      # (the common mode)
    # the squared singular values of the centred video: within F eps lam_1, a symmetric eigensolver's backward error
    X = v.astype(np.float64)
    sv = np.linalg.svd(X - X.mean(0, keepdims=True), compute_uv=False)
    err = np.abs(sv[:k] ** 2 - lam).max()
    print("components against the SVD: largest difference %.3g, F eps lam_1 = %.3g" % (err, F * eps * lam[0]))
    assert err <= F * eps * lam[0]
    # the sign rule: the entry of largest magnitude is positive
    for c in range(k):
        assert U[np.argmax(np.abs(U[:, c])), c] > 0.0
    assert np.array_equal(_bits(pca.components(G, 3)[1]), _bits(U[:, :3]))
    for bad in (0, F):
        with pytest.raises(ValueError, match=r"%d components of %d frames \(need 1\.\.%d\)" % (bad, F, F - 1)):
            pca.components(G, bad)
    with pytest.raises(ValueError, match=r"1 frames \(need at least 2\)"):
        pca.components(G[:1, :1], 1)


def test_components_sign_rule_on_ties():
    """Two frames: the centred Gram matrix is a [[1, -1], [-1, 1]], its vector (1, -1) / sqrt 2 up to sign, a tie in
    magnitude: the first entry is the positive one.  Four frames in two equal pairs likewise."""
    v = np.array([[10, 20, 30, 40], [40, 10, 20, 30]], np.uint8)
    G, _ = ref.gram(v)
    lam, U, share = pca.components(G, 1)
    assert abs(U[0, 0]) == abs(U[1, 0]) and U[0, 0] > 0.0 > U[1, 0] and share[0] == 1.0
    assert np.array_equal(_bits(U), _bits(ref.components(G, 1)[1]))
    v4 = np.concatenate((v, v))
    G4, _ = ref.gram(v4)
    U4 = pca.components(G4, 1)[1]
    first = int(np.argmax(np.abs(U4[:, 0])))
    assert U4[first, 0] > 0.0 and (np.abs(U4[:first, 0]) < abs(U4[first, 0])).all()
    assert np.array_equal(_bits(U4), _bits(ref.components(G4, 1)[1]))


def test_planted_video_components_span_the_ensembles(planted):
    for seed, f in enumerate(planted):
        print("seed %d: shares %s, lowest R^2 K = 3: %.4f, K = 4: %.4f" % (seed, " ".join("%.4f" % s for s in f["share"]),
                                                                        f["r2"][3], f["r2"][4]))
    for f in planted:
        assert f["r2"][3] < R2_MID < f["r2"][4]
        assert f["share"][0] > 0.5 and f["share"][3] > 2.0 * f["share"][4]


def test_planted_video_first_component_is_the_neuropil(planted):
    for seed, f in enumerate(planted):
        print("seed %d: |r| of components 1..4 with the neuropil %s" % (seed, " ".join("%.4f" % s for s in f["npil"])))
    for f in planted:
        assert f["npil"][0] > NPIL_MID > f["npil"][1:].max()
