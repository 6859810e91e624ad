"""The cases of tests/measure_cases.py are what their names say -- triangle and neighbour counts, star region tiles on the
stated side of TMASK_STRIDE, candidates per k_render_iter strip -- so that no GPU test of tests/test_measure_limits_gpu.py
can move off its limit unnoticed.  The host restatement of the star region is held against the oracle's coverage: no
pixel a star covers in any of the five configurations lies outside its region."""
import numpy as np
import pytest

import measure_cases as mc
from oracle import ekf_ref


def _cover(X, N, tri, W, H):
    """how many triangles of `tri` cover each pixel (the oracle's image render of a texture of ones)"""
    ones = np.ones((H, W), np.uint8)
    im, _, _, _ = ekf_ref.render(X, N, tri, np.zeros((N, 2)), ones, W, H)
    return im.astype(np.int64)                    # saturates at 255: enough to tell "many"


def _check_region(c, X, verts):
    m = c["mesh"]
    N, W, H = len(m.p), c["W"], c["H"]
    for v in verts:
        c0, r0, rw, rh = mc.star_region(X, N, m.t, v, W, H)
        assert c0 % 8 == 0 and r0 % 8 == 0 and rw % 8 == 0 and rh % 8 == 0
        inside = np.zeros((H, W), bool)
        inside[r0:r0 + rh, c0:c0 + rw] = True
        tri = m.t[mc.star(m.t, v)]
        for Xc in mc.configurations(X, N, v):
            cov = _cover(Xc, N, tri, W, H)
            assert not np.any((cov > 0) & ~inside), (c["name"], v)


@pytest.mark.parametrize("k", mc.HUB_DEGREES)
def test_hubs(k):
    c = {x["name"]: x for x in mc.hub_cases()}["hub%d" % k]
    t = c["mesh"].t
    assert len(mc.star(t, 0)) == k and len(mc.neighbours(t, 0)) == k
    assert mc.prep_entries(t, 0) == 4 * (k + 1) <= mc.PREP_MAX_ENTRIES
    # some vertex is not a neighbour of the hub (an HTH block that must stay zero)
    assert len(c["mesh"].p) > k + 1
    assert max(len(mc.star(t, v)) for v in range(1, len(c["mesh"].p))) <= 6
    N = len(c["mesh"].p)
    for name, X in c["states"].items():
        _check_region(c, X, [0] + list(mc.neighbours(t, 0)))
    # the folded state turns triangles of the hub's star over
    P = c["states"]["folded"][:2 * N].reshape(N, 2)
    tri = t[mc.star(t, 0)]
    a = lambda Q: (Q[tri[:, 1], 0] - Q[tri[:, 0], 0]) * (Q[tri[:, 2], 1] - Q[tri[:, 0], 1]) - \
        (Q[tri[:, 1], 1] - Q[tri[:, 0], 1]) * (Q[tri[:, 2], 0] - Q[tri[:, 0], 0])
    assert np.any(np.sign(a(P)) != np.sign(a(c["mesh"].p)))


def test_border_fan_fills_the_prep_row():
    c = mc.border_fan_case()
    t = c["mesh"].t
    assert len(mc.star(t, 0)) == mc.EKF_MAX_STAR
    assert len(mc.neighbours(t, 0)) == mc.EKF_MAX_STAR + 1
    assert mc.prep_entries(t, 0) == mc.PREP_MAX_ENTRIES == 104
    assert max(len(mc.neighbours(t, v)) for v in range(1, len(c["mesh"].p))) <= 6
    for X in c["states"].values():
        _check_region(c, X, [0] + list(mc.neighbours(t, 0)))


def test_refused_meshes_break_one_limit_each():
    over, pinch, big = mc.refused_cases()
    assert len(mc.star(over["mesh"].t, 0)) == mc.EKF_MAX_STAR + 1
    assert mc.prep_entries(over["mesh"].t, 0) <= mc.PREP_MAX_ENTRIES            # only the star is over
    assert len(mc.star(pinch["mesh"].t, 0)) == mc.EKF_MAX_STAR                   # the star is not over ...
    assert len(mc.neighbours(pinch["mesh"].t, 0)) == 26                          # ... the neighbours are
    assert mc.prep_entries(pinch["mesh"].t, 0) > mc.PREP_MAX_ENTRIES
    t = big["mesh"].t
    assert len(t) == mc.EKF_MAX_TRI + 1
    assert max(len(mc.star(t, v)) for v in range(len(big["mesh"].p))) <= 6


def test_coarse_regions_sit_on_their_side_of_the_tile_limit():
    cs = {c["name"]: c for c in mc.coarse_cases()}
    at, above = cs["region_at"], cs["region_above"]
    assert above["R"] - at["R"] == 1.0 / mc.SUB                                  # neighbouring radii on the 1/256 grid
    tiles = {}
    for name, c in cs.items():
        m = c["mesh"]
        tiles[name] = mc.region_tiles(c["states"]["rest"], len(m.p), m.t, 0, c["W"], c["H"])
    assert tiles["region_at"] == mc.TMASK_STRIDE
    assert tiles["region_above"] == 1056 > mc.TMASK_STRIDE                        # 32 x 33 tiles
    assert tiles["region_wide"] > 3 * mc.TMASK_STRIDE and cs["region_wide"]["W"] == 4096
    c = cs["region_clipped"]
    assert c["W"] % 8 != 0 and tiles["region_clipped"] > mc.TMASK_STRIDE
    c0, r0, rw, rh = mc.star_region(c["states"]["rest"], len(c["mesh"].p), c["mesh"].t, 0, c["W"], c["H"])
    assert c0 + rw > c["W"]                                                      # the last tile column leaves the frame
    # on the 320 x 320 frame every other vertex keeps a tile list (the wide and clipped wheels' rim vertices do not)
    for name, c in cs.items():
        m = c["mesh"]
        if name in ("region_at", "region_above"):
            for v in range(1, len(m.p)):
                assert mc.region_tiles(c["states"]["rest"], len(m.p), m.t, v, c["W"], c["H"]) <= mc.TMASK_STRIDE, (name, v)
        _check_region(c, c["states"]["rest"], range(len(m.p)))


def test_grid_fills_the_triangle_masks():
    c = mc.grid_case()
    m = c["mesh"]
    N, T = len(m.p), len(m.t)
    assert (mc.GRID_ROWS, mc.GRID_COLS, T) == (33, 65, mc.EKF_MAX_TRI)
    assert np.bincount(m.bars.reshape(-1), minlength=N).max() == 6
    W, H = c["W"], c["H"]
    for name, X in c["states"].items():
        P = ekf_ref.snap(X[:2 * N].reshape(N, 2))
        for tr in m.t:
            assert mc.tri_box(P[tr], W, H)[0] <= mc.tri_box(P[tr], W, H)[1], name          # nothing degenerate
    cand = mc.strip_candidates(c["states"]["shrunk"], N, m.t, W, H)
    assert cand.max() == mc.EKF_MAX_TRI and (cand > 0).sum() == 1                # one strip, 128 chunks
    assert -(-cand.max() // mc.RI_CHUNK) == 128
    cand = mc.strip_candidates(c["states"]["folded"], N, m.t, W, H)
    assert cand.max() > 64 * mc.RI_CHUNK and (cand > 0).sum() == 2
    cov = _cover(c["states"]["folded"], N, m.t, W, H)
    assert cov.max() >= 100                                                      # saturates any texture above 2
    assert mc.strip_candidates(c["states"]["rest"], N, m.t, W, H).max() > mc.RI_CHUNK


@pytest.mark.parametrize("n", mc.STRIP_COUNTS)
def test_ribbon_strips_have_their_candidate_counts(n):
    c = mc.ribbon_case(n)
    m = c["mesh"]
    N, W, H = len(m.p), c["W"], c["H"]
    for name, X in c["states"].items():
        cand = mc.strip_candidates(X, N, m.t, W, H)
        assert cand[1, 0] == n and cand.sum() == n, name
        P = ekf_ref.snap(X[:2 * N].reshape(N, 2))
        for tr in m.t:
            b = mc.tri_box(P[tr], W, H)
            assert b[0] <= b[1], name
    # folded: pixels covered by triangles of different chunks, three or more deep (f32 sums whose order shows)
    X = c["states"]["folded"]
    cov = _cover(X, N, m.t, W, H)
    assert cov.max() >= 3
    if n > mc.RI_CHUNK:
        first = _cover(X, N, m.t[:mc.RI_CHUNK], W, H)
        rest = _cover(X, N, m.t[mc.RI_CHUNK:], W, H)
        assert np.any((first > 0) & (rest > 0) & (cov >= 3))
