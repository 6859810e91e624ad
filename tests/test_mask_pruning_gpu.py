"""The contour pruning on the device (hm_prune_mask: k_ccl_* in csrc/project_kernels.h) and the projection built on it
(hm_project_mask) against the oracle (oracle/ekf_ref.pruned_object, project_mask) at frame scale: a single tile, one
pixel into a second tile each way, partial last tiles in both directions, 512^2 and 1024^2.  The masks
(tests/mask_cases.py) put diagonals, bridges, corridors, chains of unions and thresholds on the 64 x 16 tile seams of
the labelling, at several offsets against the tile grid; tests/test_mask_cases_cpu.py pins the oracle on them first."""
import numpy as np
import pytest

import mask_cases as mc
from oracle import ekf_ref

pytestmark = pytest.mark.gpu

SIZES = [(96, 96), (16, 64), (17, 65), (300, 517), (512, 512), (1024, 1024)]


@pytest.fixture(scope="module")
def renderers(hm):
    """(H, W) -> (renderer, mesh), one per frame size: a small box mesh in the middle of the frame"""
    from hydra_mi import mesh, renderer
    made = {}

    def get(H, W):
        if (H, W) not in made:
            dm = mesh.box_mesh(0.25 * W, 0.25 * H, 0.75 * W, 0.75 * H, max(3.0, min(H, W) / 8.0))
            tex = np.random.default_rng(H * W).integers(0, 256, (H, W), dtype=np.uint8)
            R = renderer.Renderer(dm, np.zeros((dm.size(), 2)), np.zeros((H, W, 2), np.float32), H, tex, True,
                                  1e-3, 1.0, 1.0)
            assert (R.ny, R.nx) == (H, W)
            made[(H, W)] = (R, dm)
        return made[(H, W)]
    yield get
    for R, _ in made.values():
        R.close()


def _local_oracle(m):
    """ekf_ref.pruned_object(m) computed on the bounding box of the object pixels grown by one pixel (clipped to the
    frame): everything outside that box is background that reaches the frame edge in both, so the result is the same
    -- and cheap for a small structure in a large frame"""
    out = np.zeros(m.shape, bool)
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return out
    y0, y1 = max(0, ys.min() - 1), min(m.shape[0], ys.max() + 2)
    x0, x1 = max(0, xs.min() - 1), min(m.shape[1], xs.max() + 2)
    out[y0:y1, x0:x1] = ekf_ref.pruned_object(m[y0:y1, x0:x1])
    return out


def _mismatches(R, masks, oracle=ekf_ref.pruned_object):
    """[(label, pixels that differ)] of the masks on which the device's pruning is not the oracle's, bit for bit"""
    bad = []
    for label, m in masks:
        got = R.prune_mask(m.astype(np.uint8)).astype(bool)
        want = oracle(m)
        if not np.array_equal(got, want):
            bad.append((label, int((got != want).sum())))
    return bad


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_prune_seam_cases_match_oracle(renderers, H, W):
    R, _ = renderers(H, W)
    masks = [((Y, X, name), m) for Y, X in mc.anchors(H, W) for name, m in mc.seam_cases(H, W, Y, X).items()]
    masks += [(kind, m) for kind in ("pockets", "tie_before", "tie_after")
              for m in [mc.frame_edge(H, W, kind)] if m is not None]
    assert len(masks) >= 40
    bad = _mismatches(R, masks, _local_oracle)
    assert not bad, bad[:20]
    bad = _mismatches(R, [("zeros", np.zeros((H, W), bool)), ("ones", np.ones((H, W), bool))])
    assert not bad, bad


@pytest.mark.parametrize("H,W,k", [(16, 64, 12), (17, 65, 12), (300, 517, 8), (1024, 1024, 3)])
def test_prune_blobs_match_oracle(renderers, H, W, k):
    """seeded random masks: few blobs and a few dozen specks, so that the oracle stays fast"""
    R, _ = renderers(H, W)
    rng = np.random.default_rng(H + W)
    masks = [(t, mc.blobs(rng, H, W, int(rng.integers(1, 4)), specks=min(0.01, 40.0 / (H * W)))) for t in range(k)]
    bad = _mismatches(R, masks)
    assert not bad, bad


@pytest.mark.parametrize("H,W", [(300, 517), (512, 512), (1024, 1024)], ids=["300x517", "512x512", "1024x1024"])
def test_prune_keeps_the_deeply_nested_object(renderers, H, W):
    """40 concentric outlines (80 levels of nesting) against a solid square of slightly smaller contour area, and the
    same outlines inside a kept hole of the larger object: the pixels deepest down count for the area of every contour
    around them, however many there are (mask_cases.deep_rings, deep_in_hole)"""
    R, _ = renderers(H, W)
    bad, n = [], 0
    for Y, X in ((0, 0), (H - 200, W - 366), (101, 7)):
        for name, a in (("deep_rings", (Y + 20, X + 10)), ("deep_in_hole", (Y + 4, X + 4))):
            m = getattr(mc, name)(H, W, Y, X)
            if m is None:
                continue
            n += 1
            got = R.prune_mask(m.astype(np.uint8)).astype(bool)
            want = _local_oracle(m)
            assert want[a], (name, Y, X)                            # the oracle keeps A (whose first pixel is a)
            if not np.array_equal(got, want):
                first = np.argwhere(got)[:1].tolist()
                bad.append((name, Y, X, "kept: first pixel %s, A's is %s" % (first, list(a)), int((got != want).sum())))
    assert n >= 4
    assert not bad, bad


# ---- the projection onto the pruned mask at frame scale -----------------------------------------------------------
def _disk_masks(n):
    """the bench's disk mask (synth.disk_video, as bench.py makes it) and a variant with a kept hole (30 x 40) and a
    filled one (5 x 5)"""
    from hydra_mi import synth
    video, masks, centre, radius = synth.disk_video(n, 2, "translate_leftup", 0)
    disk = masks[1].astype(bool)
    holed = disk.copy()
    cy, cx = int(centre[1]), int(centre[0])
    holed[cy - 15:cy + 15, cx - 20:cx + 20] = False
    holed[cy + 60:cy + 65, cx - 80:cx - 75] = False
    return video[1], {"disk": disk, "holed": holed}


def _check_projection(R, dm, m, seed, label):
    N = dm.size()
    H, W = m.shape
    rng = np.random.default_rng(seed)
    for trial, spread in enumerate((0.5, 4.0, 15.0, 60.0)):
        X = np.concatenate((dm.p.reshape(-1) + rng.normal(0, spread, 2 * N), rng.normal(0, 1.0, 2 * N)))
        if trial == 3:
            X[0:2] = (-7.3, 5.1)                                    # off the frame
            X[2:4] = (W + 11.0, H + 2.5)
            X[4:6] = (17.0, 33.0)                                   # on a pixel centre
        want = ekf_ref.project_mask(X, N, m)[:, 0]
        got, moved = R.project_mask(X, m.astype(np.uint8))
        assert got.shape == X.shape
        inside_before = int((np.abs(want - X)[:2 * N].reshape(-1, 2).max(axis=1) > 0).sum())
        assert moved >= inside_before, (label, trial)               # moved counts d > 1, some of which may step by 0
        assert np.array_equal(got, want), (label, trial, np.abs(got - want).max())


def test_project_mask_at_1024_matches_oracle(renderers):
    n = 1024
    R, dm = renderers(n, n)
    frame, masks = _disk_masks(n)
    for kind, m in masks.items():
        _check_projection(R, dm, m, 7, kind)
    # the observation's mask, resident on the device
    N = dm.size()
    X = np.concatenate((dm.p.reshape(-1) + np.random.default_rng(8).normal(0, 30.0, 2 * N), np.zeros(2 * N)))
    R.update_frame(frame, np.zeros((n, n, 2), np.float32), masks["holed"].astype(np.uint8))
    got, moved = R.project_mask(X)
    want = ekf_ref.project_mask(X, N, masks["holed"])[:, 0]
    assert moved > 0 and np.array_equal(got, want)


def test_project_mask_on_seam_case_matches_oracle(renderers):
    H, W = 300, 517
    R, dm = renderers(H, W)
    m = mc.bg_diag_corner(H, W, 160, 256, big=True)
    assert m is not None
    _check_projection(R, dm, m, 9, "bg_diag_big")


def test_filter_projectmask_at_300x517(hm):
    from hydra_mi import kalman, mesh
    H, W = 300, 517
    dm = mesh.box_mesh(0.25 * W, 0.25 * H, 0.75 * W, 0.75 * H, 37.5)
    tex = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    kf = kalman.KalmanFilter(dm, tex, np.zeros((H, W, 2), np.float32), True)
    N = dm.size()
    m = mc.hole_threshold(H, W, 144, 192, 80)
    m[100:200, 300:420] = True                                      # the larger object: the hole's object goes
    kf.state.X[:2 * N, 0] += np.random.default_rng(6).normal(0, 4.0, 2 * N)
    X0 = kf.state.X.copy()
    kf.projectmask(m.astype(np.uint8))
    want = ekf_ref.project_mask(X0, N, m)
    assert kf.state.X.shape == X0.shape and np.array_equal(kf.state.X, want)
    assert not np.array_equal(kf.state.X, X0)
