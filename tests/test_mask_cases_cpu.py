"""The oracle of the contour pruning (oracle/ekf_ref.pruned_object, reference imgproc.py:198-228) pinned on the masks of
tests/mask_cases.py before the device is held against it (tests/test_mask_pruning_gpu.py): known answers worked out by
Pick's theorem for the hand-countable cases, and the product's host form (imgproc._object_and_holes, written
independently) equal to it on every case at frame sizes with full, partial and single tiles."""
import numpy as np
import pytest
from scipy import ndimage

import mask_cases as mc
from oracle import ekf_ref


def _four(region):
    """pixels 4-adjacent to `region` (not in it), with the frame surrounded by nothing"""
    pad = np.pad(region, 1, constant_values=False)
    return (pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]) & ~region


def _object_a2(obj):
    """doubled contour area of a solid object (no holes) by Pick: 2 (pixels) - (pixels 4-adjacent to the outside or on
    the frame edge) - 2"""
    outside = np.pad(~obj, 1, constant_values=True)
    nb = outside[:-2, 1:-1] | outside[2:, 1:-1] | outside[1:-1, :-2] | outside[1:-1, 2:]
    return 2 * int(obj.sum()) - int((obj & nb).sum()) - 2


def _agree(m):
    from hydra_mi import imgproc
    want = ekf_ref.pruned_object(m)
    assert np.array_equal(imgproc._object_and_holes(m), want)
    return want


def test_seam_cases_known_answers(hm):
    H, W, Y, X = 64, 192, 32, 128
    cases = mc.seam_cases(H, W, Y, X)
    for name in ("diag_corner", "diag_corner_flip", "diag_vseam", "diag_vseam_flip", "bridge_vseam", "bridge_hseam",
                 "serpentine_1_1", "serpentine_2_1", "serpentine_1_2", "serpentine_2_2"):
        m = cases[name]
        assert ndimage.label(m, np.ones((3, 3)))[1] == 1, name             # one 8-connected object ...
        assert np.array_equal(_agree(m), m), name                           # ... kept whole
    for name in ("diag_corner", "diag_corner_flip", "diag_vseam", "diag_vseam_flip"):
        # the halves touch only diagonally: cut the diagonal pair and the smaller half goes
        m = cases[name]
        lab, n = ndimage.label(m)                                          # 4-connected: the two halves
        assert n == 2
        big = np.argmax(np.bincount(lab.ravel())[1:]) + 1
        assert np.array_equal(ekf_ref.pruned_object(lab == big), lab == big)
    # background meets background only diagonally: the pocket stays a hole -- 3 x 4: 2 I + R - 2 = 24 + 14 - 2 = 36 < 80,
    # filled; 6 x 10: 120 + 32 - 2 = 150, kept
    for name, filled in (("bg_diag", True), ("bg_diag_flip", True), ("bg_diag_big", False), ("bg_diag_big_flip", False)):
        m = cases[name]
        holes, nh = ndimage.label(~m & ndimage.binary_fill_holes(m))
        assert nh == 1, name
        assert np.array_equal(_agree(m), m | (holes == 1) if filled else m), name
    # a 1-px corridor across a seam takes the 3 x 5 pocket (area 22: it would be filled as a hole) outside
    for name in ("corridor_v", "corridor_h"):
        m = cases[name]
        assert np.array_equal(ndimage.binary_fill_holes(m), m), name
        assert np.array_equal(_agree(m), m), name
    # combs: open ones are kept as they are; closed ones have only small holes (gaps of 7 x 1..2 px: area <= 22), filled
    for name, m in cases.items():
        if name.startswith("comb_"):
            want = ndimage.binary_fill_holes(m) if "closed" in name else m
            assert ndimage.label(m, np.ones((3, 3)))[1] == 1, name
            assert np.array_equal(_agree(m), want), name
    # checkerboard: one object through diagonals only, every background cell inside a 1-px hole (area 1 + 4/2 - 1 = 2)
    for name in ("checker_0", "checker_1"):
        m = cases[name]
        assert ndimage.label(m)[1] == m.sum() and ndimage.label(m, np.ones((3, 3)))[1] == 1
        assert np.array_equal(_agree(m), ndimage.binary_fill_holes(m)), name
    # hole thresholds: I hole pixels, R object pixels 4-adjacent to the hole, doubled area 2 I + R - 2 against 80
    for name, I, R, kept in (("hole_80", 30, 22, True), ("hole_79", 30, 21, False), ("hole_78", 29, 22, False)):
        m = cases[name]
        hole = ndimage.binary_fill_holes(m) & ~m
        assert int(hole.sum()) == I and int(_four(hole).sum()) == R and 2 * I + R - 2 == int(name[-2:]), name
        assert np.array_equal(_agree(m), m if kept else m | hole), name
    # object thresholds: 6 x 9 = 54 pixels, 26 on its border: 108 - 26 - 2 = 80 (area 40, kept); without a corner
    # 106 - 25 - 2 = 79 (39.5: nothing is kept)
    assert _object_a2(cases["object_80"]) == 80 and _object_a2(cases["object_79"]) == 79
    assert np.array_equal(_agree(cases["object_80"]), cases["object_80"])
    assert not _agree(cases["object_79"]).any()
    # tie: two 6 x 9 objects (area 40 each); the one first in raster order stays though it is the later one in x
    m = cases["tie"]
    lab, n = ndimage.label(m, np.ones((3, 3)))
    assert n == 2 and _object_a2(lab == 1) == _object_a2(lab == 2) == 80
    first = lab == lab.ravel()[np.flatnonzero(m)[0]]
    assert np.argwhere(first)[:, 1].min() > np.argwhere(m & ~first)[:, 1].min()
    assert np.array_equal(_agree(m), first)


@pytest.mark.parametrize("H,W", [(16, 64), (17, 65), (45, 130), (300, 517)])
def test_frame_edge_known_answers(hm, H, W):
    m = mc.frame_edge(H, W, "pockets")
    assert m[:, W - 1].any() and m[H - 1].any()
    assert np.array_equal(_agree(m), m)                                     # both pockets reach the frame edge: outside
    for kind, keep_corner in (("tie_before", False), ("tie_after", True)):
        m = mc.frame_edge(H, W, kind)
        lab, n = ndimage.label(m, np.ones((3, 3)))
        corner = lab == lab[H - 1, W - 1]
        assert n == 2 and _object_a2(corner) == _object_a2(m & ~corner) == 80, kind
        assert np.array_equal(_agree(m), corner if keep_corner else m & ~corner), kind


def test_deep_nesting_known_answers(hm):
    """Forty 1-px outlines 2 px apart: 80 levels of nesting.  The outermost outline's contour encloses 160 x 160 pixel
    centres (doubled area 2 x 159^2 = 50562) and beats the solid 159 x 159 square (2 x 158^2 = 49928); inside a hole of
    a 176 x 176 square (2 x 175^2 = 61250) they make that square beat a solid 173 x 173 one (2 x 172^2 = 59168)."""
    m = mc.deep_rings(200, 360)
    lab, n = ndimage.label(m, np.ones((3, 3)))
    assert n == 41
    outer = lab == lab[20, 10]
    assert _object_a2(ndimage.binary_fill_holes(outer)) == 50562 and _object_a2(lab == lab[25, 190]) == 49928
    assert np.array_equal(_agree(m), outer)                                 # the outline; what it encloses is a kept hole
    m = mc.deep_in_hole(184, 366)
    lab, n = ndimage.label(m, np.ones((3, 3)))
    assert n == 42
    a = lab == lab[4, 4]
    assert _object_a2(ndimage.binary_fill_holes(a)) == 61250 and _object_a2(lab == lab[6, 188]) == 59168
    assert np.array_equal(_agree(m), a)


@pytest.mark.parametrize("H,W", [(16, 64), (17, 65), (96, 96), (45, 130)])
def test_seam_cases_follow_host_form(hm, H, W):
    """every case at every anchor (tile corners and the frame centre, shifted off the grid)"""
    n = 0
    for Y, X in mc.anchors(H, W):
        for name, m in mc.seam_cases(H, W, Y, X).items():
            _agree(m)
            n += 1
    assert n > 0
    for kind in ("pockets", "tie_before", "tie_after"):
        m = mc.frame_edge(H, W, kind)
        if m is not None:
            _agree(m)
