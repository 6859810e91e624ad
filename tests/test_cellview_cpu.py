"""The cell view without a GPU: properties of the NumPy restatement (tests/cellview_ref.py) that must hold whatever the
kernel does, and the host-side helpers of hydra_mi.cellview."""
import numpy as np
import pytest

import cellview_ref

W, H = 40, 24


def _square():
    """two triangles over (6, 4) .. (30, 20): whole-pixel corners, so every pixel centre inside maps onto itself"""
    p = np.array([[6.0, 4.0], [30.0, 4.0], [30.0, 20.0], [6.0, 20.0]])
    t = np.array([[0, 1, 2], [0, 2, 3]])
    return p, t


def _labels():
    lab = np.full((H, W), -1, np.int32)
    lab[6:11, 8:14] = 0
    lab[6:11, 14:19] = 1           # shares an edge with cell 0
    lab[15:22, 20:33] = 2          # partly outside the mesh (rows >= 20, columns >= 30)
    return lab


def _frame():
    return np.random.default_rng(0).integers(0, 200, (H, W), dtype=np.uint8)


COL = np.array([[10, 200, 30], [250, 5, 90], [0, 0, 255]], np.uint8)


def _expect_rest(frame, lab, p):
    """colour[label] on the labelled map pixels, the frame elsewhere"""
    want = np.repeat(frame[:, :, None], 3, axis=2)
    inmap = np.zeros((H, W), bool)
    inmap[4:20, 6:30] = True       # pixel centres c + 0.5 in [6, 30), r + 0.5 in [4, 20): the top-left rule at whole corners
    on = inmap & (lab >= 0)
    want[on] = COL[lab[on]]
    return want, on


def test_rest_state_shows_the_labels_in_place():
    p, t = _square()
    frame, lab = _frame(), _labels()
    got = cellview_ref.view_cells(p.reshape(-1), t, p, frame, lab, None, COL, None, outline=False)
    want, on = _expect_rest(frame, lab, p)
    assert on.sum() > 0 and (lab[~on] >= 0).any()          # some labelled pixels lie outside the mesh and stay gray
    assert np.array_equal(got, want)


def test_whole_pixel_translation_moves_the_picture():
    p, t = _square()
    frame, lab = np.full((H, W), 77, np.uint8), _labels()
    rest = cellview_ref.view_cells(p.reshape(-1), t, p, frame, lab, None, COL, None, outline=True)
    moved = cellview_ref.view_cells((p + (3.0, -2.0)).reshape(-1), t, p, frame, lab, None, COL, None, outline=True)
    want = np.full_like(rest, 77)
    want[:-2, 3:] = rest[2:, :-3]
    assert np.array_equal(moved, want)
    assert (rest != 77).any()


def test_a_layer_of_weight_zero_changes_nothing():
    p, t = _square()
    frame, lab = _frame(), _labels()
    X = (p * 1.1 + (0.3, -0.7)).reshape(-1)
    lab2 = np.stack([lab, np.roll(lab, 3, axis=1)])
    w2 = np.stack([np.full((H, W), 65535, np.uint16), np.zeros((H, W), np.uint16)])
    one = cellview_ref.view_cells(X, t, p, frame, lab, None, COL, [255, 128, 1])
    two = cellview_ref.view_cells(X, t, p, frame, lab2, w2, COL, [255, 128, 1])
    assert np.array_equal(one, two)


def test_level_zero_leaves_the_base_and_the_outlines():
    p, t = _square()
    frame, lab = _frame(), _labels()
    got = cellview_ref.view_cells(p.reshape(-1), t, p, frame, lab, None, COL, [0, 0, 0], outline=True)
    want = np.repeat(frame[:, :, None], 3, axis=2)
    _, on = _expect_rest(frame, lab, p)
    edge = on & cellview_ref.outline_plane(lab)
    want[edge] = COL[lab[edge]]
    assert np.array_equal(got, want)
    assert edge[6, 8] and edge[8, 13] and edge[8, 14] and not edge[8, 10]      # the shared edge is outline on both sides
    assert np.array_equal(cellview_ref.view_cells(p.reshape(-1), t, p, frame, lab, None, COL, [0, 0, 0], outline=False),
                          np.repeat(frame[:, :, None], 3, axis=2))


def test_outline_counts_the_frame_border_as_another_label():
    lab = np.zeros((3, 4), np.int32)
    o = cellview_ref.outline_plane(lab)
    assert o[0].all() and o[2].all() and o[1, 0] and o[1, 3] and not o[1, 1] and not o[1, 2]


def test_layers_from_shapes_order_and_dropped(hm):
    from hydra_mi import cellview
    R = 1
    a = np.zeros((3, 3, 3), np.uint16)
    a[0] = [[5, 6, 7], [0, 9, 1], [2, 3, 4]]
    a[1] = 11
    a[2] = 21
    seeds = np.array([[2, 2], [3, 2], [3, 3]])        # (column, row): windows overlap in columns 2..3
    lab, w, dropped = cellview.layers_from_shapes(a, seeds, R, (6, 7), n_layers=2)
    assert lab.shape == (2, 6, 7) and w.dtype == np.uint16 and lab.dtype == np.int32
    # pixel (row 2, column 2): cells 0 (its centre, 9), 1 (11) and 2 (21) -> the first two kept, one dropped
    assert (lab[0, 2, 2], w[0, 2, 2], lab[1, 2, 2], w[1, 2, 2]) == (0, 9, 1, 11)
    # pixel (row 2, column 1): cell 0's window value is 0 there -> not a cell of that pixel
    assert lab[0, 2, 1] == -1 and w[0, 2, 1] == 0
    # pixel (row 1, column 1): cell 0 alone
    assert (lab[0, 1, 1], w[0, 1, 1], lab[1, 1, 1]) == (0, 5, -1)
    # pixel (row 4, column 4): cell 2 alone, in layer 0
    assert (lab[0, 4, 4], w[0, 4, 4], lab[1, 4, 4]) == (2, 21, -1)
    count = np.zeros((6, 7), int)
    for s, (c, r) in enumerate(seeds):
        count[r - 1:r + 2, c - 1:c + 2] += a[s] > 0
    assert dropped == np.maximum(count - 2, 0).sum() and dropped > 0
    lab1, w1, dropped1 = cellview.layers_from_shapes(a, seeds, R, (6, 7), n_layers=1)
    assert np.array_equal(lab1[0], lab[0]) and np.array_equal(w1[0], w[0])
    assert dropped1 == np.maximum(count - 1, 0).sum() and dropped1 > dropped
    # a window cut by the frame
    lab3, _, d3 = cellview.layers_from_shapes(a[:1], np.array([[0, 0]]), R, (6, 7))
    assert d3 == 0 and lab3[0, 0, 0] == 0 and lab3[0, 1, 0] == 0 and (lab3[0] >= 0).sum() == 4      # [[9, 1], [3, 4]] of the window is on the frame
    with pytest.raises(ValueError):
        cellview.layers_from_shapes(a, seeds, R, (6, 7), n_layers=5)
    l1, wl = cellview.layers_from_labels(lab[0])
    assert l1.shape == (1, 6, 7) and (wl == 65535).all()


def test_levels(hm):
    from hydra_mi import cellview
    F = 101
    x = np.zeros((F, 4))
    x[:, 0] = 3.5                                   # constant: 0
    x[:, 1] = np.arange(F)                          # percentiles 10 and 99 of 0..100 are 10 and 99
    x[:, 2] = np.arange(F)
    x[7, 2] = np.nan
    x[:, 3] = np.nan
    lv = cellview.levels(x)
    assert lv.dtype == np.uint8 and lv.shape == (F, 4)
    assert not lv[:, 0].any() and not lv[:, 3].any()
    assert lv[0, 1] == 0 and lv[10, 1] == 0 and lv[99, 1] == 255 and lv[100, 1] == 255         # clipped at both ends
    assert lv[50, 1] == int(np.rint(255.0 * ((50.0 - 10.0) / (99.0 - 10.0))))
    assert lv[7, 2] == 0 and lv[60, 2] > 0
    assert np.array_equal(cellview.palette(30)[12:24], cellview.palette(12)) and len(np.unique(cellview.palette(12), axis=0)) == 12


def test_markers():
    img = np.zeros((10, 12, 3), np.uint8)
    red, green = (0, 0, 255), (0, 255, 0)
    # truncation toward zero: (-0.9, -0.9) is pixel (0, 0), not (-1, -1)
    cellview_ref.markers(img, [[-0.9, -0.9]], [red], 0)
    assert tuple(img[0, 0]) == red and np.count_nonzero(img.any(axis=2)) == 1
    # (-1.5, 3.7) is (-1, 3): with radius 1 only its right neighbour (0, 3) is on the frame
    img[:] = 0
    cellview_ref.markers(img, [[-1.5, 3.7]], [red], 1)
    assert tuple(img[3, 0]) == red and np.count_nonzero(img.any(axis=2)) == 1
    # a disc of radius 2 has 13 pixels; cut by each border
    for (x, y), n in (((5.2, 5.9), 13), ((0.0, 5.0), 9), ((11.9, 5.0), 9), ((5.0, 0.5), 9), ((5.0, 9.0), 9), ((0.0, 0.0), 6)):
        img[:] = 0
        cellview_ref.markers(img, [[x, y]], [green], 2)
        assert np.count_nonzero(img.any(axis=2)) == n, (x, y)
    # a later point over an earlier one; non-finite and far points skipped
    img[:] = 0
    cellview_ref.markers(img, [[5, 5], [6, 5], [np.nan, 2], [3e6, 2], [np.inf, 1]], [red, green, red, red, red], 2)
    assert tuple(img[5, 6]) == green and tuple(img[5, 5]) == green and tuple(img[5, 3]) == red
    assert np.count_nonzero(img.any(axis=2)) == 13 + 5
