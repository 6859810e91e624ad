"""The restatement of the views (tests/view_ref.py) against exact arithmetic, and the scenes and states of
tests/view_cases.py held to the limits they are named for.  No GPU: what tests/test_view_limits_gpu.py compares the
kernels with is checked here on its own."""
from fractions import Fraction
import math

import numpy as np
import pytest

import view_cases
import view_ref


# ---- view_ref.segment ------------------------------------------------------------------------------------------------
def _exact_pixels(x0, y0, x1, y1):
    """pixel i = 0..n of the header's rule in exact rationals: x0 + floor(i dx / n + 1/2)"""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)]
    half = Fraction(1, 2)
    return [(x0 + math.floor(Fraction(i * dx, n) + half), y0 + math.floor(Fraction(i * dy, n) + half)) for i in range(n + 1)]


def test_segment_equals_exact_rationals_on_a_small_frame():
    W, H, pad = 5, 4, 8
    r = range(-6, 7)
    for x0 in r:
        for y0 in r:
            for x1 in r:
                for y1 in r:
                    px = _exact_pixels(x0, y0, x1, y1)
                    want = [y * W + x for x, y in px if 0 <= x < W and 0 <= y < H]
                    got = view_ref.segment(x0, y0, x1, y1, W, H)
                    assert got.tolist() == want, (x0, y0, x1, y1)
                    if (x0 + y0) % 3:                          # a third of them: the unclipped properties
                        continue
                    Wp = W + 2 * pad
                    full = view_ref.segment(x0 + pad, y0 + pad, x1 + pad, y1 + pad, Wp, H + 2 * pad)
                    n = max(abs(x1 - x0), abs(y1 - y0))
                    assert len(full) == n + 1
                    assert full[0] == (y0 + pad) * Wp + x0 + pad and full[-1] == (y1 + pad) * Wp + x1 + pad
                    xs, ys = full % Wp, full // Wp
                    assert (np.maximum(np.abs(np.diff(xs)), np.abs(np.diff(ys))) == 1).all()      # 8-neighbours, no repeats


BIG = 1 << 20


@pytest.mark.parametrize("seg", [(-BIG, -BIG, BIG, BIG), (-BIG, -BIG + 7, BIG, BIG - 3), (BIG, -BIG, -BIG, BIG - 1),
                                 (-BIG + 1, 5, BIG, -2), (2, -BIG, 1, BIG), (BIG, 3, -BIG, 0), (-BIG, BIG, 3, 1)])
def test_segment_at_the_widest_the_kernel_accepts(seg):
    """|d| ~ 2^21: the in-frame pixels against exact rationals (only the i that can land on the frame are formed)"""
    W, H = 5, 4
    x0, y0, x1, y1 = seg
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    half = Fraction(1, 2)
    want = []
    if abs(dx) == n:                                           # x-major: x = x0 + sign(dx) i exactly
        cand = sorted((x - x0) * (1 if dx > 0 else -1) for x in range(W))
    else:
        cand = sorted((y - y0) * (1 if dy > 0 else -1) for y in range(H))
    for i in cand:
        if 0 <= i <= n:
            x, y = x0 + math.floor(Fraction(i * dx, n) + half), y0 + math.floor(Fraction(i * dy, n) + half)
            if 0 <= x < W and 0 <= y < H:
                want.append(y * W + x)
    got = view_ref.segment(x0, y0, x1, y1, W, H)
    assert got.tolist() == want
    if seg in ((-BIG, -BIG, BIG, BIG), (-BIG + 1, 5, BIG, -2), (2, -BIG, 1, BIG)):
        assert len(want) > 0                                   # (some of them do cross the frame)


# ---- view_ref.norm_plane ---------------------------------------------------------------------------------------------
def test_norm_plane_non_finite_rule():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    p = np.array([[1.0, nan, 3.0], [inf, 2.0, -inf]], np.float32)
    assert view_ref.norm_plane(p).tolist() == [[0, 0, 255], [0, 127, 0]]
    assert not view_ref.norm_plane(np.full((3, 2), nan, np.float32)).any()
    assert not view_ref.norm_plane(np.array([inf, -inf, nan], np.float32)).any()
    assert not view_ref.norm_plane(np.full((2, 2), 7.25, np.float32)).any()
    assert not view_ref.norm_plane(np.array([-0.0, 0.0, 0.0, -0.0], np.float32)).any()
    assert not view_ref.norm_plane(np.array([inf, 5.0, 5.0, nan], np.float32)).any()             # one finite value: max == min
    # the extremes of binary32: nothing overflows in binary64
    big = np.finfo(np.float32).max
    assert view_ref.norm_plane(np.array([-big, 0.0, big, inf], np.float32)).tolist() == [0, 127, 255, 0]
    # an ulp apart: only 0 and 255
    a = np.float32(0.75)
    assert view_ref.norm_plane(np.array([a, np.nextafter(a, np.float32(1)), a], np.float32)).tolist() == [0, 255, 0]
    assert view_ref.norm_plane(p).dtype == np.uint8 and view_ref.norm_plane(p).shape == p.shape


def test_norm_plane_equals_exact_rationals():
    rng = np.random.default_rng(5)
    p = np.concatenate((rng.normal(0, 3, 40), [0.1, -0.1, 1e-3, 2.5, -7.0, 1e6 + 0.5, -1e6])).astype(np.float32).reshape(-1)
    for plane in (p[:40], p, p[40:], np.array([0.0, 1.0, 2.0, 3.0, 255.0], np.float32), np.arange(256, dtype=np.float32)):
        ex = [Fraction(float(v)) for v in plane]
        lo, hi = min(ex), max(ex)
        want = [math.floor(255 * (v - lo) / (hi - lo)) for v in ex]
        # the values are chosen so that the binary64 quotient has the floor of the exact one (no exact quotient is so
        # close below a whole number that rounding lifts it over): hold that, then the restatement to the exact floors
        flo, fhi = np.float64(float(lo)), np.float64(float(hi))
        f64 = [math.floor(255.0 * (np.float64(v) - flo) / (fhi - flo)) for v in plane]
        assert f64 == want
        assert view_ref.norm_plane(plane).tolist() == want
        assert want[int(np.argmin(plane))] == 0 and want[int(np.argmax(plane))] == 255


def test_ids_view_channels():
    ids = np.array([[0, 255, 256], [65535, 65534, 0x1234]], np.int64)
    wire = np.array([[0, 1, 2], [0, 0, 3]], np.int64)
    m = np.array([[0, 255, 255], [255, 255, 0]], np.uint8)
    v = view_ref.ids_view(ids, wire, m)
    assert v[:, :, 1].tolist() == [[0, 0, 1], [255, 255, 0x12]]
    assert v[:, :, 0].tolist() == [[0, 255, 255], [255, 254, 255]]
    assert v[:, :, 2].tolist() == [[0, 255, 255], [255, 255, 0]]
    assert np.array_equal(view_ref.view("mask", (m, None, None, m), np.zeros((0, 3), np.int64), np.zeros(0), ids=ids)[:, :, 1],
                          v[:, :, 1])


def test_the_two_wheels_agree_within_a_level():
    g = np.linspace(-40, 40, 81, dtype=np.float32)
    gx, gy = np.meshgrid(g, g)
    a, b = view_ref.wheel(gx, gy).astype(int), view_ref.wheel64(gx, gy).astype(int)
    assert np.abs(a - b).max() <= 1
    assert np.count_nonzero(a != b) <= a.size // 100
    assert not view_ref.wheel64(np.float32([0.0, np.nan, 1e9]), np.float32([0.0, 1.0, 0.0])).any()


# ---- view_cases -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(hm):
    return {n: view_cases.scene(n) for n in view_cases.SCENES}


@pytest.mark.parametrize("name", view_cases.SCENES)
def test_every_state_has_its_property(scenes, name):
    sc = scenes[name]
    N = sc["mesh"].size()
    inside = view_cases.state(sc, "inside")
    for st in view_cases.STATES:
        X = view_cases.state(sc, st)
        assert X.shape == (4 * N,) and X.dtype == np.float64
        view_cases.check_state(sc, st, X)
        if st in view_cases.VELOCITY_STATES and st != "velulp":
            assert np.array_equal(X[:2 * N], inside[:2 * N])                  # velocity variants of `inside`
    for pal in ("mixed", "high"):
        lab = view_cases.palette(sc, pal)
        assert lab.shape == (sc["mesh"].t.shape[0],) and lab.min() >= -1 and lab.max() <= 65534
    assert view_cases.palette(sc, "mixed")[:5].tolist() == [-1, 0, 255, 256, 65534]
    assert view_cases.palette(sc, None) is None


@pytest.mark.parametrize("name", view_cases.SCENES)
def test_straddle_really_drops_pixels(scenes, name):
    sc = scenes[name]
    X = view_cases.state(sc, "straddle")
    segs = view_cases.segments(sc, X)
    assert all(s is not None for s in segs)
    pad = max(max(abs(v) for v in s) for s in segs) + 2
    total, kept, window = view_cases.unclipped_count(sc, X, pad)
    assert total == sum(max(abs(s[2] - s[0]), abs(s[3] - s[1])) + 1 for s in segs)      # nothing clipped on the padded frame
    assert 0 < kept < total
    N = sc["mesh"].size()
    assert np.array_equal(window, view_ref.wire_count(sc["mesh"].t, X[:2 * N], sc["W"], sc["H"]))
    # and the control loses nothing
    Xi = view_cases.state(sc, "inside")
    total, kept, _ = view_cases.unclipped_count(sc, Xi, 4)
    assert total == kept
