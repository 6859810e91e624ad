"""The residual video of the demixed model on the CPU: the rule of hm_body_rec_residual_* (tests/residual_ref.py) against
brute force in Python integers, the recovery of the hidden partners of the paired planted video over the restatements
(roi_ref, demix_ref, bodystats_ref), and the argument checks of hydra_mi.residual.  No GPU."""
import numpy as np
import pytest

import demix_ref
import residual_ref as ref
import roi_ref

T16 = 1 << 16


def _brute(regs, inmap, labels, weights, traces, blank, offset):
    """Python integers, pixel by pixel.  m = floor((acc + 2^23) / 2^24): the shift floors, so half a grey level goes up
    on both sides of zero (-0.5 -> 0, +0.5 -> 1)."""
    F, H, W = regs.shape
    out = np.zeros((F, H, W), np.uint8)
    clipped = 0
    for k in range(F):
        for y in range(H):
            for x in range(W):
                if not inmap[y, x] or (blank is not None and blank[y, x]):
                    continue
                acc = 0
                for j in range(labels.shape[0]):
                    s = int(labels[j, y, x])
                    if s >= 0:
                        acc += (65535 if weights is None else int(weights[j, y, x])) * int(traces[k, s])
                r = offset + int(regs[k, y, x]) - (acc + 2 ** 23) // 2 ** 24
                clipped += r < 0 or r > 255
                out[k, y, x] = min(255, max(0, r))
    return out, clipped


def _case():
    """An 8 x 8 map, 5 frames, 3 cells, 2 layers; (row, column) below."""
    rng = np.random.default_rng(1)
    regs = rng.integers(60, 180, (5, 8, 8)).astype(np.uint8)
    m = np.ones((8, 8), bool)
    m[0, 0] = False                                                   # a pixel off the map (it carries cell 0 and a value)
    lab = np.full((2, 8, 8), -1, np.int32)
    wt = np.zeros((2, 8, 8), np.uint16)
    lab[0, 0:5, 0:5], wt[0, 0:5, 0:5] = 0, rng.integers(1, 65536, (5, 5))
    lab[1, 3:6, 3:6], wt[1, 3:6, 3:6] = 1, rng.integers(1, 65536, (3, 3))  # (3, 3) .. (4, 4) carry two cells
    lab[0, 5, 3:6], wt[0, 5, 3:6] = 1, 65535                          # (cell 1 alone, in layer 0 there)
    lab[1, 5, 3:6] = -1
    for x, w in ((1, 128), (2, 1), (4, 256), (5, 256)):               # cell 2: single pixels of row 6 with chosen weights
        lab[0, 6, x], wt[0, 6, x] = 2, w
    tr = np.zeros((5, 3), np.int32)
    tr[:, 0] = rng.integers(-40 * 256, 40 * 256, 5)                   # both signs, up to +-40 grey levels at full weight
    tr[:, 1] = rng.integers(-40 * 256, 40 * 256, 5)
    tr[0, 0], tr[1, 1] = -30 * 256, -20 * 256                         # (a negative trace, whatever the draw)
    tr[:, 2] = (T16, -T16, -(1 << 23) - 1, 65 * T16, 0)
    regs[3, 6, 4], regs[3, 6, 5] = 0, 1                               # frame 3: m = 65 at weight 256 -> r = -1 and 0
    regs[:, 7, 0], regs[:, 7, 1] = 191, 192                           # no cell: r = 255 and 256
    blank = np.zeros((8, 8), np.uint8)
    blank[7, 2] = 1
    regs[:, 7, 2] = 250                                               # (blanked: 314 is not counted as clipped)
    return regs, m, lab, wt, tr, blank


def test_the_rule_against_brute_force():
    regs, m, lab, wt, tr, blank = _case()
    got, clipped = ref.planes(regs, m, lab, wt, tr, blank, 64)
    want, wclip = _brute(regs, m, lab, wt, tr, blank, 64)
    assert np.array_equal(got, want) and clipped == wclip
    # the rounding tie: acc = 128 x 2^16 = +2^23 -> m = 1; acc = -2^23 -> m = 0; acc = -2^23 - 1 -> m = -1
    assert got[0, 6, 1] == 64 + int(regs[0, 6, 1]) - 1
    assert got[1, 6, 1] == 64 + int(regs[1, 6, 1])
    assert got[2, 6, 2] == 64 + int(regs[2, 6, 2]) + 1
    # r = -1, 0, 255, 256
    assert got[3, 6, 4] == 0 and got[3, 6, 5] == 0 and (got[:, 7, 0] == 255).all() and (got[:, 7, 1] == 255).all()
    only = np.zeros((8, 8), bool)
    only[6, 4] = only[6, 5] = only[7, 0] = only[7, 1] = True
    assert _brute(regs[3:4], m & only, lab, wt, tr[3:4], None, 64)[1] == 2          # r = -1 and r = 256 alone are counted
    assert not got[:, 7, 2].any() and not got[:, 0, 0].any()                    # blanked, off the map
    assert ref.planes(regs, m, lab, wt, tr, None, 64)[1] == clipped + 5         # (the blanked pixel would have clipped)
    two = (lab[0] >= 0) & (lab[1] >= 0) & m
    assert two.sum() == 4 and (tr < 0).any() and (tr > 0).any()
    # weights None: 65535 everywhere; one layer; all labels -1
    for w, l in ((None, lab), (wt[:1], lab[:1]), (None, np.full((1, 8, 8), -1, np.int32))):
        a, b = ref.planes(regs, m, l, w, tr, blank, 0), _brute(regs, m, l, w, tr, blank, 0)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    none = ref.planes(regs, m, np.full((1, 8, 8), -1, np.int32), None, tr, None, 200)[0]
    assert np.array_equal(none, np.where(m, np.minimum(255, regs.astype(np.int64) + 200), 0))
    # the largest magnitudes: four layers of weight 65535 and traces at the ends of int32 stay exact in int64
    big_l = np.zeros((4, 8, 8), np.int32)
    big_t = np.array([[-2 ** 31], [2 ** 31 - 1], [0], [1], [-1]], np.int32)
    a, b = ref.planes(regs, m, big_l, None, big_t, None, 64), _brute(regs, m, big_l, None, big_t, None, 64)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and (a[0][0][m] == 255).all() and not a[0][1].any()


RUNS = [(seed, sep) for sep in (6, 5) for seed in range(6)]


@pytest.mark.parametrize("seed,sep", RUNS)
def test_recovery_of_the_hidden_partners(seed, sep):
    """paired_video(seed, sep): the first pass (corr, radius 6, scores >= 0.8) finds the six pair leaders; find_more
    (blank 2, offset 64) ends with the twelve cells, by a round that accepts none, and their demixed traces are as good as
    those of the planted seeds (DESIGN.md section 15 has the table)."""
    v, cs, act, s0, sc0, o = ref.paired_more(seed, sep)
    assert len(s0) == 6 and ref.found(s0, cs) == 6
    assert len(o["seeds"]) == 12 and ref.matched(o["seeds"], cs)
    assert np.array_equal(o["seeds"][:6], s0) and np.array_equal(o["round"], [0] * 6 + [1] * 6)
    assert o["ended"] == "none accepted" and len(o["accepted"]) <= 3 and o["accepted"][-1] == 0
    d = ((o["seeds"][:, None, :] - cs[None]) ** 2).sum(2)
    worst = demix_ref.worst_cell(o["e"]["C"], act[d.argmin(1)])
    planted = demix_ref.worst_cell(demix_ref.paired_run(seed, sep)[3]["C"], act)
    print("seed %d sep %d: accepted %s, lowest accepted %.3f, best rejected %.3f, worst cell %.4f (planted seeds %.4f), "
          "clipped %s" % (seed, sep, o["accepted"], o["scores"][0].min(), o["top"][0][len(o["scores"][0])], worst, planted,
                          o["clipped"]))
    assert abs(worst - planted) <= 0.02
    assert max(o["clipped"]) <= v.size // 10000


@pytest.mark.parametrize("seed", range(6))
def test_four_pixels_apart_is_measured(seed):
    """sep 4, min_score 0.76: how many of the twelve are found is recorded in DESIGN.md section 15, not asserted.  With
    and (seed 1) without blanking, whatever is refused, find_more returns: unblanked, seed 1 puts a residual peak into a
    seeded pixel in both rounds, and the search goes on past it."""
    v, cs, act, s0, sc0, o = ref.paired_more(seed, 4, 0.76)
    print("seed %d sep 4: %d of 12 found, %d seeds, refused %s" % (seed, ref.found(o["seeds"], cs), len(o["seeds"]),
                                                                 [(r[0], r[1].tolist(), r[3]) for r in o["refused"]]))
    assert len(o["seeds"]) >= 6 and len(o["round"]) == len(o["seeds"])
    assert all(r[3] in ("seeded", "roi") for r in o["refused"])
    if seed == 1:
        raw = ref.find_more(v, roi_ref.planted_map(), s0, 0.76, blank=None, alpha=1.0)
        print("  without blanking: %d of 12 found, refused %s" % (ref.found(raw["seeds"], cs),
                                                                   [(r[0], r[1].tolist(), r[3]) for r in raw["refused"]]))
        assert len(raw["seeds"]) >= 6 and raw["refused"] and all(r[3] == "seeded" for r in raw["refused"])
        assert len(raw["seeds"]) == 6 + sum(raw["accepted"])


def test_model_and_blank_discs_equal_the_restatement():
    from hydra_mi import residual
    rng = np.random.default_rng(3)
    P, R, F, shape = 4, 3, 9, (20, 24)
    pts = np.array([[3.5, 2.5], [5.5, 4.5], [22.5, 18.5], [6.5, 3.5]])             # windows off the frame, three overlapping
    a_q = rng.integers(0, 3, (P, 7, 7)).astype(np.uint16) * rng.integers(1, 32768, (P, 7, 7)).astype(np.uint16)
    a_q[:, R, R] = 65535
    e = {"shapes_q": a_q, "C": rng.normal(0.0, 30.0, (F, P))}
    seeds = np.floor(pts).astype(np.int64)
    for nl in (1, 2, 4):
        got, want = residual.model(e, shape, nl, points=pts), ref.model(e, seeds, shape, nl)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
    assert residual.model(e, shape, 1, points=pts)[3] > 0 and (got[2] < 0).any() and (got[2] > 0).any()
    assert np.array_equal(residual.model(dict(e, points=pts), shape)[2], want[2])  # (find_more's dicts carry their points)
    # a one-pixel cell of l grey levels (C = l there: sum a^2 / sum a = 65535) takes l levels off its pixel
    one = np.zeros((1, 7, 7), np.uint16)
    one[0, R, R] = 65535
    lev = np.array([[-3.0], [0.0], [3.0]])
    tr = residual.model({"shapes_q": one, "C": lev}, shape, points=pts[:1])[2]
    assert np.array_equal((65535 * tr[:, 0].astype(np.int64) + (1 << 23)) >> 24, [-3, 0, 3])
    for radius in (0, 1, 2, 5):
        b = residual.blank_discs(pts, radius, shape)
        assert b.dtype == np.uint8 and np.array_equal(b, ref.blank_discs(seeds, radius, shape))
    assert residual.blank_discs(pts[:1], 2, shape).sum() == 13 and residual.blank_discs(pts[2:3], 2, shape).sum() == 11


def test_argument_checks_of_the_python_layer():
    from hydra_mi import residual

    class Body:
        keep, H, W, r = False, 8, 8, None

    e = {"shapes_q": np.full((1, 3, 3), 65535, np.uint16), "C": np.zeros((4, 1))}
    with pytest.raises(ValueError, match="carries no points"):
        residual.model(e, (8, 8))
    with pytest.raises(ValueError, match=r"shapes of shape \(1, 3, 3\) and 2 points for traces of 1 cells"):
        residual.model(e, (8, 8), points=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="n_layers 5 outside 1..4"):
        residual.model(e, (8, 8), 5, points=np.ones((1, 2)))
    with pytest.raises(OverflowError, match="trace of cell 0 does not fit int32"):
        residual.model(dict(e, C=np.array([[0.0], [1e8], [0.0], [0.0]])), (8, 8), points=np.ones((1, 2)))
    with pytest.raises(OverflowError):
        residual.model(dict(e, C=np.array([[0.0], [np.nan], [0.0], [0.0]])), (8, 8), points=np.ones((1, 2)))
    for call in (lambda: residual.summary(Body(), e, points=np.ones((1, 2))),
                 lambda: residual.find_more(Body(), np.ones((1, 2)), 0.8),
                 lambda: residual.write_video(Body(), "x.avi", e, points=np.ones((1, 2)))):
        with pytest.raises(RuntimeError, match="without keep=True"):
            call()
    kept = Body()
    kept.keep = True
    for kw, text in ((dict(blank=-1), "blank -1"), (dict(blank=1.5), "blank 1.5"), (dict(offset=256), "offset 256 outside 0..255"),
                     (dict(offset=-1), "offset -1 outside 0..255")):
        with pytest.raises(ValueError, match=text):
            residual.summary(kept, e, points=np.ones((1, 2)), **kw)
        with pytest.raises(ValueError, match=text):
            residual.find_more(kept, np.ones((1, 2)), 0.8, **kw)
    for kw, text in ((dict(min_score=None), "min_score None"), (dict(min_score=np.nan), "min_score nan"),
                     (dict(min_score=0.8, rounds=0), "rounds 0"), (dict(min_score=0.8, max_new=-1), "max_new -1")):
        with pytest.raises(ValueError, match=text):
            residual.find_more(kept, np.ones((1, 2)), **kw)
    with pytest.raises(ValueError, match="no point to start from"):
        residual.find_more(kept, np.zeros((0, 2)), 0.8)
    with pytest.raises(TypeError):
        residual.find_more(kept, np.ones((1, 2)))                               # min_score has no default
