"""Co-active cells on the CPU: the restatement (tests/network_ref.py) against np.corrcoef and Python integers, the host
arithmetic of hydra_mi.network against the restatement bit for bit (the device's sums supplied by the restatement), the
rules of ensembles, lead_lag, ensemble_map and quantise on hand-made cases, and the planted video with ensembles, which
has to show that the planted ensembles and the planted lag are found."""
import numpy as np
import pytest

import network_ref as ref
import roi_ref

ROI_THR = 0.47        # hydra_mi.roi.DEFAULT_THR
SEEDS = (0, 1, 2, 3, 4)
WITHIN = 0.68         # the lowest within-ensemble correlation of the restatement over SEEDS, 0.6822 (seed 1), rounded down
BETWEEN = 0.43        # the highest between two ensembles, 0.4235 (seed 4), rounded up
THR = 0.55            # hydra_mi.network.DEFAULT_THR: halfway between the two


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Sums:
    """the reduction of the device, computed by the restatement on a video in host memory"""

    def __init__(self, regs, inmap):
        self.regs, self.m = regs, inmap

    def body_rec_count(self):
        return self.regs.shape[0]

    def body_rec_trace_maps(self, q, want=("c", "w1", "w2")):
        assert q.dtype == np.int32 and q.flags["C_CONTIGUOUS"] and q.shape[0] == self.regs.shape[0] and 1 <= q.shape[1] <= 1024
        c, w1, w2 = ref.trace_maps(self.regs, self.m, q)
        return {k: v for k, v in (("c", c), ("w1", w1), ("w2", w2)) if k in want}


class _Body:
    keep = True

    def __init__(self, regs, inmap):
        self.r = _Sums(regs, inmap)
        self.tri_of_pixel = np.where(inmap, 0, -1).astype(np.int32)


def _small(seed=3, F=40, H=9, W=11, K=5):
    rng = np.random.default_rng(seed)
    regs = rng.integers(0, 256, (F, H, W)).astype(np.uint8)
    regs[:, 2, 3] = 77                                             # a constant pixel
    regs[0, 4, 4], regs[1, 4, 4] = 0, 255
    m = np.ones((H, W), bool)
    m[0, :], m[:, 0], m[5, 6] = False, False, False
    x = rng.normal(0.0, 1.0, (K, F))
    x[1] = 0.0                                                     # a trace that is zero
    x[2] = 0.25 * regs[:, 3, 3] - 7.0                              # a trace that is a pixel: rho 1 there
    return regs, m, x


def test_restated_rho_matches_corrcoef(hm):
    """The restated rho is the correlation of a pixel with the quantised trace: against np.corrcoef on the same whole
    numbers as floats within 1e-12 (the sums are exact, so only corrcoef's own rounding of n = 40 terms is in it)."""
    regs, m, x = _small()
    q = ref.quantise(x)
    got = ref.maps(regs, m, x)
    assert np.isnan(got[:, ~m]).all() and not np.isnan(got[:, m]).any()
    assert (got[1][m] == 0.0).all() and (got[:, 2, 3] == 0.0).all()
    worst = 0.0
    for s in (0, 2, 3, 4):
        for y, xx in zip(*np.nonzero(m)):
            if (y, xx) == (2, 3):
                continue
            worst = max(worst, abs(got[s, y, xx] - np.corrcoef(regs[:, y, xx].astype(np.float64), q[s].astype(np.float64))[0, 1]))
    print("rho against np.corrcoef: %.3g" % worst)
    assert worst <= 1e-12
    assert abs(got[2, 3, 3] - 1.0) <= 1e-4                          # (the quantised copy of the pixel)


def test_int64_path_equals_python_integers(hm):
    """network.rho_from_sums (int64, one rounding each) on the restated sums equals the restatement in Python integers bit
    for bit, also at the largest values a short record allows: v 255 and q +-32767 throughout."""
    from hydra_mi import network
    regs, m, x = _small()
    q = ref.quantise(x)
    assert np.array_equal(network.quantise(x), q) and network.quantise(x).dtype == np.int32
    c, w1, w2 = ref.trace_maps(regs, m, q.T)
    # the sums themselves, in Python integers
    for s, y, xx in ((0, 1, 1), (2, 3, 3), (4, 8, 10), (3, 5, 6)):
        v = [int(t) for t in regs[:, y, xx]] if m[y, xx] else [0] * len(regs)
        assert int(c[s, y, xx]) == sum(a * int(b) for a, b in zip(v, q[s])) and int(w1[y, xx]) == sum(v)
        assert int(w2[y, xx]) == sum(a * a for a in v)
    assert _same(network.rho_from_sums(c, w1, w2, q, m), ref.rho(c, w1, w2, q, m))
    assert _same(network.maps(_Body(regs, m), x), ref.maps(regs, m, x))
    F = 64
    big = np.full((F, 2, 2), 255, np.uint8)
    big[::3, 0, 0] = 0
    qb = np.full((2, F), 32767, np.int32)
    qb[0, ::3] = -32767
    mb = np.ones((2, 2), bool)
    cb, b1, b2 = ref.trace_maps(big, mb, qb.T)
    assert int(cb[1, 1, 1]) == 255 * 32767 * F                      # (trace 1 is constant: its rho is 0)
    got = network.rho_from_sums(cb, b1, b2, qb, mb)
    assert _same(got, ref.rho(cb, b1, b2, qb, mb)) and abs(got[0, 0, 0] - 1.0) <= 1e-15 and (got[:, 1, 1] == 0.0).all() and (got[1] == 0.0).all()
    with pytest.raises(RuntimeError, match="without keep=True"):
        network.maps(type("B", (), {"keep": False})(), x)
    with pytest.raises(ValueError, match="traces of 39 frames for a record of 40"):
        network.maps(_Body(regs, m), x[:, :39])


def test_coactivity_symmetry_and_diagonal(hm):
    from hydra_mi import network
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.0, (6, 50))
    x[3, 10:] = x[0, :40]                                           # cell 3 follows cell 0 by 10 frames
    x[4] = 2.5                                                      # a constant trace
    x[5, :45] = 1.0                                                 # constant but for its end: a constant piece at large lags
    L = 12
    r = network.coactivity(x, L)
    assert r.shape == (6, 6, 2 * L + 1) and _same(r, ref.coactivity(x, L))
    assert _same(r, np.transpose(r, (1, 0, 2))[:, :, ::-1])         # (i, j, l) <-> (j, i, -l)
    live = [0, 1, 2, 3, 5]
    assert all(r[i, i, L] == 1.0 for i in live)
    assert np.isnan(r[4]).all() and np.isnan(r[:, 4]).all()
    assert np.isnan(r[0, 5, L - 6]) and not np.isnan(r[0, 5, L + 6]) and not np.isnan(r[0, 5, L])    # x_5[:F - 6] is constant
    assert abs(r[0, 3, L + 10] - 1.0) <= 1e-12 and np.nanargmax(r[0, 3]) == L + 10 and np.nanargmax(r[3, 0]) == L - 10
    worst = 0.0
    for i in live:
        for j in live:
            for l in (0, 3, 12):
                if not np.isnan(r[i, j, L + l]):
                    worst = max(worst, abs(r[i, j, L + l] - np.corrcoef(x[i, :50 - l], x[j, l:])[0, 1]))
    print("coactivity against np.corrcoef: %.3g" % worst)
    assert worst <= 1e-12
    assert _same(network.coactivity(x)[:, :, 0], r[:, :, L])
    short = network.coactivity(x[:, :3], 5)                         # lags beyond the frames: NaN
    assert np.isnan(short[:, :, [0, 1, 2, 8, 9, 10]]).all() and _same(short, ref.coactivity(x[:, :3], 5))
    with pytest.raises(ValueError, match="negative"):
        network.coactivity(x, -1)


def test_ensembles_chain_tie_and_singleton(hm):
    """Six cells: 1 - 3 - 5 is a chain (1 and 5 are joined through 3 only), 0 - 2 a pair, 4 alone."""
    from hydra_mi import network
    r0 = np.eye(6)
    for i, j, v in ((1, 3, 0.8), (3, 5, 0.6), (1, 5, 0.1), (0, 2, 0.6), (4, 0, 0.59), (4, 1, np.nan)):
        r0[i, j] = r0[j, i] = v
    want = np.array([1, 0, 1, 0, -1, 0], np.int32)
    for f in (network.ensembles, ref.ensembles):
        got = f(r0, 0.6)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    # a tie in size: three pairs -> numbered by lowest member
    r1 = np.eye(6)
    for i, j in ((4, 5), (0, 3), (1, 2)):
        r1[i, j] = r1[j, i] = 0.9
    assert np.array_equal(network.ensembles(r1, 0.9), [0, 1, 1, 0, 2, 2]) and np.array_equal(ref.ensembles(r1, 0.9), [0, 1, 1, 0, 2, 2])
    assert np.array_equal(network.ensembles(r1, 0.91), [-1] * 6) and np.array_equal(ref.ensembles(r1, 0.91), [-1] * 6)
    assert np.array_equal(network.ensembles(r1), network.ensembles(r1, THR)) and network.DEFAULT_THR == THR
    assert network.ensembles(np.zeros((0, 0))).shape == (0,)
    x = np.arange(12.0).reshape(6, 2) ** 2
    et = network.ensemble_traces(x, want)
    assert _same(et, ref.ensemble_traces(x, want)) and _same(et[1], (x[0] + x[2]) / 2.0) and et.shape == (2, 2)
    assert network.ensemble_traces(x, np.full(6, -1)).shape == (0, 2)


def test_lead_lag_ties(hm):
    from hydra_mi import network
    F = 40
    a = np.zeros(F)
    a[[10, 25]] = 1.0
    b = np.zeros(F)
    b[[13, 28]] = 1.0                                               # a, 3 frames later
    lag, peak = network.lead_lag(np.array([a, b]), 5)
    lr, pr = ref.lead_lag(np.array([a, b]), 5)
    assert lag.dtype == np.int32 and np.array_equal(lag, lr) and _same(peak, pr)
    assert lag[0, 1] == 3 and lag[1, 0] == -3 and lag[0, 0] == 0 and peak[0, 0] == 1.0 and peak[0, 1] > 0.99
    # ties: a trace periodic in 4 frames against itself has r = 1 at lags -4, 0 and 4 up to rounding; made exact here by
    # patching coactivity's values, the rule is what is under test
    r = np.full((2, 2, 7), 0.25)
    r[0, 1, [0, 2, 4]] = 0.75                                       # lags -3, -1, 1: -1 and 1 are as near, the positive wins
    r[1, 0, [1, 6]] = 0.5                                           # lags -2, 3: the smaller |lag|
    r[1, 1, :] = np.nan
    r[0, 0, [0, 3, 6]] = 1.0
    for mod in (network, ref):
        old = mod.coactivity
        mod.coactivity = lambda x, max_lag, r=r: r
        try:
            lag, peak = mod.lead_lag(np.zeros((2, 9)), 3)
        finally:
            mod.coactivity = old
        assert lag.tolist() == [[0, 1], [-2, 0]]
        assert peak[0, 0] == 1.0 and peak[0, 1] == 0.75 and peak[1, 0] == 0.5 and np.isnan(peak[1, 1])


def test_ensemble_map_ties_and_nan(hm):
    from hydra_mi import network
    nan = np.nan
    rho = np.array([[[0.5, 0.2, nan, nan, 0.3, 0.7]],
                    [[0.5, 0.6, 0.4, nan, 0.3, nan]],
                    [[0.1, 0.6, nan, nan, 0.29, 0.9]]])
    want = np.array([[0, 1, 1, -1, -1, 2]], np.int16)
    for f in (network.ensemble_map, ref.ensemble_map):
        got = f(rho, 0.4)
        assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(network.ensemble_map(rho, 0.3)[0], [0, 1, 1, -1, 0, 2])          # exactly thr counts; the tie to 0
    assert np.array_equal(network.ensemble_map(np.zeros((0, 2, 3)), 0.1), np.full((2, 3), -1))
    img = network.colour_map(want, np.array([[10, 20, 30, 40, 50, 60]], np.uint8))
    from hydra_mi import cellview
    pal = cellview.palette(3).astype(int)
    assert img.dtype == np.uint8 and img.shape == (1, 6, 3) and img[0, 3].tolist() == [40, 40, 40]
    assert img[0, 0].tolist() == ((10 + pal[0] + 1) >> 1).tolist() and img[0, 5].tolist() == ((60 + pal[2] + 1) >> 1).tolist()


def test_quantise_extremes(hm):
    from hydra_mi import network
    x = np.array([[0.0, 0.0, 0.0, 0.0],
                  [2.0 ** -1000, -2.0 ** -1000, 2.0 ** -1001, 0.0],             # 16383.5: the tie goes to even
                  [2.0 ** 1000, -2.0 ** 1000, 0.0, 2.0 ** 999],
                  [-3.0, 1.0, 2.0, 1.5 / 32767.0 * 3.0],
                  [0.5 / 32767.0, 1.0, -0.5 / 32767.0, 1.5 / 32767.0]])
    q = network.quantise(x)
    assert q.dtype == np.int32 and np.array_equal(q, ref.quantise(x))
    assert q[0].tolist() == [0, 0, 0, 0] and q[1].tolist() == [32767, -32767, 16384, 0]
    assert q[2].tolist() == [32767, -32767, 0, 16384] and q[3].tolist()[:3] == [-32767, 10922, 21845]
    assert np.abs(q).max() == 32767 and q[4, 1] == 32767 and abs(q[4, 0]) <= 1 and q[4, 3] in (1, 2)
    assert network.quantise(np.zeros((0, 5))).shape == (0, 5) and network.quantise(np.zeros((2, 0))).shape == (2, 0)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[3, 2] = bad
        with pytest.raises(ValueError, match="trace 3 is not finite in frame 2"):
            network.quantise(y)
        with pytest.raises(ValueError):
            ref.quantise(y)


def test_strain_coupling(hm):
    from hydra_mi import network
    rng = np.random.default_rng(2)
    ens = rng.normal(0.0, 1.0, (3, 30))
    J = 1.0 + 0.1 * rng.normal(0.0, 1.0, (30, 5))
    J[:, 1] = 1.0 - 0.05 * ens[2]                                   # a triangle that shrinks with ensemble 2
    J[7, 3] = np.nan
    J[:, 4] = 1.0
    got = network.strain_coupling(ens, J)
    assert got.shape == (3, 5) and _same(got, ref.strain_coupling(ens, J))
    assert abs(got[2, 1] + 1.0) <= 1e-12 and np.isnan(got[:, 3]).all() and np.isnan(got[:, 4]).all() and not np.isnan(got[:, :3]).any()
    assert abs(got[0, 0] - np.corrcoef(ens[0], J[:, 0])[0, 1]) <= 1e-12


@pytest.fixture(scope="module")
def planted():
    m = roi_ref.planted_map()
    out = {}
    for seed in SEEDS:
        v, cs, act = ref.planted_video(seed)
        out[seed] = (v, cs, act, roi_ref.extract(v, m, cs, thr=ROI_THR))
    return m, out


def test_planted_ensembles_and_lag_are_found(hm, planted):
    """On the planted video with ensembles through roi_ref.extract (its defaults, thr 0.47), seeds 0..4, measured on the
    restatement: the lowest correlation of dF/F within an ensemble is 0.7770, 0.6822, 0.7178, 0.7001, 0.7116 and the
    highest between two ensembles 0.2438, 0.3471, 0.1801, 0.3237, 0.4235, a gap of 0.29 at the least (every seed has the
    0.2 asked for); DEFAULT_THR 0.55 is halfway between 0.6822 and 0.4235.  Ensemble 0 leads ensemble 2 by 8 frames
    with r 0.902 .. 0.960, against 0.043 .. 0.300 at lag 0.  Asserted: the three planted ensembles exactly, the lag, the
    two figures, and hydra_mi.network equal to the restatement bit for bit."""
    from hydra_mi import network
    m, runs = planted
    for seed in SEEDS:
        v, cs, act, e = runs[seed]
        x = e["dff"].T
        lo, hi, (lag, peak, at0) = ref.figures(e["dff"])
        print("seed %d: within %.4f between %.4f, 0 -> 2 at lag %d r %.4f (lag 0: %.4f)" % (seed, lo, hi, lag, peak, at0))
        assert lo >= WITHIN and hi <= BETWEEN and lo - hi >= 0.2
        r = network.coactivity(x, 10)
        assert _same(r, ref.coactivity(x, 10))
        labels = network.ensembles(r[:, :, 10])
        assert np.array_equal(labels, ref.planted_labels()) and np.array_equal(labels, ref.ensembles(r[:, :, 10], THR))
        ens = network.ensemble_traces(x, labels)
        assert _same(ens, ref.ensemble_traces(x, labels))
        ll, pk = network.lead_lag(ens, 10)
        lr, pr = ref.lead_lag(ens, 10)
        assert np.array_equal(ll, lr) and _same(pk, pr)
        assert ll[0, 2] == 8 and ll[2, 0] == -8 and pk[0, 2] >= 0.9 and pk[0, 2] == peak and at0 <= 0.31


def test_planted_maps_show_the_ensembles(hm, planted):
    """The ensembles' maps of the planted video (seed 1, the narrowest gap within an ensemble): network.maps on the
    restated sums equals the restatement bit for bit.  Measured over seeds 0..4: the map of its own ensemble is 0.812 at
    the least at a planted centre; another ensemble's map at a centre, or any map more than 8 px from every cell, is
    0.428 at the most; DEFAULT_MAP_THR 0.62 is halfway.  Asserted for seed 1 (0.8120 and 0.4080): both figures, every
    planted centre in its own ensemble in the ensemble map, and no pixel far from the cells in any."""
    from hydra_mi import network
    m, runs = planted
    v, cs, act, e = runs[1]
    ens = ref.ensemble_traces(e["dff"].T, ref.planted_labels())
    rho = network.maps(_Body(v, m), ens)
    assert rho.shape == (3,) + m.shape and _same(rho, ref.maps(v, m, ens))
    own = min(rho[ref.planted_ensemble(i), r, c] for i, (c, r) in enumerate(cs))
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    far = m & np.all([(xx - c) ** 2 + (yy - r) ** 2 > 64 for c, r in cs], axis=0)
    other = max(np.nanmax(rho[:, far]), max(rho[k, r, c] for i, (c, r) in enumerate(cs) for k in range(3) if k != ref.planted_ensemble(i)))
    print("seed 1: own ensemble at a centre %.4f at the least, elsewhere %.4f at the most" % (own, other))
    assert own >= 0.81 and other <= 0.43 and network.DEFAULT_MAP_THR == 0.62
    em = network.ensemble_map(rho, network.DEFAULT_MAP_THR)
    assert np.array_equal(em, ref.ensemble_map(rho, network.DEFAULT_MAP_THR)) and (em[~m] == -1).all() and (em[far] == -1).all()
    assert [int(em[r, c]) for c, r in cs] == [ref.planted_ensemble(i) for i in range(12)]
