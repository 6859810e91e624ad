"""Exact reference of the measurement sums, its entrywise bound and its case table, shared by
tests/test_measure_exact_cpu.py (the reference alone), tests/test_measure_precision_gpu.py (the device against it) and
tools/measure_precision_table.py (the record under profiles/measure_precision.md).

The measurement (csrc/ekf_kernels.h: k_star_regions, k_measure_vertex, k_measure_edge, k_hth_scatter; the per-pixel
reductions k_jz, k_j, k_jz_multi, k_j_multi and the flow terms of k_render_iter) forms sums over pixels whose every
term can be written down exactly, so the reference here rounds nothing that matters: python ints and Fractions.

Definitions.  Inputs: a state X (4N doubles), delta (2.0), the texture, eps_Z, eps_J, eps_M as the exact values of their
doubles, an observation y_im (uint8), the flow as passed (binary32, masked or raw) and y_m in {0, 1}.  R(X) is the
oracle's render (ekf_ref.render, to which existing tests hold the device bit for bit): im (uint8), fx, fy (binary32),
m in {0, 255}; r = R(X).  The difference image of coordinate k with sign s is D^s_k = R(X + s delta e_k) - r: integers
for im and m (units of 1/255), the binary32 difference fl32(p - r) for fx and fy.  The residuals are z_im = y_im - r.im,
z_m = 255 y_m - r.m (integers), z_fx = fl32(flow_x - r.fx), z_fy = fl32(flow_y + r.fy).  Then

    Hzc[k] = ( sum (D+ - D-)_im z_im / 255^2 / eps_Z,    sum (D+ - D-)_fx z_fx / eps_J,
              -sum (D+ - D-)_fy z_fy / eps_J,            sum (D+ - D-)_m z_m / 255^2 / eps_M ) / delta / 2
    Hz[k]  = the sum of the four
    HTH[i,j] = ( sum D+_i,im D+_j,im / 255^2 / eps_Z + sum D+_i,fx D+_j,fx / eps_J + sum D+_i,fy D+_j,fy / eps_J
               + sum D+_i,m D+_j,m / 255^2 / eps_M ) / delta^2        where J[i,j] = 1 (ekf_ref.adjacency), else 0

Image and mask terms are integers over 255^2 and summed as python ints.  A flow term is a product of two binary32
numbers, exact in binary64; a channel's flow terms are summed with math.fsum, which rounds the exact sum once
(counted in C below).  Everything after that is Fraction arithmetic.

Next to each exact value stand the absolute mass M -- the same expression with every term replaced by its absolute
value, |D+ - D-| by |D+| + |D-| -- and the count n of (pixel, channel) terms whose absolute value is not zero.

The bar, per entry:    |device - exact| <= (n + C) u M,    u = 2^-53.

n u M covers the sum itself: n non-zero terms added in any order and any tree take n - 1 rounded additions (adding
a zero is exact), each rounding at most u times a partial sum of at most M: (n - 1) u M to first order, and
gamma_(n-1) <= n u exactly as long as n (n - 1) u <= 1.  Workgroup splits, wave shuffles and fused multiply-adds
only lower it.  C counts the roundings outside the sum, each at most u M, along the longest path of any code held to
this bar:

    path                                  per term                         after the sum                          count
    k_measure_vertex, Hz position row     k255[D+], k255[D-], their        / eps, three channel additions,           9
      (A_X, A_Y; k_hth_scatter)           difference, k255[z]  (3; the     / delta, / 2  (1 + 3 + 2)
                                          flow difference D+ - D- formed
                                          in binary64 is 1, z exact)
    k_measure_vertex / k_measure_edge,    k255[D_i], k255[D_j], iZ =       / delta, / delta  (2)                     6
      HTH geometry block                  1 / eps_Z, D_i iZ  (4; flow: iJ
                                          and the product, 2; mask: iM, 1)
    HTH velocity entries                  none (binary32 products)         / eps_J, / delta, / delta  (3)            3
    hm_jz, hm_jz_multi (k_jz, k_jz_multi) D / 255, z / 255, product (3)    / eps, three additions  (4)               7
    hm_j, hm_j_multi (k_j, k_j_multi)     two quotients, product (3)       / eps, three additions  (4)               7
    hm_error flow terms (k_render_iter)   none                             none                                      0
    the binary64 oracle (ekf_ref, ekf_c)  D / 255, z / 255, product (3)    / eps, three additions, / delta twice,   10
      central difference of two jz                                         the subtraction, / 2  (1 + 3 + 2 + 1 + 1,
                                                                           the last exact)
    this reference                        none                             math.fsum of a flow channel               1

The oracle's path and the reference's own rounding add up to 11, the largest count:  C = 11.  (With mixed channels a
term's share is bounded by its channel's count, so the largest count bounds the whole entry.)  C is this derivation,
not a measurement.

Precondition of exactness (measure only; `coverage`): k_measure_vertex forms a perturbed flow pixel as
(r - star_ref) + star_perturbed in binary32.  That is the full render of the perturbed state bit for bit as long as no
pixel is covered by more than one triangle in the reference configuration and by more than two in a perturbed one
(binary32 addition of two summands is commutative; with three the order matters).  The jz / j / error operators
render every state in full and need no such condition.

Test infrastructure: the package does not import this module."""
import math
import os
import zlib
from fractions import Fraction

import numpy as np

import measure_cases as mc
from oracle import ekf_c, ekf_ref

U = Fraction(1, 2 ** 53)
C = 11
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q255 = 255 * 255
CHANNELS = ("im", "fx", "fy", "m")


def bound(n, M):
    """(n + C) u M as a Fraction (M a Fraction or a float)"""
    return (int(n) + C) * U * Fraction(M)


# ---- difference images, cropped to their support ----------------------------------------------------------------------
class _Diff:
    """D = p - r of one perturbed state, the four channels cropped to the bounding box of their non-zero pixels
    (box = r0, r1, c0, c1, ends exclusive; 0, 0, 0, 0: nothing differs).  im, m: int64; fx, fy: the binary32 differences
    held in float64."""

    def __init__(self, p, r):
        d = (p[0].astype(np.int64) - r[0].astype(np.int64), (p[1] - r[1]).astype(np.float64),
             (p[2] - r[2]).astype(np.float64), p[3].astype(np.int64) - r[3].astype(np.int64))
        nz = (d[0] != 0) | (d[1] != 0) | (d[2] != 0) | (d[3] != 0)
        rows, cols = np.flatnonzero(nz.any(axis=1)), np.flatnonzero(nz.any(axis=0))
        self.box = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1) if len(rows) else (0, 0, 0, 0)
        b = self.box
        self.ch = tuple(np.ascontiguousarray(a[b[0]:b[1], b[2]:b[3]]) for a in d)

    def on(self, box):
        """the four channels on `box` (zeros where it leaves this difference's own box)"""
        b = self.box
        r0, r1, c0, c1 = max(box[0], b[0]), min(box[1], b[1]), max(box[2], b[2]), min(box[3], b[3])
        if (r0, r1, c0, c1) == tuple(box):
            return tuple(a[r0 - b[0]:r1 - b[0], c0 - b[2]:c1 - b[2]] for a in self.ch)
        out = tuple(np.zeros((box[1] - box[0], box[3] - box[2]), a.dtype) for a in self.ch)
        if r0 < r1 and c0 < c1:
            for o, a in zip(out, self.ch):
                o[r0 - box[0]:r1 - box[0], c0 - box[2]:c1 - box[2]] = a[r0 - b[0]:r1 - b[0], c0 - b[2]:c1 - b[2]]
        return out


def _union(a, b):
    if a[0] >= a[1]:
        return b
    if b[0] >= b[1]:
        return a
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))


def _meet(a, b):
    return (max(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), min(a[3], b[3]))


def _empty(b):
    return b[0] >= b[1] or b[2] >= b[3]


# ---- one channel of one entry: sum over `pairs` (sign, a, b) of sign * a * b over the pixels -----------------------
class Sum:
    """exact value S, absolute mass M (Fractions), count n of non-zero terms, `big`: the term of the largest absolute
    value (signed, a Fraction), `terms`: the terms as binary64 (only when asked for: the planted faults)"""
    __slots__ = ("S", "M", "n", "big", "terms")

    def __init__(self, S=Fraction(0), M=Fraction(0), n=0, big=Fraction(0), terms=None):
        self.S, self.M, self.n, self.big, self.terms = S, M, n, big, terms

    def scaled(self, w):
        """the same sum with every term multiplied by the Fraction w"""
        t = None if self.terms is None else self.terms * float(w)
        return Sum(self.S * w, self.M * abs(w), self.n, self.big * w, t)

    @staticmethod
    def add(parts):
        """the sum of several channels' sums (their terms side by side)"""
        big = max((p.big for p in parts), key=abs)
        terms = None
        if all(p.terms is not None for p in parts):
            terms = np.concatenate([p.terms for p in parts])
        return Sum(sum((p.S for p in parts), Fraction(0)), sum((p.M for p in parts), Fraction(0)),
                   sum(p.n for p in parts), big, terms)

    def bound(self):
        return bound(self.n, self.M)


def _channel(pairs, integer, keep):
    """pairs: (sign, a, b), arrays over the same pixels -> Sum.  A pixel is one term of n: the pairs' products there
    added up with their signs; its absolute value in the mass is the sum of the products' absolute values.  `big` is the
    largest single product (one pixel of one pair: at least M / (len(pairs) n))."""
    if integer:
        prods = [(sg, a * b) for sg, a, b in pairs]
        mass = sum(np.abs(p) for _, p in prods)
        n = int(np.count_nonzero(mass))
        if n == 0:
            return Sum(terms=np.zeros(0) if keep else None)
        tot = sum(sg * p for sg, p in prods)
        big = max((int(sg * p.ravel()[np.argmax(np.abs(p))]) for sg, p in prods), key=abs)
        return Sum(Fraction(int(tot.sum()), Q255), Fraction(int(mass.sum()), Q255), n, Fraction(big, Q255),
                   tot.ravel()[mass.ravel() != 0] / float(Q255) if keep else None)
    prods = [(sg, a * b) for sg, a, b in pairs]                   # binary32 x binary32: exact in binary64
    nzm = np.zeros(prods[0][1].shape, bool)
    for _, p in prods:
        nzm |= p != 0
    n = int(np.count_nonzero(nzm))
    if n == 0:
        return Sum(terms=np.zeros(0) if keep else None)
    signed = np.concatenate([(sg * p)[p != 0] for sg, p in prods])
    S = Fraction(math.fsum(signed.tolist()))
    M = Fraction(math.fsum(np.abs(signed).tolist()))
    big = Fraction(float(signed[np.argmax(np.abs(signed))]))
    tot = sum(sg * p for sg, p in prods)                          # (a pixel's net term, rounded: the planted faults only)
    return Sum(S, M, n, big, tot.ravel()[nzm.ravel()] if keep else None)


INTEGER = (True, False, False, True)


class Exact:
    """The exact sums of one case: a mesh (p, t), a texture, a state X, an observation, eps = (eps_Z, eps_J, eps_M) and
    delta.  `flow` is the flow as passed to the operator (masked or raw)."""

    def __init__(self, p, t, tex, X, y_im, flow, y_m, eps=(1e-3, 1.0, 1.0), delta=2.0, keep_terms=False):
        self.p, self.t = np.asarray(p, np.float64), np.asarray(t, np.int64)
        self.N = len(self.p)
        tex = np.asarray(tex)
        self.tex = np.ascontiguousarray(tex if tex.ndim == 2 else tex[:, :, 0], np.uint8)
        self.H, self.W = self.tex.shape
        self.X = np.array(X, np.float64).reshape(-1)
        self.eps = tuple(float(e) for e in eps)
        self.w = (1 / Fraction(self.eps[0]), 1 / Fraction(self.eps[1]), 1 / Fraction(self.eps[1]), 1 / Fraction(self.eps[2]))
        self.delta = float(delta)
        self.keep = keep_terms
        self.obs = (np.asarray(y_im, np.uint8), np.asarray(flow, np.float32), np.asarray(y_m, np.uint8))
        self._cm = ekf_c.Measurement(self.N, self.t, self.p, self.tex, *self.eps)      # renders bit for bit like ekf_ref
        self.r = self.render(self.X)
        r = self.r
        self.z = ((self.obs[0].astype(np.int64) - r[0].astype(np.int64)),
                  (self.obs[1][:, :, 0] - r[1]).astype(np.float64),
                  (self.obs[1][:, :, 1] + r[2]).astype(np.float64),
                  (255 * self.obs[2].astype(np.int64) - r[3].astype(np.int64)))
        self._d = {}

    def render(self, X):
        return self._cm.render(X)

    def diff(self, k, sign=1):
        """D^sign_k, cached"""
        if (k, sign) not in self._d:
            Xp = self.X.copy()
            Xp[k] += sign * self.delta
            self._d[(k, sign)] = _Diff(self.render(Xp), self.r)
        return self._d[(k, sign)]

    # -- the two kinds of sums ---------------------------------------------------------------------------------------
    def _against_z(self, plus, minus=None, select=None):
        """the four channel sums of (plus - minus) . z, signed and weighted as the components of jz (the fy channel
        negative); select: a boolean image, only those pixels"""
        box = plus.box if minus is None else _union(plus.box, minus.box)
        if _empty(box):
            return [Sum(terms=np.zeros(0) if self.keep else None) for _ in range(4)]
        a = plus.on(box)
        b = None if minus is None else minus.on(box)
        sl = (slice(box[0], box[1]), slice(box[2], box[3]))
        out = []
        for ch in range(4):
            z = self.z[ch][sl]
            if select is not None:
                z = np.where(select[sl], z, 0)
            pairs = [(1, a[ch], z)] + ([] if b is None else [(-1, b[ch], z)])
            w = self.w[ch] * (-1 if ch == 2 else 1)
            out.append(_channel(pairs, INTEGER[ch], self.keep).scaled(w))
        return out

    def _product(self, da, db, select=None):
        """the four channel sums of da . db, weighted by 1 / eps"""
        box = _meet(da.box, db.box)
        if _empty(box):
            return [Sum(terms=np.zeros(0) if self.keep else None) for _ in range(4)]
        a, b = da.on(box), db.on(box)
        sl = (slice(box[0], box[1]), slice(box[2], box[3]))
        out = []
        for ch in range(4):
            bb = b[ch] if select is None else np.where(select[sl], b[ch], 0)
            out.append(_channel([(1, a[ch], bb)], INTEGER[ch], self.keep).scaled(self.w[ch]))
        return out

    # -- Renderer.measure ------------------------------------------------------------------------------------------------
    def measure(self):
        """-> Hz [4N], Hzc [4N, 4], HTH [4N, 4N]: object arrays of Sum; HTH holds None off the pattern (the value there
        is exactly 0) and the same Sum object at [i, j] and [j, i]"""
        n4 = 4 * self.N
        sc = 1 / Fraction(self.delta) / 2
        Hz, Hzc = np.empty(n4, object), np.empty((n4, 4), object)
        for k in range(n4):
            c = [s.scaled(sc) for s in self._against_z(self.diff(k, 1), self.diff(k, -1))]
            Hzc[k] = c
            Hz[k] = Sum.add(c)
        _, J = ekf_ref.adjacency(self.N, self.t)
        HTH = np.empty((n4, n4), object)
        s2 = 1 / Fraction(self.delta) ** 2
        for i, j in zip(*np.nonzero(np.triu(J == 1))):
            HTH[i, j] = HTH[j, i] = Sum.add(self._product(self.diff(i), self.diff(j))).scaled(s2)
        return Hz, Hzc, HTH

    # -- the single operators (every state rendered in full: no precondition) ------------------------------------------
    def jz(self, Xp):
        """Renderer.jz at the perturbed state Xp -> (total, [im, fx, fy, m]) as Sums"""
        c = self._against_z(_Diff(self.render(Xp), self.r))
        return Sum.add(c), c

    def j_states(self, Xp, Xq):
        """sum over channels of (R(Xp) - r)(R(Xq) - r) / eps (not divided by delta^2, like Renderer.j)"""
        return Sum.add(self._product(_Diff(self.render(Xp), self.r), _Diff(self.render(Xq), self.r)))

    def j(self, i, j):
        Xp, Xq = self.X.copy(), self.X.copy()
        Xp[i] += self.delta
        Xq[j] += self.delta
        return self.j_states(Xp, Xq)

    def _face(self, labels, *states):
        m = ekf_ref.Measurement(self.N, self.t, self.p, self.tex, *self.eps)
        return m._face(np.asarray(labels), *states)

    def jz_multi(self, Xp, labels, n_labels):
        """Renderer.jz_multi: the terms of jz(Xp) per label of the pixel (ekf_ref.Measurement._face)
        -> (hz [n_labels], hzc [n_labels, 4]) of Sums"""
        face = self._face(labels, self.X, Xp)
        d = _Diff(self.render(Xp), self.r)
        hz, hzc = np.empty(n_labels, object), np.empty((n_labels, 4), object)
        for lab in range(n_labels):
            c = self._against_z(d, select=(face == lab) & (face < 65535))
            hzc[lab] = c
            hz[lab] = Sum.add(c)
        return hz, hzc

    def j_multi(self, ee, labels, n_labels):
        """Renderer.j_multi for the pairs ee (all first indices perturbed in one state, all second in another)
        -> (h [n_labels], count of the label's pixels [n_labels], hc [n_labels, 4])"""
        ee = np.asarray(ee).reshape(-1, 2)
        Xp, Xq = self.X.copy(), self.X.copy()
        Xp[ee[:, 0]] += self.delta
        Xq[ee[:, 1]] += self.delta
        face = self._face(labels, self.X, Xp, Xq)
        da, db = _Diff(self.render(Xp), self.r), _Diff(self.render(Xq), self.r)
        h, hc = np.empty(n_labels, object), np.empty((n_labels, 4), object)
        for lab in range(n_labels):
            c = self._product(da, db, select=(face == lab) & (face < 65535))
            hc[lab] = c
            h[lab] = Sum.add(c)
        return h, np.bincount(face[face < n_labels], minlength=n_labels)[:n_labels], hc

    def error_flow(self, Xs, flow=None):
        """the two flow sums of Renderer.error at state Xs (flow: the one passed to error, default the case's)
        -> (e_fx, e_fy) as Sums"""
        fl = self.obs[1] if flow is None else np.asarray(flow, np.float32)
        _, fx, fy, _ = self.render(Xs)
        dx = (fl[:, :, 0] - fx).astype(np.float64)
        dy = (fl[:, :, 1] + fy).astype(np.float64)
        return _channel([(1, dx, dx)], False, self.keep), _channel([(1, dy, dy)], False, self.keep)

    # -- the smallest change one wrong image difference makes (the planted faults) ---------------------------------------
    def unit_fault_hz(self, k):
        """the smallest non-zero change of Hzc[k, im] (and of Hz[k]) when D+_k,im is off by one unit of 1/255 at one
        pixel of the two difference images' box: the pixel of the smallest non-zero |z_im| (None: z_im is 0 there)"""
        box = _union(self.diff(k, 1).box, self.diff(k, -1).box)
        z = np.abs(self.z[0][box[0]:box[1], box[2]:box[3]])
        if not np.any(z):
            return None
        return int(z[z != 0].min()) * self.w[0] / Q255 / Fraction(self.delta) / 2

    def unit_fault_hth(self, i, j):
        """the same for HTH[i, j] and D+_i,im: the pixel of the smallest non-zero |D+_j,im| (None: there is none); for
        i = j both factors are wrong, (D + 1)^2 - D^2 = 2 D + 1, smallest where D = 0"""
        if i == j:
            return self.w[0] / Q255 / Fraction(self.delta) ** 2
        d = np.abs(self.diff(j).ch[0])
        if not np.any(d):
            return None
        return int(d[d != 0].min()) * self.w[0] / Q255 / Fraction(self.delta) ** 2

    # -- the precondition ------------------------------------------------------------------------------------------------
    def coverage(self):
        """-> (most triangles over a pixel in the reference configuration, most in any position-perturbed one); the
        velocity perturbations keep the geometry.  The render of a texture of ones shows the count as its image."""
        ones = ekf_c.Measurement(self.N, self.t, self.p, np.ones((self.H, self.W), np.uint8), *self.eps)
        cnt = lambda X: int(ones.render(X)[0].max())
        worst = 0
        for k in range(2 * self.N):
            for s in (1, -1):
                Xp = self.X.copy()
                Xp[k] += s * self.delta
                worst = max(worst, cnt(Xp))
        return cnt(self.X), worst


def precondition_holds(ex):
    ref, pert = ex.coverage()
    return ref <= 1 and pert <= 2


# ---- comparing an array of numbers with an array of Sums -------------------------------------------------------------
def ratio_one(g, s):
    """one number g against one Sum s (None: exactly 0 expected) -> (error / bound, out of bounds?).  Exact arithmetic;
    the ratio is rounded for printing.  Zero mass: g must be exactly 0."""
    g = float(g)
    if s is None or s.M == 0:
        return 0.0, g != 0.0
    if not math.isfinite(g):
        return math.inf, True
    err, b = abs(Fraction(g) - s.S), s.bound()
    return float(err / b), err > b


def ratios(got, sums):
    """got: floats, sums: Sums, same shape -> (largest error / bound over the entries of non-zero mass, the indices of
    the entries out of bounds: beyond the bound, or non-zero where the mass is zero)"""
    got = np.asarray(got, np.float64)
    worst, bad = 0.0, []
    for idx in np.ndindex(got.shape):
        r, b = ratio_one(got[idx], sums[idx])
        worst = max(worst, r)
        if b:
            bad.append(idx)
    return worst, bad


def describe(case, what, idx, got, sums):
    """the per-entry report: which job and channel an entry belongs to, n and M"""
    s = sums[idx]
    N = len(case["p"])
    vert = lambda k: "%s of vertex %d" % (("x", "y", "vx", "vy")[(k % 2) + 2 * (k >= 2 * N)], (k % (2 * N)) // 2)
    if what == "HTH":
        i, j = idx
        vi, vj = (i % (2 * N)) // 2, (j % (2 * N)) // 2
        job = "vertex job %d" % vi if vi == vj else "edge job (%d, %d)" % (min(vi, vj), max(vi, vj))
        name = "HTH[%s, %s] (%s)" % (vert(i), vert(j), job)
    elif what == "Hzc":
        name = "Hzc[%s, channel %s] (vertex job %d)" % (vert(idx[0]), CHANNELS[idx[1]], (idx[0] % (2 * N)) // 2)
    else:
        name = "Hz[%s] (vertex job %d)" % (vert(idx[0]), (idx[0] % (2 * N)) // 2)
    g = float(np.asarray(got)[idx])
    if s is None:
        return "%s %s: %r where the pattern has no entry" % (case["name"], name, g)
    return "%s %s: device %r exact %r error %.3e bound %.3e n %d M %.6e" % (
        case["name"], name, g, float(s.S), float(abs(Fraction(g) - s.S)) if math.isfinite(g) else float("nan"),
        float(s.bound()), s.n, float(s.M))


# ---- the case table ---------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, p, t, tex, X, y_im, flow, y_m, eps=(1e-3, 1.0, 1.0), masked=False, note="", delta=mc.DELTA):
    """flow: the raw observed flow; masked: the operators get MaskedFlow(flow, y_m), i.e. the reference works on
    ekf_ref.mask_flow(flow, y_m)"""
    tex = np.asarray(tex, np.uint8)
    return dict(name=name, p=np.asarray(p, np.float64), t=np.asarray(t, np.int64), tex=tex, H=tex.shape[0], W=tex.shape[1],
                X=np.asarray(X, np.float64).reshape(-1), y_im=np.asarray(y_im, np.uint8), flow=np.asarray(flow, np.float32),
                y_m=np.asarray(y_m, np.uint8), eps=tuple(eps), masked=masked, note=note, delta=float(delta))


def golden_case(eps=(1e-3, 1.0, 1.0), name="golden"):
    g = np.load(os.path.join(GOLD, "measure_64.npz"))
    c = _case(name, g["p"], g["t"], g["tex"], g["X"], g["y_im"], g["flow"], g["y_m"], eps,
              note="tests/golden/measure_64.npz (N = 18, 64 x 64)")
    if tuple(eps) == (1e-3, 1.0, 1.0):
        c["oracle"] = (g["Hz"].reshape(-1), g["Hzc"], g["HTH"])
    return c


def _moved_observation(name, p, t, tex, shift, noise=0.05):
    """the oracle's render of the mesh moved by `shift` px with a velocity of 0.5, noise on the flow (the observation of
    tests/test_measure_limits_gpu.py)"""
    N = len(p)
    H, W = tex.shape
    Xo = np.concatenate(((np.asarray(p) + shift).reshape(-1), np.full(2 * N, 0.5)))
    y_im, fx, fy, ym = ekf_ref.render(Xo, N, t, p, tex, W, H)
    flow = (np.dstack((fx, -fy)) + _rng("obs:" + name).normal(0, noise, (H, W, 2))).astype(np.float32)
    return y_im, flow, (ym // 255).astype(np.uint8)


def limits_case(c, note):
    """a case of tests/measure_cases.py at its rest state"""
    m = c["mesh"]
    obs = _moved_observation(c["name"], m.p, m.t, c["tex"], [1.5, -1.0])
    return _case(c["name"], m.p, m.t, c["tex"], c["states"]["rest"], *obs, note=note)


def _disk(n, h0, seed):
    from hydra_mi import mesh, synth
    dm = mesh.disk_mesh((n - 1) / 2.0, (n - 1) / 2.0, 0.31 * n, h0)
    return dm, synth.noise_texture(n, seed + 2).astype(np.uint8)


def _disk_state(dm, rng, pos_sigma=0.7, vel_sigma=1.0):
    N = dm.size()
    return np.concatenate((dm.p.reshape(-1) + rng.normal(0, pos_sigma, 2 * N), rng.normal(0, vel_sigma, 2 * N)))


def _disk_observation(dm, tex, rng, n):
    """the observation of tests/test_ekf_gpu.py: the mesh moved by 1.5 px both ways"""
    N = dm.size()
    Xo = np.concatenate((dm.p.reshape(-1) + 1.5, np.full(2 * N, 0.5)))
    y_im, fx, fy, ym = ekf_ref.render(Xo, N, dm.t, dm.p, tex, n, n)
    flow = (np.dstack((fx, -fy)) + rng.normal(0, 0.05, (n, n, 2))).astype(np.float32)
    return y_im, flow, (ym // 255).astype(np.uint8)


def edge_case(kind):
    """the `outside` and `blank` cases of test_ekf_gpu.test_measure_edge_cases_match_oracle (same seeds, same draws)"""
    n = 48
    dm, tex = _disk(n, 10.0, 14)
    rng = np.random.default_rng(17)
    X = _disk_state(dm, rng, pos_sigma=0.5)
    if kind == "outside":
        X[0:2 * dm.size():2] -= 0.45 * n
        X[1:2 * dm.size():2] += 0.30 * n
    y_im, flow, y_m = _disk_observation(dm, tex, rng, n)
    if kind == "blank":
        y_im, y_m, flow = np.zeros_like(y_im), np.zeros_like(y_m), np.zeros_like(flow)
    return _case(kind, dm.p, dm.t, tex, X, y_im, flow, y_m,
                 note={"outside": "a third of the mesh outside the frame", "blank": "empty observation"}[kind])


def masked_case():
    """test_ekf_gpu.test_masked_flow_path: non-zero flow outside the mask, multiplied away on the device (k_mask_flow)"""
    n = 64
    dm, tex = _disk(n, 11.0, 0)
    rng = np.random.default_rng(9)
    X = _disk_state(dm, rng)
    y_im, flow, y_m = _disk_observation(dm, tex, rng, n)
    return _case("masked_flow", dm.p, dm.t, tex, X, y_im, flow + np.float32(0.3), y_m, masked=True,
                 note="MaskedFlow, flow + 0.3 outside the mask")


def pool_case():
    """the 48^2 / h0 = 3.0 mesh, state and observation of test_ekf_gpu.test_dense_mesh_grows_the_difference_image_pool: on
    a fresh context the measurement checked is the one that finds the pool too small and grows it (pool_demand).
    With delta = 2 a vertex of this mesh crosses its neighbours' edges and three triangles meet over some pixels of a
    perturbed configuration, whatever the state (also at rest): the precondition fails, and the device's difference
    images do differ from the full renders' in two flow values.  delta = 1.5 keeps it to two triangles and still asks
    for 22 848 pixels against the pool's 18 432."""
    n = 48
    dm, tex = _disk(n, 3.0, 6)
    rng = np.random.default_rng(21)
    X = _disk_state(dm, rng, pos_sigma=0.2)
    y_im, flow, y_m = _disk_observation(dm, tex, rng, n)
    return _case("pool_growth", dm.p, dm.t, tex, X, y_im, flow, y_m, note="106 vertices on 48 x 48, delta 1.5: the pool grows",
                 delta=1.5)


def pool_demand(case):
    """-> (pixels of all star regions as k_star_regions pads them, pixels of a fresh context's pool: 8 frames)"""
    N = len(case["p"])
    area = sum(int(np.prod(mc.star_region(case["X"], N, case["t"], v, case["W"], case["H"], case["delta"])[2:])) for v in range(N))
    return area, 8 * case["W"] * case["H"]


def odd_frame_case():
    """a 75 x 53 frame (neither a multiple of 8): a wheel of 7 whose outer ring ends 2 px above the frame's last row, so
    that the last tile row of its star regions leaves the frame"""
    p, t = mc.wheel_mesh(7, (37.3, 26.6), 12.0, R2=24.0)
    c = mc.case("odd_frame", p, t, 75, 53, hub=0)
    return limits_case(c, "75 x 53 frame, star regions padded past its last row")


def three_scales_case():
    return golden_case((1e-3, 1.0, 1e3), "three_scales")


def _limits(name):
    if name in ("region_above", "region_clipped"):
        return {c["name"]: c for c in mc.coarse_cases()}[name]
    return {c["name"]: c for c in mc.hub_cases() + [mc.border_fan_case()]}[name]


LIMIT_NOTES = {"hub7": "odd star count", "hub13": "odd star count", "hub24": "all 24 bits of a tile word",
               "fan24": "104 terms of a k_solve_prep row", "region_above": "no tile list: per-triangle boxes",
               "region_clipped": "region padding leaves the frame"}
CASES = ("golden", "hub7", "hub13", "hub24", "fan24", "region_above", "region_clipped", "outside", "blank", "masked_flow",
         "pool_growth", "three_scales", "odd_frame")
SPLIT_CASES = ("golden", "hub24")
MEASURE_SPLITS = (1, 2, 7, 16)
EDGE_SPLITS = (1, 3, 16)


def make_case(name):
    if name == "golden":
        return golden_case()
    if name in LIMIT_NOTES:
        return limits_case(_limits(name), LIMIT_NOTES[name])
    if name in ("outside", "blank"):
        return edge_case(name)
    return {"masked_flow": masked_case, "pool_growth": pool_case, "three_scales": three_scales_case,
            "odd_frame": odd_frame_case}[name]()


def passed_flow(case):
    """the flow the reference works on"""
    return ekf_ref.mask_flow(case["flow"], case["y_m"]) if case["masked"] else case["flow"]


_exact_cache = {}


def exact_of(case, keep_terms=False):
    """the Exact of a case and its measure(), computed once per process and left unchanged"""
    key = (case["name"], keep_terms)
    if key not in _exact_cache:
        ex = Exact(case["p"], case["t"], case["tex"], case["X"], case["y_im"], passed_flow(case), case["y_m"], case["eps"],
                   case["delta"], keep_terms)
        _exact_cache[key] = (ex, ex.measure())
    return _exact_cache[key]


def exact_measure(case):
    """-> Hz [4N], Hzc [4N, 4], HTH [4N, 4N] of Sums (exact value S, mass M, count n each); None in HTH off the pattern"""
    return exact_of(case)[1]


def oracle_measure(case):
    """the binary64 oracle (the C twin of ekf_ref) -> Hz [4N], Hzc [4N, 4], HTH [4N, 4N]"""
    N = len(case["p"])
    cm = ekf_c.Measurement(N, case["t"], case["p"], case["tex"], *case["eps"], threads=min(16, os.cpu_count() or 1))
    Hz, Hzc = cm.jacobian_all(case["X"], case["y_im"], passed_flow(case), case["y_m"], case["delta"])
    _, J = ekf_ref.adjacency(N, case["t"])
    return Hz.reshape(-1), Hzc, cm.hessian_all(case["X"], J, case["delta"])


def pattern(case):
    return ekf_ref.adjacency(len(case["p"]), case["t"])[1] == 1


def old_bar_worse_than(arr, rel=1e-6, old=1e-9):
    """how many non-zero entries of `arr` the bar `old` x max|arr| holds to worse than `rel` relative"""
    a = np.abs(np.asarray(arr, np.float64))
    return int(np.count_nonzero((a > 0) & (old * a.max() > rel * a)))


# ---- the device ------------------------------------------------------------------------------------------------------
class St:
    def __init__(self, X):
        self.X = np.asarray(X, np.float64).reshape(-1, 1)


def device_renderer(case):
    """a fresh context for the case, the observation in place"""
    from hydra_mi import mesh, renderer
    N = len(case["p"])
    R = renderer.Renderer(mesh.Mesh(case["p"], case["t"]), np.zeros((N, 2)), np.zeros((case["H"], case["W"], 2), np.float32),
                          case["H"], case["tex"], True, *case["eps"])
    R.update_frame(case["y_im"], case["flow"], case["y_m"])
    return R


def device_flow(case):
    from hydra_mi.renderer import MaskedFlow
    return MaskedFlow(case["flow"], case["y_m"]) if case["masked"] else case["flow"]


def device_measure(case, tunes=None, R=None):
    """Renderer.measure of the case -> Hz [4N], Hzc [4N, 4], HTH [4N, 4N]"""
    own = R is None
    if own:
        R = device_renderer(case)
    try:
        for k, v in (tunes or {}).items():
            R.tune(k, v)
        Hz, HTH, Hzc = R.measure(St(case["X"]), case["y_im"], device_flow(case), case["y_m"], case["delta"])
    finally:
        if own:
            R.close()
    return Hz.reshape(-1), Hzc, HTH


def check_measure(case, got, sums):
    """-> ({array: largest error / bound}, [per-entry reports of everything out of bounds]); the arrays: Hz, the four
    channels of Hzc, the self blocks and the edge blocks of HTH"""
    Hz, Hzc, HTH = got
    eHz, eHzc, eHTH = sums
    N = len(case["p"])
    out, reports = {}, []
    w, bad = ratios(Hz, eHz)
    out["Hz"] = w
    reports += [describe(case, "Hz", i, Hz, eHz) for i in bad]
    for ch in range(4):
        w, bad = ratios(Hzc[:, ch], eHzc[:, ch])
        out["Hzc " + CHANNELS[ch]] = w
        reports += [describe(case, "Hzc", (i[0], ch), Hzc, eHzc) for i in bad]
    vert = (np.arange(4 * N) % (2 * N)) // 2
    own = vert[:, None] == vert[None, :]
    worst = {"HTH self": 0.0, "HTH edge": 0.0}
    for idx in np.ndindex(HTH.shape):
        s = eHTH[idx]
        if s is None:
            continue                                              # off the pattern: the caller asserts the zeros at once
        r, bad = ratio_one(HTH[idx], s)
        key = "HTH self" if own[idx] else "HTH edge"
        worst[key] = max(worst[key], r)
        if bad:
            reports.append(describe(case, "HTH", idx, HTH, eHTH))
    out.update(worst)
    return out, reports
