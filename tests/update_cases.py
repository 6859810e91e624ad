"""Cases that send the iterated update (hm_update_run, reference kalman.py:774-831) through each of its four doors on
purpose, shared by the CPU test (the cases hold what their names promise, for the oracle alone), the GPU test (the
device against the oracle) and tools/make_update_golden.py (the oracle's results, tests/golden/update_paths.npz).

    door            state kept        covariance kept
    revert_first    the prior mean    the prior                          a triangle flips in round 1
    revert_later    iterate k-1       inv(inv(W) + HTH) of round k-1     a triangle flips in round k > 1
    converge        iterate k         of round k                         |e_new - e_old| / e_new < reltol in round k
    limit           iterate max_iter  of round max_iter                  max_iter reached

How a fold is provoked: one interior vertex of the mesh is moved along the line from its rest position to the midpoint
of the opposite edge of one of its triangles (position s on that line: 1 = rest, 0 = on the edge, < 0 = folded).  The
prior mean has it at a small positive s (a sliver triangle), the observation is rendered from the state with it at
s < 0, and a vague prior lets the update follow the observation across the edge.

reltol is chosen per case from the oracle's own sequence of convergence figures (the geometric mean of the figure of
the round meant to stop and the smallest figure before it), never the other way round; max_iter, the prior and the
sliver parameters are what selects the door.

Every case is a dict: name, door, round (the round that ends the loop), mesh, n (frame side), tex, eps (eps_Z, eps_J,
eps_M), X0 (4N), W (4N x 4N), y_im, flow (the raw observed flow), y_m, masked (the update takes MaskedFlow(flow, y_m),
the error sums of hm_update_last_error the raw flow), max_iter, reltol, deltaX, second (y_im, flow, y_m, max_iter,
reltol of another frame, for an update that follows on the same handle)."""
import zlib

import numpy as np

from hydra_mi import mesh
from oracle import ekf_ref

DELTA = 2.0
EPS = (1e-3, 1.0, 1.0)
GOLDEN = "update_paths.npz"

# decision margins the CPU test holds every case to (device iterates agree with the oracle's to ~1e-9)
AREA_MARGIN = 1e-3          # px^2, signed doubled area of every triangle of an accepted / of the flipped iterate
SNAP_MARGIN = 1e-6          # px, distance of every vertex coordinate from a boundary of the rasteriser's snap grid


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def texture(name, n):
    """smooth noise (a few pixels of correlation, so that the image term has a gradient), seeded by the case name"""
    from scipy import ndimage
    t = ndimage.gaussian_filter(_rng("tex:" + name).normal(size=(n, n)), 2.0)
    t = (t - t.min()) / (t.max() - t.min())
    return np.rint(30 + 200 * t).astype(np.uint8)


def oriented(m):
    """one orientation at rest (positive doubled area), as the filter's fold test expects"""
    p, t = m.p, m.t.copy()
    a = doubled_areas(p.reshape(-1), t)
    t[a < 0] = t[a < 0][:, [0, 2, 1]]
    return mesh.Mesh(p, t, m.h0)


def doubled_areas(P, tri):
    """signed doubled area of every triangle with the vertices at P (2N): the quantity whose sign update_orientation
    takes (kalman.py:410-414)"""
    ver = np.asarray(P, np.float64).reshape(-1, 2)
    a = ver[tri[:, 1]] - ver[tri[:, 0]]
    b = ver[tri[:, 2]] - ver[tri[:, 0]]
    return a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]


def state_areas(X, N, tri):
    return doubled_areas(np.asarray(X, np.float64).reshape(-1)[:2 * N], tri)


def snap_distance(X, N, deltaX=DELTA):
    """smallest distance (px) of a vertex coordinate of X, or of its +-deltaX perturbed positions, from a boundary of
    the snap grid: ekf_ref.snap rounds x * SUB to the nearest integer, the boundaries are at (k + 1/2) / SUB"""
    x = np.asarray(X, np.float64).reshape(-1)[:2 * N]
    d = np.inf
    for s in (0.0, deltaX, -deltaX):
        g = (x + s) * ekf_ref.SUB
        d = min(d, float(np.abs(g - np.floor(g) - 0.5).min()) / ekf_ref.SUB)
    return d


def hub_sliver(m):
    """The interior vertex of highest degree, one of its triangles and the midpoint of that triangle's opposite edge ->
    (v, rest position, midpoint).  The triangle: the first of the vertex's star in mesh order."""
    t = m.t
    border = set()
    edges = {}
    for tr in t:
        for a, b in ((tr[0], tr[1]), (tr[1], tr[2]), (tr[2], tr[0])):
            k = (min(a, b), max(a, b))
            edges[k] = edges.get(k, 0) + 1
    for (a, b), c in edges.items():
        if c == 1:
            border |= {a, b}
    deg = np.bincount(t.reshape(-1), minlength=m.size())
    cand = [v for v in range(m.size()) if v not in border]
    v = max(cand, key=lambda q: (deg[q], -q))
    tr = t[np.nonzero((t == v).any(axis=1))[0][0]]
    a, b = [q for q in tr if q != v]
    return int(v), m.p[v].copy(), (m.p[a] + m.p[b]) / 2.0


def sliver_state(m, s, vel=None):
    """rest positions with the hub vertex at position s of its sliver line; zero velocities unless given"""
    v, rest, mid = hub_sliver(m)
    P = m.p.copy()
    P[v] = mid + s * (rest - mid)
    V = np.zeros_like(P) if vel is None else np.asarray(vel, np.float64).reshape(P.shape)
    return np.concatenate((P.reshape(-1), V.reshape(-1)))


def observe(name, meas, Xobs, n, noise=0.05):
    """the observation a tracker would see of the mesh at Xobs: its render, its flow planes plus noise, its mask"""
    y_im, yfx, yfy, ym = meas.render(Xobs)
    y_m = (ym // 255).astype(np.uint8)
    flow = (np.dstack((yfx, -yfy)) + _rng("obs:" + name).normal(0, noise, (n, n, 2))).astype(np.float32)
    return y_im, flow, y_m


def measurement(case, cls=None):
    m = case["mesh"]
    return (cls or ekf_ref.Measurement)(m.size(), m.t, m.p, case["tex"], *case["eps"])


def _case(name, door, rnd, m, n, X0, Wdiag, Xobs, max_iter, reltol, masked=False, outside_flow=0.0, tex=None):
    N = m.size()
    tex = texture(tex or name, n)
    c = dict(name=name, door=door, round=rnd, mesh=m, n=n, tex=tex, eps=EPS, X0=np.asarray(X0, np.float64),
             W=np.diag(np.broadcast_to(np.asarray(Wdiag, np.float64), (4 * N,))).copy(), masked=masked,
             max_iter=max_iter, reltol=reltol, deltaX=DELTA)
    y_im, flow, y_m = observe(name, measurement(c), Xobs, n)
    if outside_flow:
        # a flow that does not vanish outside the object: the update must not see it (kalman.py:679-687), error() does (:700)
        flow = flow.copy()
        flow[y_m == 0] += np.float32(outside_flow)
    c.update(y_im=y_im, flow=flow, y_m=y_m)
    # a second, ordinary frame for the same handle: the mesh near rest, slightly moved
    c["second"] = observe(name + ":2", measurement(c), moved(m, (0.5, -0.5), (0.2, 0.1)), n) + (3, 1e-4)
    return c


def disk64():
    """the 64 px disk of the measurement tests: N = 18, 4N = 72 = 2 * 32 + 8 (three block columns, the last one partial)"""
    return oriented(mesh.disk_mesh(31.5, 31.5, 0.31 * 64, 11.0))


def square32():
    """4 vertices, 4N = 16: the whole system inside one 32-column block"""
    return oriented(mesh.square4_mesh(8, 24))


def moved(m, shift, vel, scale=1.0):
    """the rest mesh scaled about its centroid, shifted, every vertex with velocity vel"""
    c = m.p.mean(axis=0)
    P = c + scale * (m.p - c) + np.asarray(shift, np.float64)
    V = np.broadcast_to(np.asarray(vel, np.float64), P.shape)
    return np.concatenate((P.reshape(-1), V.reshape(-1)))


def rest(m):
    return np.concatenate((m.p.reshape(-1), np.zeros(2 * m.size())))


# name -> (door, round, builder); the parameters were found with the oracle (tools/make_update_golden.py --explore prints
# the sequence of convergence figures and the smallest areas of a case) and are held by tests/test_update_cases_cpu.py
def build(name):
    d = disk64()
    if name == "revert_first":
        return _case(name, "revert_first", 1, d, 64, sliver_state(d, 0.06), 100.0, sliver_state(d, -0.35), 10, 1e-4)
    if name == "revert_later":
        return _case(name, "revert_later", REVERT_LATER_ROUND, d, 64, sliver_state(d, REVERT_LATER_S), REVERT_LATER_W,
                     sliver_state(d, -0.35), 10, 1e-4, tex="revert_first")
    if name == "revert_later_6":
        return _case(name, "revert_later", 6, d, 64, sliver_state(d, 0.5), 100.0, sliver_state(d, -0.35), 10, 1e-4,
                     tex="revert_first")
    if name == "converge_early":
        return _case(name, "converge", CONVERGE_ROUND, d, 64, rest(d), 1.0, moved(d, (1.5, 1.5), (0.5, 0.5)), 10,
                     CONVERGE_RELTOL)
    if name == "limit":
        return _case(name, "limit", 4, d, 64, rest(d), 1.0, moved(d, (1.5, 1.5), (0.5, 0.5)), 4, LIMIT_RELTOL,
                     tex="converge_early")
    if name == "limit_1":
        return _case(name, "limit", 1, d, 64, rest(d), 10.0, moved(d, (1.0, -1.0), (0.3, -0.2)), 1, 1e-4)
    if name == "masked":
        return _case(name, "converge", MASKED_ROUND, d, 64, rest(d), 1.0, moved(d, (-1.0, 1.5), (-0.4, 0.6)), 10,
                     MASKED_RELTOL, masked=True, outside_flow=0.75)
    if name == "small":
        s = square32()
        return _case(name, "limit", 3, s, 32, rest(s), 1.0, moved(s, (1.0, 0.5), (0.4, 0.2)), 3, SMALL_RELTOL)
    raise KeyError(name)


# figures chosen from the oracle's sequences (see build)
# (revert_later: with the sliver at 0.15 the first round is accepted with a smallest doubled area of 10.5 px^2 and the
# second folds it to -25 px^2; at 0.5 five rounds are accepted, figures 1, .18, .0063, .029, .069, before the fold)
REVERT_LATER_S, REVERT_LATER_W, REVERT_LATER_ROUND = 0.15, 100.0, 2
# converge_early: figures 1, .469, .312, .0963, .1226, .0187: round 6 stops at sqrt(.0187 * .0963)
CONVERGE_ROUND, CONVERGE_RELTOL = 6, 0.0424
LIMIT_RELTOL = 1e-4
# masked: figures 1, .551, .602, .686, .0973, .00188: round 6 stops at sqrt(.00188 * .0973)
MASKED_ROUND, MASKED_RELTOL = 6, 0.0135
SMALL_RELTOL = 1e-6

NAMES = ("revert_first", "revert_later", "revert_later_6", "converge_early", "limit", "limit_1", "masked", "small")


def update_flow(case):
    """the flow the update's residuals use"""
    return ekf_ref.mask_flow(case["flow"], case["y_m"]) if case["masked"] else case["flow"]


def run_oracle(case, cls=None, max_iter=None):
    """oracle/ekf_ref.iekf_update of the case -> dict of arrays, the layout of the golden file (one entry per key under
    '<name>/').  cls: the Measurement class (ekf_ref.Measurement, or its C twin oracle.ekf_c.Measurement)."""
    m = case["mesh"]
    N = m.size()
    meas = measurement(case, cls)
    _, J = ekf_ref.adjacency(N, m.t)
    fm = update_flow(case)
    hist = []
    nI = case["max_iter"] if max_iter is None else max_iter
    X, W, niter, trace = ekf_ref.iekf_update(meas, case["X0"], case["W"], J, m.t, case["y_im"], fm, case["y_m"], nI=nI,
                                             reltol=case["reltol"], deltaX=case["deltaX"], history=hist)
    reverted = len(trace) > 0 and trace[-1] == ("reverted",)
    accepted = niter - (1 if reverted else 0)
    ratios = np.array([h["ratio"] for h in hist[:accepted]])
    converged = (not reverted) and accepted > 0 and ratios[-1] < case["reltol"]
    if reverted:
        door = "revert_first" if accepted == 0 else "revert_later"
    else:
        door = "converge" if converged else "limit"
    Hzc = hist[-1]["Hzc"]
    gains = np.vstack((W @ Hzc[:, 0], W @ (Hzc[:, 1] + Hzc[:, 2]), W @ Hzc[:, 3]))
    out = dict(door=np.array(door), info=np.array([niter, accepted, int(reverted), int(converged)], np.int64),
               errs=np.array([list(map(float, t)) for t in trace[:accepted]], np.float64).reshape(accepted, 4),
               ratios=ratios, iterates=np.array([h["X"] for h in hist]), X_meas_last=hist[-1]["X_meas"],
               X_kept=np.asarray(X, np.float64).reshape(-1).copy(), W_kept=np.array(W), Hzc_last=Hzc, gains=gains,
               cond_prior=np.array(np.linalg.cond(case["W"])), cond_A=np.array([np.linalg.cond(h["A"]) for h in hist]),
               min_eig_A=np.array([np.linalg.eigvalsh(h["A"]).min() for h in hist]),
               min_area=np.array([state_areas(h["X"], N, m.t).min() for h in hist]),
               snap_distance=np.array([snap_distance(h["X"], N, case["deltaX"]) for h in [dict(X=case["X0"])] + hist]))
    if not reverted:
        # Renderer.error of the state kept against the observation as given (the raw flow), kalman.py:700
        e = meas.error(out["X_kept"], case["y_im"], case["flow"], case["y_m"])
        out["last_error"] = np.array([float(e[0]), e[1], e[2], float(e[3])])
    return out


def load_golden(path):
    """-> name -> dict, from the file tools/make_update_golden.py writes"""
    z = np.load(path)
    out = {}
    for k in z.files:
        name, key = k.split("/", 1)
        out.setdefault(name, {})[key] = z[k]
    return out
