"""Extended / iterated Kalman filter of the mesh tracker -- the reference's filter API.

Drop-in for the classes of reference kalman.py on the hot path: ``KFState``
(:106-624), ``KalmanFilter`` (:626-765), ``IteratedKalmanFilter`` (:767-831),
``IteratedMSKalmanFilter`` (:834-960) and the module-level ``stats`` (:25-104).
Constructor arguments, defaults, method names, the state layout
``X = [x0,y0,...,vx0,vy0,...]`` (:178) and the return value of ``compute`` are the
reference's.  What changes is where the work is done:

* ``KFState.update`` (:437-449) is one call into libhydra_mi.so
  (``Renderer.measure`` -> ``hm_measure``): the mesh is rasterised and every
  finite-difference perturbation of kalman.py:491-518 / :583-606 is evaluated and
  reduced on the GPU, inside the bounding box of the triangles it moves.  The
  result has the single-perturbation semantics of the reference
  (``multi=False``); ``multi=True`` -- the reference's way of batching several
  perturbations into one render -- is accepted and gives the same numbers.
* the dense algebra of the update runs on the device (``hm_update_run`` /
  ``hm_update_begin`` / ``_step`` / ``_cov``): one blocked Cholesky factorisation per IEKF
  iteration on the f64 matrix cores instead of an explicit inverse per iteration; the
  covariance is formed once, for the state that is kept, and stays on the device between
  predict and update.  Same mathematics, rounding-level differences.
* the mass-spring predict is native code (``hm_ms_newton``: block-eliminated Newton, the spring
  operator applied bar by bar), the covariance prediction a device kernel (``hm_cov_predict``).

There is no CPU measurement path: ``cuda=False`` raises.

The filters take every step through one object, ``state.algebra``, decided once in the constructor of ``KFState``:
the native ``Renderer`` itself, or -- when a caller supplies its own measurement object (``renderer=``, an object with
``measure`` and ``error``; the CPU tests of the host logic do) -- a ``kalman_host.HostAlgebra`` around it, which offers
the same step-wise verbs in NumPy / SciPy.  What only the native path has (the fused run, the arming calls, the worker
on the device, the chain) is asked for with ``state.native``.  The mass-spring filter's state prediction started ahead
of the frame that needs it has one owner, ``PredictionAhead``.
"""
import contextlib
import ctypes
import sys
import time

import numpy as np
import scipy.sparse as sp

from . import _lib
from .kalman_host import HostAlgebra, _mask_distance  # noqa: F401 -- (_mask_distance: read from here by the host tests)
from .renderer import ChainedPredictionFailed, DeviceCovariance, Renderer, MaskedFlow, DeviceObservation


class Statistics:
    """reference kalman.py:25-62: counters the timing study reads (timing_synthetic.py:60-90)."""

    _scalars = ("niter", "meshpts", "gridsize", "jacobianpartitions", "hessianpartitions", "nzj")
    _lists = dict(jacobianrenderstc=2, hessianrenderstc=2, renders=1, statepredtime=1, stateupdatetc=2,
                  hessinc=1, jacinc=1, hessincsparse=1)

    def __init__(self):
        for k in self._scalars:
            setattr(self, k, 0)
        for k, n in self._lists.items():
            setattr(self, k, [0] * n)

    def reset(self):
        for k in self._scalars:
            setattr(self, k, 0)
        for k, n in self._lists.items():
            getattr(self, k)[:] = [0] * n


stats = Statistics()


def _log(msg):
    sys.stdout.write(msg + "\n")


class KFState:
    _ori_stale = False

    def __init__(self, distmesh, im, flow, cuda, eps_F=1, eps_Z=1e-3, eps_J=1e-3, eps_M=1e-3, vel=None,
                 sparse=True, multi=True, verbose=False, renderer=None, device=0):
        self.multi = multi
        self.sparse = sparse
        self.verbose = verbose
        self._ver = np.array(distmesh.p, np.float32)
        self._vel = np.zeros(self._ver.shape, np.float32) if vel is None else np.asarray(vel).reshape(self._ver.shape)
        self.tex = im
        self.nx, self.ny = im.shape[0], im.shape[1]
        self.M = self.nx * self.ny
        self.NZ = self.M
        self.eps_F, self.eps_Z, self.eps_J, self.eps_M = eps_F, eps_Z, eps_J, eps_M
        self.N = distmesh.size()
        self.u = self._ver

        # orientation of the faces and removal of slivers, |sin(angle at vertex 0)| <= 0.06 (:148-161)
        tri = np.asarray(distmesh.t)
        a = self._ver[tri[:, 1]] - self._ver[tri[:, 0]]
        b = self._ver[tri[:, 2]] - self._ver[tri[:, 0]]
        cr = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        sine = cr / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        keep = np.abs(sine) > 0.06
        if verbose:
            _log("Removing %d faces for being too flat" % int(np.sum(~keep)))
        self.sineface = sine[keep]
        self.ori = np.sign(cr)[keep]
        self.tri = tri[keep]
        distmesh.t = self.tri
        self.NT = self.tri.shape[0]

        # bars that no remaining face uses are dropped (:163-175)
        t = self.tri
        allbars = np.vstack((t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]))
        allbars = np.unique(np.sort(allbars, axis=1), axis=0)
        have = set(map(tuple, allbars))
        sel = np.array([tuple(bar) in have for bar in np.asarray(distmesh.bars)], bool)
        distmesh.bars = np.asarray(distmesh.bars)[sel]
        distmesh.L = np.asarray(distmesh.L)[sel]

        # state, transition and covariances (:178-186)
        N = self.N
        self.X = np.vstack((self._ver.reshape(-1, 1), self._vel.reshape(-1, 1))).astype(np.float64)
        e = np.eye(2 * N)
        z = np.zeros((2 * N, 2 * N))
        self.F = np.block([[e, e], [z, e]])
        self.Weps = eps_F * np.block([[e / 4, e / 2], [e / 2, e]])
        self.W = np.block([[1e-2 * e, z], [z, e]])

        # vertex adjacency and the sparsity pattern of HTH (:189-205)
        Jv = np.eye(N)
        for k in range(3):
            for l in range(3):
                Jv[t[:, k], t[:, l]] = 1
        self.Jv = Jv
        self.J = np.kron(np.ones((2, 2)), np.kron(Jv, np.ones((2, 2))))

        # spring incidence and rest lengths (:206-218)
        bars = distmesh.bars
        self.I = bars.shape[0]
        Kp = np.zeros((N, self.I))
        Kp[bars[:, 0], np.arange(self.I)] = 1
        Kp[bars[:, 1], np.arange(self.I)] = -1
        self.Kp = Kp
        self.K = np.kron(Kp, np.eye(2))
        self.Ks = sp.csr_matrix(self.K)
        self.l0 = self.lengths()
        self.L = self.lengths()

        # perturbation partitions of the reference's multi-render scheme (:223-389); kept as
        # attributes for API compatibility, the native path does not need them
        self.E, self.labels = self._vertex_partitions()
        self.Q, self.E_hessian, self.E_hessian_idx, self.labels_hess = self._pair_partitions()

        # `renderer` lets a caller supply the measurement object (tests of the host logic do);
        # by default it is the HIP one -- there is no CPU implementation in this package
        self.renderer = renderer if renderer is not None else Renderer(
            distmesh, self._vel, flow, self.nx, im, cuda, eps_Z, eps_J, eps_M, self.labels, self.labels_hess,
            self.Q, showtracking=False, device=device)
        # the filters' steps go through `algebra`: the native renderer itself, or the host algebra around a measurement
        # object that only offers measure / error; `native` stands for what only the former has (the fused run, the
        # arming calls, the worker on the device, the chain)
        self.native = isinstance(self.renderer, Renderer)
        self.algebra = self.renderer if self.native else HostAlgebra(self.renderer)
        self.host_cap = contextlib.nullcontext if self.native else self.algebra.blas_cap

        stats.meshpts = self.N
        stats.gridsize = getattr(distmesh, "h0", 0)
        stats.nzj = np.sum(self.J) / 2 + (self.N * 4) / 2
        stats.hessinc[0] = 2 + (stats.meshpts * 4) * (stats.meshpts * 4)
        stats.jacinc[0] = 2 + stats.meshpts * 4 * 2
        stats.hessincsparse[0] = 2 + stats.nzj * 2
        stats.jacobianpartitions = len(self.E)
        stats.hessianpartitions = len(self.E_hessian)

    # -- partitions ---------------------------------------------------------------------------
    def _vertex_partitions(self):
        """Greedy classes of mutually non-adjacent vertices (:223-255) and, per class, the vertex
        each triangle is attributed to, -1 if none (:263-272)."""
        nbr = [set(np.nonzero(self.Jv[q])[0]) - {q} for q in range(self.N)]
        free = set(range(self.N))
        queue = list(range(self.N))
        classes = []
        while queue:
            later = set()
            members = []
            while queue:
                q = queue[0]
                members.append(q)
                later = (later | nbr[q]) & free
                free.discard(q)
                queue = [x for x in queue if x != q and x not in nbr[q]]
            queue = sorted(later)
            classes.append(members)
        labels = -np.ones((len(self.tri), len(classes)))
        for k, members in enumerate(classes):
            for node in members:                       # later members overwrite earlier ones, as in the reference
                labels[np.any(self.tri == node, axis=1), k] = node
        return classes, labels

    def _pair_partitions(self):
        """Same idea for the vertex pairs Q = {(i,j): i<=j adjacent} of the sparse Hessian (:305-389)."""
        N = self.N
        Q = np.array([[i, j] for i in range(N) for j in range(i, N) if self.Jv[i, j]])
        nbr = [set(np.nonzero(self.Jv[q])[0]) for q in range(N)]
        diag = {int(q[0]): k for k, q in enumerate(Q) if q[0] == q[1]}
        free = set(range(len(Q)))
        queue = list(range(len(Q)))
        classes, classes_idx = [], []
        while queue:
            later = set()
            members = []
            while queue:
                qi = queue[0]
                a, b = int(Q[qi][0]), int(Q[qi][1])
                near = (nbr[a] | nbr[b]) - {a, b}
                clash = {k for k in queue if int(Q[k][0]) in near or int(Q[k][1]) in near}
                clash |= {diag[a], diag[b]} & set(queue)
                members.append(qi)
                # the reference intersects its "do later" set with the pairs not yet placed BEFORE it
                # marks the current one as placed (:341-344), and a diagonal pair clashes with itself
                # (p_self1 / p_self2, :331-332): (i,i) is scheduled once more and lands in a second
                # class -- kept, the lists must equal the reference's
                later = (later | clash) & free
                free.discard(qi)
                queue = [k for k in queue if k != qi and k not in clash]
            queue = sorted(later)
            idx = np.array(sorted(members), float)
            classes_idx.append(idx)
            classes.append(Q[idx.astype(int)].reshape(-1, 2))
        labels = -np.ones((len(self.tri), len(classes)))
        for k, pairs in enumerate(classes):
            for i, (n1, n2) in enumerate(pairs):
                hit = np.any(self.tri == n1, axis=1) | np.any(self.tri == n2, axis=1)
                labels[hit, k] = classes_idx[k][i]
        return Q, classes, classes_idx, labels

    # -- geometry -------------------------------------------------------------------------------
    def vertices(self):
        return self.X[0:2 * self.N].reshape((-1, 2))

    def velocities(self):
        return self.X[2 * self.N:].reshape((-1, 2))

    def lengths(self):
        d = self.Ks.T.dot(self.vertices().reshape(-1, 1)).reshape(-1, 2)
        return np.sqrt((d * d).sum(axis=1)).reshape(-1, 1)

    # The covariance may live on the device between the calls of a filter step (renderer.DeviceCovariance);
    # reading state.W brings it to the host once, assigning replaces it.
    @property
    def W(self):
        if isinstance(self._W, DeviceCovariance):
            self._W = self._W.fetch()
        return self._W

    @W.setter
    def W(self, value):
        self._W = value

    def update_orientation(self):
        ver = self.vertices()
        a = ver[self.tri[:, 1]] - ver[self.tri[:, 0]]
        b = ver[self.tri[:, 2]] - ver[self.tri[:, 0]]
        cr = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        self.ori = np.sign(cr)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.sineface = cr / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))

    # ori / sineface (:410-414): the fused update tests the orientation of the faces natively (hm_update_run) and only
    # marks these stale; they are formed from the state when somebody looks (eight NumPy passes over the faces, ~50 us of
    # every frame otherwise)
    @property
    def ori(self):
        if self._ori_stale:
            self._ori_stale = False
            self.update_orientation()
        return self._ori

    @ori.setter
    def ori(self, value):
        self._ori, self._ori_stale = value, False

    @property
    def sineface(self):
        if self._ori_stale:
            self._ori_stale = False
            self.update_orientation()
        return self._sineface

    @sineface.setter
    def sineface(self, value):
        self._sineface = value

    def size(self):
        return self.X.shape[0]

    def setforce(self, f):
        self.renderer.force = f

    def get_flow(self):
        return self.renderer.get_flow()

    def refresh(self, multi_idx=-1, hess=False):
        self.renderer.update_vertex_buffer(self.vertices(), self.velocities(), multi_idx, hess)

    def render(self):
        stats.renders[0] += 1
        return self.renderer.render()

    # -- linearisation of the measurement ------------------------------------------------------------
    def update(self, y_im, y_flow, y_m):
        """(Hz, HTH, Hz_components) at the current state -- reference kalman.py:437-449."""
        t0 = time.time()
        Hz, HTH, Hzc = self.renderer.measure(self, y_im, y_flow, y_m)
        dt = time.time() - t0
        stats.stateupdatetc[0] += dt
        stats.stateupdatetc[1] += 1
        self.count_renders(dt)
        return Hz, HTH, Hzc

    def count_renders(self, dt):
        """One call of renderer.measure in the counters: the reference splits this time between its Jacobian and
        Hessian passes; here it is one launch."""
        stats.jacobianrenderstc[0] += dt / 2
        stats.jacobianrenderstc[1] += stats.jacinc[0]
        stats.hessianrenderstc[0] += dt / 2
        stats.hessianrenderstc[1] += stats.hessincsparse[0] if self.sparse else stats.hessinc[0]

    def _jacobian_multi(self, y_im, y_flow, y_m, deltaX=2):
        """reference kalman.py:452-489: the vertices of one partition (mutually non-adjacent, so their stars do
        not overlap) are perturbed in ONE render and the sums are separated by triangle label
        (Renderer.jz_multi -> hm_jz_multi).  8 renders per partition instead of 8 per vertex.  The product's
        update() does not use it (measure() evaluates single perturbations inside their stars); it is the
        reference's operator sequence, kept runnable for the multi == single protocol
        (testbites/test_multipert_validation.py:98-189)."""
        n = self.size()
        Hz = np.zeros((n, 1))
        Hzc = np.zeros((n, 4))
        for idx, e in enumerate(self.E):
            e = np.asarray(e, np.int64)
            self.refresh(idx)
            self.renderer.initjacobian(y_im, y_flow, y_m)
            for i in range(2):
                for j in range(2):
                    ee = i + 2 * self.N * j + 2 * e
                    self.X[ee, 0] += deltaX
                    self.refresh(idx)
                    hz, hzc = self.renderer.jz_multi(self)
                    Hz[ee, 0] = hz[e, 0] / deltaX
                    Hzc[ee, :] = hzc[e, :] / deltaX
                    self.X[ee, 0] -= 2 * deltaX
                    self.refresh(idx)
                    hz, hzc = self.renderer.jz_multi(self)
                    Hz[ee, 0] = Hz[ee, 0] - hz[e, 0] / deltaX
                    Hzc[ee, :] -= hzc[e, :] / deltaX
                    self.X[ee, 0] += deltaX
                    Hz[ee, 0] = Hz[ee, 0] / 2
                    Hzc[ee, :] = Hzc[ee, :] / 2
        self.refresh()
        return Hz, Hzc

    def _hessian_sparse_multi(self, y_im, y_flow, y_m, deltaX=2):
        """reference kalman.py:539-581: per partition of vertex pairs 16 x 2 renders, sums separated by pair label
        (Renderer.j_multi -> hm_j_multi)."""
        n = self.size()
        HTH = np.zeros((n, n))
        for idx, e in enumerate(self.E_hessian):
            e = np.asarray(e, np.int64).reshape(-1, 2)
            self.refresh(idx, hess=True)
            self.renderer.initjacobian(y_im, y_flow, y_m)
            for i1 in range(2):
                for j1 in range(2):
                    for i2 in range(2):
                        for j2 in range(2):
                            off1 = i1 + 2 * self.N * j1
                            off2 = i2 + 2 * self.N * j2
                            ee = np.column_stack((2 * e[:, 0] + off1, 2 * e[:, 1] + off2))
                            h, hist, _ = self.renderer.j_multi(self, deltaX, ee, idx, self.E_hessian_idx[idx])
                            for qi in np.flatnonzero(hist):
                                q = self.Q[qi]
                                q1, q2 = 2 * q[0] + off1, 2 * q[1] + off2
                                HTH[q1, q2] = h[0, qi] / deltaX / deltaX
                                HTH[q2, q1] = HTH[q1, q2]
        self.refresh()
        return HTH


class KalmanFilter:
    def __init__(self, distmesh, im, flow, cuda, vel=None, sparse=True, multi=True, eps_F=1, eps_Z=1e-3,
                 eps_J=1e-3, eps_M=1e-3, verbose=False, renderer=None, device=0):
        self.distmesh = distmesh
        self.N = distmesh.size()
        self.verbose = verbose
        self.state = KFState(distmesh, im, flow, cuda, vel=vel, sparse=sparse, multi=multi, eps_F=eps_F,
                             eps_Z=eps_Z, eps_J=eps_J, eps_M=eps_M, verbose=verbose, renderer=renderer,
                             device=device)
        _lib.register(self, 1)
        self.predtime = 0
        self.updatetime = 0
        self.projecttime = 0
        # compute() returns the rendered flow planes as host arrays, as the reference does (renderer.py:485-501).
        # A streaming caller that only wants the four error sums sets this to False: the planes stay on the
        # device (8 MB less over PCIe per 1024^2 frame) and compute() returns None in their place.
        self.return_flow = True

    def size(self):
        return self.N * 4

    def close(self):
        """Releases the native state of the filter: its renderer handle (streams, page-locked blocks, device memory)."""
        r = getattr(getattr(self, "state", None), "renderer", None)
        if r is not None and hasattr(r, "close"):
            r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _say(self, msg):
        if self.verbose:
            _log(msg)

    def compute(self, y_im, y_flow, y_m, maskflow=True, imageoutput=None):
        """One frame: predict, project onto the mask, update; returns the error tuple (:676-700).

        ``y_im`` may be a renderer.DeviceObservation (frame, flow and mask already in device
        memory, e.g. the flow straight from hm_brox_calc_dev); y_flow / y_m are then ignored."""
        if isinstance(y_im, DeviceObservation):
            obs = y_im
            self.state.renderer.set_observation_dev(obs)
            y_flow, y_m = obs.raw, obs
            y_flow_mask = obs.masked if maskflow is True else obs.raw
        else:
            self.state.algebra.update_frame(y_im, y_flow, y_m)
            y_flow_mask = MaskedFlow(y_flow, y_m) if maskflow is True else y_flow
        r = self.state.renderer
        r.frame_in_place = True          # the operators below work on the frame just uploaded: no second copy
        try:
            with self.state.host_cap():
                t0 = time.time()
                if self._compute_chained(y_im, y_flow_mask, y_m):
                    t1 = t2 = t0 + (self._chain_predict_s or 0.0)
                else:
                    self.predict()
                    t1 = time.time()
                    self.projectmask(y_m)
                    t2 = time.time()
                    self.update(y_im, y_flow_mask, y_m)
                self._after_update()
                t3 = time.time()
            self.predtime += t1 - t0
            self.projecttime += t2 - t1
            self.updatetime += t3 - t2
            self._say("Prediction time: %g\nProjection time: %g\nUpdate time: %g" % (t1 - t0, t2 - t1, t3 - t2))
            if imageoutput is not None:
                self.screenshots(imageoutput)
            return self.error(y_im, y_flow, y_m, want_flow=self.return_flow)
        finally:
            r.frame_in_place = False

    def screenshots(self, basename):
        """The reference's imageoutput (renderer.py:436-475, kalman.py:638-674): <basename>_<view>.png of the six views at
        the state the update kept, and <basename>_forces.png -> the overlay."""
        from .videoio import write_png
        r = self.state.renderer
        X = self.state.X
        overlay = r.screenshot(saveall=True, basename=basename, X=X)
        orig, pred = getattr(self, "orig_x", None), getattr(self, "pred_x", None)
        tv, fv, mv = getattr(self, "tv", None), getattr(self, "fv", None), getattr(self, "mv", None)
        if not any(a is None for a in (orig, pred, tv, fv, mv)):
            write_png("%s_forces.png" % basename, r.view_forces(X, orig, pred, tv, fv, mv))
        return overlay

    _chain_predict_s = None

    def _compute_chained(self, y_im, y_flow, y_m):
        """Hook: predict -> projectmask -> update as one chain on the device, where a filter can (the mass-spring filter
        with its prediction started ahead on the device); False: the three steps are taken one by one."""
        return False

    def _after_update(self):
        """Hook for work that only needs the state the update ended with (the mass-spring filter starts the next
        frame's state prediction here)."""

    def predict(self):
        """Constant-velocity prediction (:703-718): X <- F X, W <- F W F^T + Weps, F = [[I, I], [0, I]]."""
        t0 = time.time()
        st = self.state
        self.orig_x = st.X.copy()
        st.X = st.F.dot(st.X)
        self.pred_x = st.X.copy()
        st.W = st.algebra.cov_predict(st._W, None, None, 1.0, 0.0, st.eps_F, fetch=False)
        stats.statepredtime[0] += time.time() - t0

    def projectmask(self, y_m):
        """Vertices more than 1 px outside the object are pulled back onto its outline (:724-742).

        The signed distance is the reference's (imgproc.py:195-235): the mask's contours pruned as there (:205-228: the
        largest object and its holes of area >= 40), then the distance to the polygon through the centres of the border
        pixels of what is left, negative inside (imgproc.outline_distance; on the device csrc/project_kernels.h, k_ccl_*
        + k_outline + k_project_mask).  Steps, step size and the stale d / index set follow the reference
        (hm_project_mask; HostAlgebra.project_mask)."""
        if y_m is None:
            return
        X, moved = self.state.algebra.project_mask(self.state.X, None if isinstance(y_m, DeviceObservation) else y_m)
        if moved:
            self.state.X = X
        self.proj_x, self.moved = np.array(self.state.X), moved

    def update(self, y_im, y_flow, y_m):
        """Single EKF step in information form (:745-761): W = inv(inv(W) + HTH), X += W Hz."""
        st = self.state
        X, W = st.X, st.W
        st.algebra.update_begin(W, X)
        t0 = time.time()
        step, Hzc, _ = st.algebra.update_step(st, y_im, y_flow, y_m, want_error=False)   # X0 - X = 0: step = W_new Hz
        stats.stateupdatetc[0] += time.time() - t0
        stats.stateupdatetc[1] += 1
        if not np.all(np.isfinite(step)):
            raise FloatingPointError("information matrix of the update is not positive definite")
        Wn = st.algebra.update_cov(0)
        st.X = X + step
        st.W = Wn
        self.tv = Wn.dot(Hzc[:, 0])
        self.fv = Wn.dot(Hzc[:, 1] + Hzc[:, 2])
        self.mv = Wn.dot(Hzc[:, 3])

    def error(self, y_im, y_flow, y_m, want_flow=True):
        return self.state.renderer.error(self.state, y_im, y_flow, y_m, want_flow=want_flow)


class IteratedKalmanFilter(KalmanFilter):
    def __init__(self, distmesh, im, flow, cuda, sparse=True, multi=True, nI=10, eps_F=1e-3, eps_Z=1e-3,
                 eps_J=1e-3, eps_M=1e10, **kw):
        KalmanFilter.__init__(self, distmesh, im, flow, cuda, sparse=sparse, multi=multi, eps_F=eps_F, eps_Z=eps_Z,
                              eps_J=eps_J, eps_M=eps_M, **kw)
        self.nI = nI
        self.reltol = 1e-4
        self.fused_update = True         # hm_update_run; False: the same loop in Python over hm_update_step
        # the diagnostics of reference kalman.py:826-828 (tv, fv, mv = W Hzc[:, 0], W (Hzc[:, 1] + Hzc[:, 2]), W Hzc[:, 3])
        # are formed on the device by the fused update; True: they cross to the host when they are read, not every frame
        self.lazy_gains = True
        self._gains = (None, None, None)

    def _gain(self, k):
        if self._gains is None:
            _, g = self.state.algebra.update_tail()
            self._gains = (g[0], g[1], g[2])
        return self._gains[k]

    def _set_gain(self, k, v):
        g = list(self._gains) if self._gains is not None else [None, None, None]
        g[k] = v
        self._gains = tuple(g)

    tv = property(lambda self: self._gain(0), lambda self, v: self._set_gain(0, v))
    fv = property(lambda self: self._gain(1), lambda self, v: self._set_gain(1, v))
    mv = property(lambda self: self._gain(2), lambda self, v: self._set_gain(2, v))

    def _update_fused(self, y_im, y_flow, y_m):
        """The whole loop below in one native call (hm_update_run): same numbers, the iterate and
        the covariance stay on the device."""
        st = self.state
        t0 = time.time()
        # (the gains -- tv, fv, mv below -- are fetched when somebody reads them: the call does not wait for their kernels)
        lazy = bool(self.lazy_gains)
        # (an update that raises leaves no gains of an earlier frame behind: tv / fv / mv then ask update_tail(), which
        # reports that the last update failed)
        self._gains = None
        X, info, errs, Hzc, gains, W = st.algebra.update_run(st._W, st.X, y_im, y_flow, y_m, self.nI, self.reltol, tail=not lazy)
        stats.stateupdatetc[0] += time.time() - t0
        stats.stateupdatetc[1] += info["niter"]
        for i, e in enumerate(errs):
            self._say("   IEKF K = %d" % i)
            if info["reverted"] and i == len(errs) - 1:
                self._say("** Mesh inconsistent ** Reverting to last good state and continuing")
            else:
                self._say("-- e_im: %d, e_fx: %d, e_fy: %d, e_m: %d" % tuple(e))
        st.X = X
        st.W = W
        st._ori_stale = True             # (update_orientation when ori / sineface are next read)
        self.niter = info["niter"]
        stats.niter += self.niter
        self.reverted, self.converged = info["reverted"], info["converged"]
        if lazy:
            self._gains = None                # tv / fv / mv: renderer.update_tail() on first access
        else:
            self._gains = (gains[0], gains[1], gains[2])

    def update(self, y_im, y_flow, y_m):
        """Iterated EKF in information form (:774-831).

        Per iteration the reference forms W = inv(invW0 + HTH) and
        X = X0 + W Hz - W HTH (X0 - X).  Only W (Hz - HTH (X0 - X)) is needed to move the state,
        so each iteration factorises invW0 + HTH once (Cholesky) and solves; the covariance is
        formed for the state that is kept (the last accepted one).  With the HIP renderer the
        factorisations run on the device (hm_update_begin / _step / _cov) and only the 4N-vector
        of the step crosses PCIe per iteration."""
        st = self.state
        if self.fused_update and st.native:
            return self._update_fused(y_im, y_flow, y_m)
        X = st.X
        X_orig, X_old = X.copy(), X.copy()
        st.algebra.update_begin(st._W, X_orig)
        accepted = 0                     # iterations whose state was kept
        eold = 0.0
        conv = False
        reverted = False
        Hzc = np.zeros((st.size(), 4))
        self.niter = 0
        for i in range(self.nI):
            self._say("   IEKF K = %d" % i)
            t0 = time.time()
            step, Hzc, _ = st.algebra.update_step(st, y_im, y_flow, y_m)
            if not np.all(np.isfinite(step)):
                # inv(W) is positive definite and HTH is a Gram matrix of the difference images
                # (positive semi-definite), so this only happens with non-finite inputs
                raise FloatingPointError("the update system inv(W) + HTH is not positive definite "
                                         "(non-finite state, covariance or observation?)")
            stats.stateupdatetc[0] += time.time() - t0
            stats.stateupdatetc[1] += 1
            X = X_orig + step
            st.X = X
            self.niter += 1
            st.update_orientation()
            if np.any(st.ori < 0):
                st.X = X_old
                reverted = True
                self._say("** Mesh inconsistent ** Reverting to last good state and continuing")
                break
            # the error of the iterate just stepped to: natively it came back with the step; a measurement object on the
            # host is asked only now -- an iterate that is reverted is never rendered
            e_im, e_fx, e_fy, e_m = st.algebra.step_error(st, y_im, y_flow, y_m)
            enew = float(np.sqrt(float(e_im) ** 2 + e_fx ** 2 + e_fy ** 2 + float(e_m) ** 2))
            self._say("-- e_im: %d, e_fx: %d, e_fy: %d, e_m: %d" % (e_im, e_fx, e_fy, e_m))
            accepted += 1
            if abs(enew - eold) / enew < self.reltol:
                conv = True
                break
            eold = enew
            X_old = X.copy()
        stats.niter += self.niter
        # the covariance of the state that is kept: of the last step (0), of the one before (1) or the prior (-1)
        if reverted:
            st.W = st.algebra.update_cov(-1 if accepted == 0 else 1, fetch=False)
        else:
            st.W = st.algebra.update_cov(-1 if self.niter == 0 else 0, fetch=False)
        self.reverted = reverted
        Wd = st.W
        self.tv = Wd.dot(Hzc[:, 0])
        self.fv = Wd.dot(Hzc[:, 1] + Hzc[:, 2])
        self.mv = Wd.dot(Hzc[:, 3])
        self.converged = conv


class PredictionAhead:
    """The state prediction of the mass-spring filter `kf` started ahead of the frame that needs it: the hm_ms_worker
    handle (a host thread; attached to the renderer, its jobs run as one launch on the device), the inputs the job in
    flight was started from, and what the fused update was armed with."""

    def __init__(self, kf):
        self._kf = kf
        self._worker = None
        self.attached = None             # the worker is attached to the renderer's device (None: not yet decided)
        self._job = None                 # (X, bars, l0, parameters) the job in flight was started from
        self._armed = None               # (bars, l0, parameters) the running update starts a job with (hm_update_arm_newton)
        self.cov_armed = False           # ... and it queues the covariance half of the prediction as well (hm_update_arm_cov)

    def inputs(self):
        """(bars, l0, parameters) a job would be started from now."""
        kf = self._kf
        return (np.ascontiguousarray(kf._bars, np.int32).copy(), np.ascontiguousarray(kf.state.l0[:, 0], np.float64).copy(),
                (float(kf.kappa), float(kf.M), float(kf.deltat), int(kf.maxiter), float(kf.tol)))

    def _state(self):
        return np.ascontiguousarray(self._kf.state.X.reshape(-1), np.float64).copy()

    def worker(self):
        st = self._kf.state
        if self._worker is None:
            w = ctypes.c_void_p()
            _lib.check(_lib.lib().hm_ms_worker_create(ctypes.byref(w)), "hm_ms_worker_create")
            self._worker = w
            self.attached = None
        dev = bool(self._kf.newton_on_device) and st.native
        if dev != self.attached:
            if st.native:
                st.algebra.attach_worker(self._worker, dev)
            self.attached = dev
        return self._worker

    def start(self):
        """Start the prediction from the filter's state, springs and parameters as they are now (hm_ms_newton_start)."""
        X = self._state()
        bars, l0, par = self.inputs()
        _lib.check(_lib.lib().hm_ms_newton_start(self.worker(), int(self._kf.state.N), int(bars.shape[0]), _lib.ptr(bars),
                                                 _lib.ptr(l0), par[0], par[1], par[2], par[3], par[4], _lib.ptr(X)),
                   "hm_ms_newton_start")
        self._job = (X, bars, l0, par)

    def arm(self, cov):
        """Before a fused update: hm_update_run starts the job itself the moment the state it ends with is known, and
        (cov) queues the covariance half of the next prediction behind its own launches."""
        r = self._kf.state.algebra
        bars, l0, par = self.inputs()
        r.arm_newton(self.worker(), bars, l0, *par)
        self._armed = (bars, l0, par)
        if cov:
            r.arm_cov(self._kf.state.eps_F)
            self.cov_armed = True

    def adopt(self):
        """After the update that was armed: the job it started is the one in flight, from the state it ended with.
        False: the update was not armed."""
        if self._armed is None:
            return False
        self._job = (self._state(),) + self._armed
        self._armed = None
        return True

    def matches(self):
        """Are the state, the springs and the parameters still what the job in flight was started from?"""
        if self._job is None:
            return False
        kf = self._kf
        X0, bars0, l00, par0 = self._job
        return (np.array_equal(X0, np.asarray(kf.state.X, np.float64).reshape(-1)) and np.array_equal(bars0, kf._bars)
                and np.array_equal(l00, kf.state.l0[:, 0])
                and par0 == (float(kf.kappa), float(kf.M), float(kf.deltat), int(kf.maxiter), float(kf.tol)))

    def finish(self):
        """Wait for the job in flight -> (X predicted [4N], Newton iterations)."""
        out = np.empty(4 * self._kf.state.N)
        its = ctypes.c_int()
        self._job = None
        _lib.check(_lib.lib().hm_ms_newton_finish(self._worker, _lib.ptr(out), ctypes.byref(its)), "hm_ms_newton_finish")
        return out, its.value

    def take(self):
        """The result of the job in flight if it still matches the filter; else None (it is waited for and dropped)."""
        if self._job is None:
            return None
        same = self.matches()
        res = self.finish()
        return res if same else None

    def release(self):
        """The job in flight is finished by someone else (the chained update, on the device)."""
        self._job = None

    def drain(self):
        """After an update that failed: whether the job it was armed with was started is not known -- wait for it if it was."""
        self.cov_armed = False
        if self._armed is None:
            return
        self._armed = None
        out = np.empty(4 * self._kf.state.N)
        rc = _lib.lib().hm_ms_newton_finish(self._worker, _lib.ptr(out), None)
        if rc != _lib.HM_ERR_STATE:          # (HM_ERR_STATE: this worker has never been given a job)
            _lib.check(rc, "hm_ms_newton_finish")

    def close(self):
        if self._worker is not None:
            st = self._kf.state
            if st.native:
                st.algebra.detach_worker(self._worker)
            _lib.lib().hm_ms_worker_destroy(self._worker)
            self._worker = None
            self._job = self._armed = None


class IteratedMSKalmanFilter(IteratedKalmanFilter):
    """Iterated filter with mass-spring dynamics (:834-960)."""

    def __init__(self, distmesh, im, flow, cuda, sparse=True, multi=True, nI=10, eps_F=1e-1, eps_Z=1e-3,
                 eps_J=1, eps_M=1, **kw):
        IteratedKalmanFilter.__init__(self, distmesh, im, flow, cuda, sparse=sparse, multi=multi, eps_F=eps_F,
                                      eps_Z=eps_Z, eps_J=eps_J, eps_M=eps_M, nI=nI, **kw)
        self.M = 1
        self.kappa = -1
        self.deltat = 0.05
        self.maxiter = 1000
        self.tol = 1e-4
        self.force = lambda l1, l2: -self.kappa * (l1 - l2)
        self.state.setforce(self.force)
        self._bars = np.asarray(self.distmesh.bars, np.int64)
        # True: hm_ms_predict, the whole prediction in one native call with the Newton iterations of the state as a
        # single workgroup on the device.  Measured at 201 vertices (tools/predict_time.py): 1.21 ms against 0.68 ms
        # for the default below -- ~500 dependent conjugate-gradient steps of a 402-unknown system are ~2 us each
        # on one CU and ~0.8 us on a host core.  False: hm_cov_predict, hm_update_prefactor (the covariance half
        # of the update queued from a helper thread) and hm_ms_newton on the host, side by side.
        self.device_predict = False
        # True: the next frame's state prediction (hm_ms_newton, 0.42 ms of host time at 201 vertices) starts on a
        # worker thread as soon as the update has its final state, instead of at the top of the next compute()
        self.predict_ahead = True
        # True (with predict_ahead): the update also queues the covariance half of the next frame's prediction -- F W F^T +
        # Weps at the state it ends with, and the factorisation of the result -- behind its own last launches
        # (hm_update_arm_cov); predict() takes it if the state, the springs and the parameters are still the same.
        self.cov_ahead = True
        # True: the prediction started ahead runs as one launch on the device (hm_ms_worker_attach: k_ms_newton4, four
        # waves, a vertex per lane) instead of on the worker's host thread, when the mesh fits the kernel (<= 256
        # vertices); the two agree to rounding
        self.newton_on_device = True
        # True: compute() chains predict -> projectmask -> update on the device when it can (_compute_chained)
        self.chain = True
        self._ahead = PredictionAhead(self)

    def _spring_blocks(self):
        """Per spring the symmetric block (Bxx, Bxy, Byy) of dfdy at the current vertices: B = k I + c d d^T with
        k = kappa (1 - l0/l), c = kappa l0 / l^3 (reference kalman.py:865-902; kalman_host._spring_jacobian assembles them)."""
        st = self.state
        y = st.vertices()
        d = y[self._bars[:, 0]] - y[self._bars[:, 1]]
        l = np.sqrt((d * d).sum(axis=1))
        l0 = st.l0[:, 0]
        k = self.kappa * (1 - l0 / l)
        c = self.kappa * l0 / (l * l * l)           # (the operations of the native spring_blocks, csrc/ctx.h: same bits)
        return np.column_stack((k + c * d[:, 0] * d[:, 0], c * d[:, 0] * d[:, 1], k + c * d[:, 1] * d[:, 1]))

    def predict(self):
        t0 = time.time()
        st = self.state
        self.orig_x = st.X.copy()
        # F = [[I, dt I], [dt/M dfdy, I]] at the state before the step (:856)
        if self.device_predict and isinstance(st._W, DeviceCovariance):
            self._ahead.take()               # a prediction started ahead on the host is not what this path uses
            # the whole prediction in one native call (hm_ms_predict): the Newton iterations of the state as one
            # workgroup on a second stream while the covariance prediction and, for the fused update, the
            # factorisation / inversion it starts with are queued on the filter's stream
            st.X, self.newton_iterations, st.W = st.algebra.ms_predict(
                st._W, st.X, self._bars, st.l0[:, 0], self.kappa, self.M, self.deltat, self.maxiter, self.tol, st.eps_F,
                prefactor=self.fused_update)
        else:
            # the covariance half first: it is queued on the device (prediction, then the
            # factorisation and inversion the update starts with) and runs while the host works
            # through the Newton iterations of the state
            self._predict_cov()
            self._newton()
        self.pred_x = st.X.copy()
        stats.statepredtime[0] += time.time() - t0

    def _predict_cov(self):
        """The covariance half of the prediction, F W F^T + Weps at the state before the step: what the update of the
        last frame queued behind its own launches (hm_update_arm_cov), if it was made from exactly this state, else
        cov_predict now -- and, for the fused update, the factorisation / inversion it starts with (update_prefactor)."""
        st = self.state
        taken = None
        if self._ahead.cov_armed:
            taken = st.algebra.predict_take(st._W, st.X, self._bars, st.l0[:, 0], self.kappa, self.deltat,
                                            self.deltat / self.M, st.eps_F)
        self._ahead.cov_armed = False
        if taken is not None:
            st.W = taken
        else:
            blocks = self._spring_blocks()
            st.W = st.algebra.cov_predict(st._W, self._bars, blocks, self.deltat, self.deltat / self.M, st.eps_F, fetch=False)
            if self.fused_update and st.native:
                st.algebra.update_prefactor(st._W)

    def _compute_chained(self, y_im, y_flow, y_m):
        """predict -> projectmask -> update (reference kalman.py:676-700) without the host between them: the state
        prediction started ahead on the device is still in flight or has just ended, projectmask of its result is queued
        behind it (hm_chain_project), the update takes the projected state from device memory as its prior mean and reports
        what the two kernels found (predicted / projected state, Newton iterations) with its own results.  The covariance
        half of predict() is what it always is here (_predict_cov).  Same numbers as the three steps; taken
        when every precondition of theirs holds: fused update, prediction started ahead on the device from exactly the
        current state, springs and parameters, mask of the observation resident on the device.  chain = False switches it
        off."""
        st = self.state
        ahead = self._ahead
        if not (self.chain and self.fused_update and self.predict_ahead and self.newton_on_device and not self.device_predict
                and ahead.attached and isinstance(y_m, DeviceObservation)
                and isinstance(st._W, DeviceCovariance) and ahead.matches()):
            return False
        t0 = time.time()
        if not st.algebra.chain_project():   # nothing in flight after all
            return False
        self.orig_x = st.X.copy()
        self._predict_cov()
        ahead.release()
        self._chain_predict_s = time.time() - t0
        stats.statepredtime[0] += self._chain_predict_s
        try:
            self.update(y_im, y_flow, y_m)
        except ChainedPredictionFailed:
            # the prediction's inner solve gave up on the device (never observed; test knob newton_fail): on the host,
            # then the three steps; the covariance prediction above stands
            self._newton()
            self.pred_x = st.X.copy()
            self.projectmask(y_m)
            self.update(y_im, y_flow, y_m)
            return True
        pred, proj, its, moved = st.algebra.chain_states()
        self.pred_x = pred.reshape(-1, 1)
        self.proj_x = proj.reshape(-1, 1)
        self.newton_iterations = its
        self.moved = moved
        return True

    def _update_fused(self, y_im, y_flow, y_m):
        """hm_update_run, armed (hm_update_arm_newton) to start the next frame's state prediction on the worker thread
        the moment the state it ends with is known -- before the covariance of that state is formed and fetched."""
        if self.predict_ahead and not self.device_predict:
            self._ahead.arm(cov=self.cov_ahead)
        if getattr(y_m, "next_mask", None):
            self.state.algebra.arm_mask(y_m.next_mask)   # the next frame's outline: queued when this update has its final state
        try:
            IteratedKalmanFilter._update_fused(self, y_im, y_flow, y_m)
        except Exception:
            self._ahead.drain()
            raise

    def _after_update(self):
        """The state the update ended with is what the next frame's _newton starts from: it runs on the worker thread
        (started by hm_update_run itself when armed, else here by hm_ms_newton_start) beside the end of this frame
        on the device and the caller's work between frames.  predict() takes the result if the state is still the
        one it was started from."""
        if self.predict_ahead and not self._ahead.adopt() and not self.device_predict:
            self._ahead.start()

    def close(self):
        ahead = getattr(self, "_ahead", None)
        if ahead is not None:
            ahead.close()
        KalmanFilter.close(self)

    def __del__(self):
        try:
            self.close()
        except Exception:               # noqa: BLE001 -- interpreter shutdown
            pass

    def _newton(self):
        """20 implicit-Euler sub-steps, each solved by Newton's method (:923-960) -- native host
        code in libhydra_mi.so (csrc/predict.cpp: block-eliminated 2N x 2N system, spring operator
        applied bar by bar, conjugate gradients)."""
        st = self.state
        res = self._ahead.take()
        if res is None and self.newton_on_device and st.native:
            # the same launch a prediction started ahead would have been: the same bits with and without predict_ahead
            self._ahead.start()
            res = self._ahead.finish()
        if res is None:
            X = np.ascontiguousarray(st.X.reshape(-1), np.float64).copy()
            bars, l0, par = self._ahead.inputs()
            its = ctypes.c_int()
            _lib.check(_lib.lib().hm_ms_newton(int(st.N), int(bars.shape[0]), _lib.ptr(bars), _lib.ptr(l0), par[0], par[1],
                                               par[2], par[3], par[4], _lib.ptr(X), ctypes.byref(its)), "hm_ms_newton")
            res = X, its.value
        self.newton_iterations = res[1]
        st.X = res[0].reshape(-1, 1)
