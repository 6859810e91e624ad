// The prediction between two frames on MI355X: the covariance prediction W' = F W F^T + Weps (hm_cov_predict), the same
// queued ahead by the update that precedes it (queue_predict_ahead, hm_predict_take), the whole mass-spring prediction in
// one call (hm_ms_predict) and the state prediction's Newton loop started ahead on a stream of its own (hm_newton_dev_*).
// Host orchestration and C-ABI (include/hydra_mi.h); the kernels are in predict_kernels.h, which this translation unit alone
// compiles -- those of the covariance are update.hip's, queued through ekf_queue_fpft and prior_inverse (ctx.h).  (Not
// predict.cpp: that is the host's Newton loop and its worker thread.)
// Of the handle (ctx.h) it writes `sp`, `pq`, `newton` and `newton4`; of the shared state d_Wres, prefactored, upd_open and
// the dense buffers the covariance launches fill; of the others' chain.pending (cleared: a new prediction is in flight).
#include "ctx.h"
#include "predict_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// (spring_csr, spring_blocks: ctx.h)
// Covariance prediction W' = F W F^T + Weps (kalman.py:717, 863) on the device.
//   W_in   : the covariance to propagate (host), or NULL to use the one hm_update_cov returned last,
//            which is still on the device;
//   bars / blocks : the springs and, per spring, the symmetric 2x2 block (Bxx, Bxy, Byy) of the force
//            Jacobian at the state before the step; n_bars = 0 gives the constant-velocity F (A = 0);
//   a, s   : F = [[I, a I], [s dfdy, I]];  eps_F : Weps = eps_F [[I/4, I/2], [I/2, I]].
// The result is copied to W_out and stays on the device as the prior of the next hm_update_begin(NULL).
// ahead: called by hm_update_run for the NEXT frame, behind launches that are still running -- nothing here may wait for
// the stream: the spring blocks go through page-locked memory (`blocks` is h->sp.pin_blk), the result goes straight to
// d_Wprior (where prior_inverse wants it) and the resident covariance (d_Wres, the posterior the caller may still
// fetch) is left alone.
static int cov_predict_core(hm_ctx *h, const double *W_in, int n_bars, const int32_t *bars, const double *blocks,
                            double a, double s, double eps_F, double *W_out, bool ahead, hipStream_t st = nullptr)
{
    if (!st) st = h->stream;
    const int N = h->N, n4 = 4 * N;
    const size_t nn = (size_t)n4 * n4 * sizeof(double);
    std::vector<int> &off = h->sp.h_off, &bar = h->sp.h_bar, &other = h->sp.h_other;   // live until the copies ran
    if (!ahead) HM_HIP(stream_wait(st));      // ... of the previous call
    // the springs' topology rarely changes between frames: its device copy is kept and only the per-spring blocks go up
    const bool same_topo = h->sp.d_off && h->sp.bars_cached.size() == 2 * (size_t)n_bars &&
                           (n_bars == 0 || memcmp(h->sp.bars_cached.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0);
    if (!same_topo) {
        for (int i = 0; i < n_bars; i++)
            HM_ARG(bars[2 * i] >= 0 && bars[2 * i] < N && bars[2 * i + 1] >= 0 && bars[2 * i + 1] < N,
                   "hm_cov_predict: spring %d refers to a vertex outside 0..%d", i, N - 1);
        spring_csr(N, n_bars, bars, off, bar, other);
        HM_HIP(h->own.alloc(&h->sp.d_off, (size_t)(N + 1) * sizeof(int)));
        HM_HIP(h->own.grow(&h->sp.d_bar, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->sp.d_other, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->sp.d_blk, 3 * (size_t)n_bars * sizeof(double)));
        HM_HIP(hipMemcpyAsync(h->sp.d_off, off.data(), (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
        if (n_bars > 0) {
            HM_HIP(hipMemcpyAsync(h->sp.d_bar, bar.data(), bar.size() * sizeof(int), hipMemcpyHostToDevice, st));
            HM_HIP(hipMemcpyAsync(h->sp.d_other, other.data(), other.size() * sizeof(int), hipMemcpyHostToDevice, st));
        }
        h->sp.bars_cached.assign(bars, bars + 2 * (size_t)n_bars);
    }
    if (n_bars > 0) {
        const double *from = blocks;
        if (!ahead) {
            h->sp.h_blk.assign(blocks, blocks + 3 * (size_t)n_bars);
            from = h->sp.h_blk.data();
        }
        HM_HIP(hipMemcpyAsync(h->sp.d_blk, from, 3 * (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const double *src = h->d_Wres;
    if (W_in) {
        HM_HIP(hipMemcpyAsync(h->d_H, W_in, nn, hipMemcpyHostToDevice, st));
        src = h->d_H;
    } else if (src == h->d_Wtmp) {               // the output buffer: move the input out of the way
        HM_HIP(hipMemcpyAsync(h->d_H, h->d_Wtmp, nn, hipMemcpyDeviceToDevice, st));
        src = h->d_H;
    }
    SpringTopo tp = {h->sp.d_off, h->sp.d_bar, h->sp.d_other, h->sp.d_blk};
    ekf_queue_fpft(st, src, h->d_Awork, ahead ? h->d_Wprior : h->d_Wtmp, N, tp, a, s, eps_F);      // (d_Awork: scratch)
    HM_HIP(hipGetLastError());
    if (ahead) return HM_OK;
    if (W_out) HM_HIP(hipMemcpyAsync(W_out, h->d_Wtmp, nn, hipMemcpyDeviceToHost, st));
    if (W_out) HM_HIP(stream_wait(st));
    h->d_Wres = h->d_Wtmp;
    h->prefactored = false;
    return HM_OK;
}

extern "C" int hm_cov_predict(hm_ctx_t h, const double *W_in, int n_bars, const int32_t *bars, const double *blocks,
                              double a, double s, double eps_F, double *W_out)
{
    HM_ARG(h && n_bars >= 0 && (n_bars == 0 || (bars && blocks)), "hm_cov_predict: bad argument");
    HM_JOIN(h);
    if (!W_in && !h->d_Wres) {
        hm_set_error("hm_cov_predict: no covariance given and none resident on the device");
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    h->pq.valid = false;                         // a prediction queued ahead (hm_update_arm_cov) is not what this caller wants
    return cov_predict_core(h, W_in, n_bars, bars, blocks, a, s, eps_F, W_out, false);
}

// hm_update_run, armed by hm_update_arm_newton + hm_update_arm_cov, when its state is final and the covariance of that
// state (d_Wres) is queued: the covariance half of the NEXT frame's prediction -- W' = F W F^T + Weps with F at this
// state (hm_cov_predict) and the factorisation / inverse of W' the next update starts with (hm_update_prefactor) --
// goes onto the stream right behind it, ~0.3 ms before the caller could ask for it (it first has to get back to
// IteratedMSKalmanFilter.predict).  Nothing is made current: hm_predict_take does that when the caller's inputs turn
// out to be the ones used here; otherwise the caller's own hm_cov_predict starts from the posterior, which is intact.
int queue_predict_ahead(hm_ctx *h, const double *X, int n_bars, const int32_t *bars, const double *l0, double kappa,
                        double M, double dt, double eps_F, hipStream_t st)
{
    for (int i = 0; i < 2 * n_bars; i++)
        if (bars[i] < 0 || bars[i] >= h->N) return HM_OK;                 // the caller's own hm_cov_predict reports it
    HM_HIP(h->own.host_grow(&h->sp.pin_blk, 3 * (size_t)n_bars * sizeof(double), hipHostMallocDefault));
    spring_blocks(n_bars, bars, l0, kappa, X, h->sp.pin_blk);
    double *const post = h->d_Wres;
    HM_TRY(cov_predict_core(h, nullptr, n_bars, bars, h->sp.pin_blk, dt, dt / M, eps_F, nullptr, true, st));
    h->d_Wres = h->d_Wprior;                     // (prior_inverse: the prior is where it belongs already)
    const int rc = prior_inverse(h, nullptr, st);
    h->d_Wres = post;
    if (rc) return rc;
    h->upd_open = false;                         // the factor slots and d_Wprior belong to the next update now
    h->pq.X.assign(X, X + 4 * (size_t)h->N);
    h->pq.bars.assign(bars, bars + 2 * (size_t)n_bars);
    h->pq.l0.assign(l0, l0 + n_bars);
    h->pq.par[0] = kappa; h->pq.par[1] = dt; h->pq.par[2] = dt / M; h->pq.par[3] = eps_F;
    h->pq.valid = true;
    return HM_OK;
}

// Makes the prediction hm_update_run queued ahead current -- as if hm_cov_predict(h, NULL, n_bars, bars, blocks at X, a, s,
// eps_F, NULL) and hm_update_prefactor(h) had just been called -- when it was made from exactly these inputs (compared
// bit for bit) and the posterior it started from is still the resident covariance.  Returns HM_OK when taken, 1 when
// there is nothing to take (the caller then makes those two calls itself).
extern "C" int hm_predict_take(hm_ctx_t h, const double *X, int n_bars, const int32_t *bars, const double *l0, double kappa,
                               double a, double s, double eps_F)
{
    HM_ARG(h && X && n_bars >= 0 && (n_bars == 0 || (bars && l0)), "hm_predict_take: bad argument");
    HM_JOIN_LAZY(h);
    if (!h->pq.valid) return 1;
    h->pq.valid = false;
    const size_t n4 = (size_t)4 * h->N;
    const bool same = h->pq.X.size() == n4 && memcmp(h->pq.X.data(), X, n4 * sizeof(double)) == 0 &&
                      h->pq.l0.size() == (size_t)n_bars &&
                      (n_bars == 0 || (memcmp(h->pq.bars.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0 &&
                                       memcmp(h->pq.l0.data(), l0, (size_t)n_bars * sizeof(double)) == 0)) &&
                      h->pq.par[0] == kappa && h->pq.par[1] == a && h->pq.par[2] == s && h->pq.par[3] == eps_F;
    if (!same || !h->d_Wres) return 1;
    h->d_Wres = h->d_Wprior;
    h->prefactored = true;
    h->upd_open = false;
    return HM_OK;
}


// IteratedMSKalmanFilter.predict (kalman.py:850-863) in one call: F from the spring Jacobian at the state before the
// step (:856, _dfdx :904-912), the state advanced by _newton (:923-960), W <- F W F^T + Weps (:863) -- and, since
// it only needs the predicted covariance, the covariance half of the update that follows (factorisation and inverse,
// what hm_update_prefactor queues).  The Newton iterations run as one workgroup on a second stream
// (csrc/predict_kernels.h) while this thread queues the ~30 launches of the covariance half on the handle's stream;
// meshes too large for that kernel's LDS footprint take the host version (hm_ms_newton).
extern "C" int hm_ms_predict(hm_ctx_t h, int n_bars, const int32_t *bars, const double *l0, double kappa, double M, double dt,
                             int maxiter, double tol, double eps_F, double *X, int *newton_iterations, int prefactor)
{
    HM_ARG(h && bars && l0 && X && n_bars >= 1, "hm_ms_predict: bad argument");
    HM_ARG(dt > 0 && M > 0 && maxiter >= 1 && tol > 0, "hm_ms_predict: bad parameter");
    HM_JOIN(h);
    if (!h->d_Wres) { hm_set_error("hm_ms_predict: no covariance resident on the device"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    const int N = h->N, n4 = 4 * N;
    for (int i = 0; i < 2 * n_bars; i++) HM_ARG(bars[i] >= 0 && bars[i] < N, "hm_ms_predict: bar refers to vertex %d", bars[i]);
    // the spring blocks of dfdy at the state before the step (kalman.py:892-901)
    std::vector<double> blk(3 * (size_t)n_bars);
    spring_blocks(n_bars, bars, l0, kappa, X, blk.data());
    const size_t lds = ((size_t)34 * N + (size_t)7 * n_bars + 8) * sizeof(double) + ((size_t)N + 1 + 4 * (size_t)n_bars) * sizeof(int);
    const bool on_device = lds <= 160 * 1024;
    if (on_device) {
        HM_TRY(ensure_stream2(h));
        if (!h->newton.ready) {
            HM_HIP(h->own.alloc(&h->newton.d_X, (size_t)n4 * sizeof(double)));
            HM_HIP(h->own.alloc(&h->newton.d_voff, (size_t)(N + 1) * sizeof(int)));
            HM_HIP(h->own.alloc(&h->newton.d_info, 2 * sizeof(int)));
            HM_HIP(hipFuncSetAttribute((const void *)k_ms_newton, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            h->newton.ready = true;
        }
        HM_HIP(h->own.grow(&h->newton.d_bars, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->newton.d_vbar, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->newton.d_l0, (size_t)n_bars * sizeof(double)));
        std::vector<int> off, vbar, other;                   // the bars of every vertex, ascending (k_ms_newton reads no `other`)
        spring_csr(N, n_bars, bars, off, vbar, other);
        HM_HIP(hipMemcpyAsync(h->newton.d_bars, bars, 2 * (size_t)n_bars * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->newton.d_l0, l0, (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->newton.d_voff, off.data(), (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->newton.d_vbar, vbar.data(), vbar.size() * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->newton.d_X, X, (size_t)n4 * sizeof(double), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipStreamSynchronize(h->stream2));            // off / vbar are locals (pageable copies have returned anyway)
        NewtonArgs a = {N, n_bars, h->newton.d_bars, h->newton.d_l0, h->newton.d_voff, h->newton.d_vbar, kappa, M, dt, tol, maxiter,
                        (int)std::ceil(1.0 / dt), h->newton.d_X, h->newton.d_info};
        hipLaunchKernelGGL(k_ms_newton, dim3(1), dim3(NEWTON_NT), lds, h->stream2, a);
        HM_HIP(hipGetLastError());
    }
    // covariance: W <- F W F^T + Weps on the handle's stream, then (prefactor) its factor and inverse
    int rc = hm_cov_predict(h, nullptr, n_bars, bars, blk.data(), dt, dt / M, eps_F, nullptr);
    if (rc == HM_OK && prefactor) {
        rc = prior_inverse(h, nullptr);
        if (rc == HM_OK) { h->prefactored = true; h->upd_open = false; }
    }
    int info[2] = {0, 0};
    if (on_device) {
        hipError_t e = hipMemcpyAsync(X, h->newton.d_X, (size_t)n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream2);
        if (e == hipSuccess) e = hipMemcpyAsync(info, h->newton.d_info, sizeof info, hipMemcpyDeviceToHost, h->stream2);
        if (e == hipSuccess) e = stream_wait(h->stream2);
        if (e != hipSuccess) { hm_set_error("hm_ms_predict: %s", hipGetErrorString(e)); return HM_ERR_HIP; }
        if (rc) return rc;
        if (info[1]) { hm_set_error("hm_ms_predict: the inner solve did not converge"); return HM_ERR_STATE; }
        if (newton_iterations) *newton_iterations = info[0];
        return HM_OK;
    }
    if (rc) return rc;
    return hm_ms_newton(N, n_bars, bars, l0, kappa, M, dt, maxiter, tol, X, newton_iterations);
}


// ---- the state prediction's Newton loop on the device, started ahead (csrc/predict_kernels.h: k_ms_newton4) -----------------
// hm_newton_dev_start queues ONE launch on a stream of its own: the state goes in and comes out through page-locked
// memory, the host watches a ticket (hm_newton_dev_finish).  Called by the worker object of csrc/predict.cpp when a
// handle is attached to it (hm_ms_worker_attach): from hm_update_run the moment its state is final, i.e. the kernel
// runs beside the covariance launches of the frame that ends and the caller's way back to predict().  Returns 1 when
// this mesh does not fit the kernel (more than 256 vertices, a vertex with more than 12 springs): the caller takes the
// host loop.
extern "C" int hm_newton_dev_start(hm_ctx_t h, int N, int n_bars, const int32_t *bars, const double *l0, double kappa, double M,
                                   double dt, int maxiter, double tol, const double *X)
{
    HM_ARG(h && bars && l0 && X && n_bars >= 1, "hm_newton_dev_start: bad argument");
    if (N != h->N || N > NEWTON4_NT) return 1;
    // it may create the resources below, so the tail of the last update must not be queueing (hm_ms_newton_start calls
    // it between frames); the prefactor worker, which creates nothing, goes on
    if (const int rc = helper_join(h)) return rc;
    HM_HIP(hipSetDevice(h->device));
    if (h->newton4.pending) {                          // a prediction nobody fetched: let it finish (its result block is dropped)
        HM_HIP(hipStreamSynchronize(h->newton4.stream));
        h->newton4.pending = false;
    }
    if (!h->newton4.ready) {
        HM_HIP(h->own.stream(&h->newton4.stream));
        // page-locked and coherent (hipHostMalloc without flags already is: the flag states the intent, it was not the
        // cause of round 3's wrong tracks -- host_block.h has that story): [X in (4N) | a result block of 4N + 2 values]
        const size_t words = (size_t)4 * N + 2 * ((size_t)4 * N + 2);
        HM_HIP(h->own.host_alloc(&h->newton4.pin, words * sizeof(double), hipHostMallocCoherent));
        memset(h->newton4.pin, 0, words * sizeof(double));
        HM_HIP(h->own.alloc(&h->newton4.d_X, ((size_t)4 * N + 2) * sizeof(double)));
        h->newton4.v.assign((size_t)4 * N + 2, 0.0);
        HM_HIP(h->own.event(&h->newton4.ev));
        h->newton4.ready = true;
    }
    const bool same = h->newton4.bars.size() == 2 * (size_t)n_bars && memcmp(h->newton4.bars.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0;
    if (!same) {
        for (int i = 0; i < 2 * n_bars; i++) HM_ARG(bars[i] >= 0 && bars[i] < N, "hm_newton_dev_start: bar refers to vertex %d", bars[i]);
        std::vector<int> deg(N, 0);
        for (int i = 0; i < 2 * n_bars; i++) deg[bars[i]]++;
        const int maxdeg = *std::max_element(deg.begin(), deg.end());
        h->newton4.bars.clear();                       // (the springs of the table once it is on the device)
        h->newton4.l0.clear();
        h->newton4.deg = maxdeg <= 8 ? 8 : maxdeg <= 12 ? 12 : 0;
        if (h->newton4.deg) {
            const int D = h->newton4.deg;
            std::vector<int> nbr((size_t)N * D), nbb((size_t)N * D, n_bars), fill(N, 0);
            for (int v = 0; v < N; v++)
                for (int q = 0; q < D; q++) nbr[(size_t)v * D + q] = v;             // padding: the vertex itself, bar I (zero terms)
            for (int i = 0; i < n_bars; i++) {                                        // ascending bar order per vertex
                const int a = bars[2 * i], b = bars[2 * i + 1];
                nbr[(size_t)a * D + fill[a]] = b; nbb[(size_t)a * D + fill[a]++] = i;
                nbr[(size_t)b * D + fill[b]] = a; nbb[(size_t)b * D + fill[b]++] = i;
            }
            HM_HIP(h->own.alloc(&h->newton4.d_nbr, (size_t)N * 12 * sizeof(int)));
            HM_HIP(h->own.alloc(&h->newton4.d_nbb, (size_t)N * 12 * sizeof(int)));
            HM_HIP(h->own.grow(&h->newton4.d_bars, 2 * (size_t)n_bars * sizeof(int)));
            HM_HIP(h->own.grow(&h->newton4.d_l0, (size_t)n_bars * sizeof(double)));
            // on the kernel's own stream and waited for (nbr / nbb are locals): ordered before the launch by the stream
            // itself rather than by hipMemcpy's return (that was not the cause of round 3's wrong tracks either -- a track
            // uploads these tables once, the wrong predictions came at frame 13 -- but it is the form that needs no argument)
            HM_HIP(hipMemcpyAsync(h->newton4.d_nbr, nbr.data(), nbr.size() * sizeof(int), hipMemcpyHostToDevice, h->newton4.stream));
            HM_HIP(hipMemcpyAsync(h->newton4.d_nbb, nbb.data(), nbb.size() * sizeof(int), hipMemcpyHostToDevice, h->newton4.stream));
            HM_HIP(hipMemcpyAsync(h->newton4.d_bars, bars, 2 * (size_t)n_bars * sizeof(int), hipMemcpyHostToDevice, h->newton4.stream));
            HM_HIP(hipStreamSynchronize(h->newton4.stream));            // (nbr / nbb are locals)
        }
        h->newton4.bars.assign(bars, bars + 2 * (size_t)n_bars);
    }
    if (!h->newton4.deg) return 1;
    if (h->newton4.l0.size() != (size_t)n_bars || memcmp(h->newton4.l0.data(), l0, (size_t)n_bars * sizeof(double)) != 0) {
        h->newton4.l0.assign(l0, l0 + n_bars);
        HM_HIP(hipMemcpyAsync(h->newton4.d_l0, h->newton4.l0.data(), (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, h->newton4.stream));
        HM_HIP(hipStreamSynchronize(h->newton4.stream));
    }
    const size_t n4 = (size_t)4 * N;
    memcpy(h->newton4.pin, X, n4 * sizeof(double));
    Newton4Args a;
    a.N = N; a.I = n_bars; a.deg_stride = h->newton4.deg;
    a.bars = h->newton4.d_bars; a.l0 = h->newton4.d_l0; a.nbr = h->newton4.d_nbr; a.nbb = h->newton4.d_nbb;
    a.kappa = kappa; a.M = M; a.dt = dt; a.tol = tol; a.maxiter = maxiter; a.steps = (int)std::ceil(1.0 / dt);
    a.Xin = h->newton4.pin; a.out = h->newton4.pin + n4; a.dev_out = h->newton4.d_X; a.ticket = (double)(++h->newton4.ticket);
    a.delay_us = h->result_delay; a.force_bad = h->newton4.fail;
    const size_t lds = ((size_t)6 * NEWTON4_NT + 4 * ((size_t)n_bars + 1) + 4 * (NEWTON4_NT / 64)) * sizeof(double) + 2 * (size_t)n_bars * sizeof(int);
    if (lds > 64 * 1024) return 1;
    if (h->newton4.deg == 8) hipLaunchKernelGGL((k_ms_newton4<8>), dim3(1), dim3(NEWTON4_NT), lds, h->newton4.stream, a);
    else hipLaunchKernelGGL((k_ms_newton4<12>), dim3(1), dim3(NEWTON4_NT), lds, h->newton4.stream, a);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->newton4.ev, h->newton4.stream));
    h->newton4.pending = true;
    h->chain.pending = false;
    return HM_OK;
}

// Waits for the launch of hm_newton_dev_start; X (4N) receives the advanced state.  Returns 1 when the kernel's inner solve
// did not converge (never observed): the caller repeats the prediction on the host.
extern "C" int hm_newton_dev_finish(hm_ctx_t h, double *X, int *newton_iterations)
{
    HM_ARG(h && X, "hm_newton_dev_finish: bad argument");
    if (!h->newton4.pending) { hm_set_error("hm_newton_dev_finish: no prediction was started"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = (size_t)4 * h->N;
    // the kernel's result block, taken when it is whole (host_block.h); the kernel is usually long done when this is
    // called (it was started at the end of the previous update)
    const int rc = hb_wait(h->newton4.stream, h->newton4.pin + n4, 0, n4 + 2, hb_stamp(h->newton4.ticket), h->newton4.v.data(), "hm_newton_dev_finish");
    h->newton4.pending = false;
    h->chain.pending = false;
    if (rc) return rc;
    if (h->newton4.v[n4 + 1] != 0.0) return 1;
    memcpy(X, h->newton4.v.data(), n4 * sizeof(double));
    if (newton_iterations) *newton_iterations = (int)h->newton4.v[n4];
    return HM_OK;
}
