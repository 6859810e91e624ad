// The Rauch-Tung-Striebel smoother (hm_smooth_*, include/hydra_mi.h): host orchestration and C-ABI; the kernels are in
// smooth_kernels.h, which this translation unit alone compiles.
// A record of the filter's per-frame results -- P_k (the covariance the update kept), x_k, the prior mean m_k the
// update started from -- and the backward recursion over it, all on the device.  What the record does not hold is
// recomputed: Pp_{k+1} = F_k P_k F_k^T + Weps by k_fw_rows / k_pft_cols from slot k and the spring blocks at x_k (the
// launches and inputs of the forward prediction, so the same bits), its factor and inverse by the factorisation the
// update uses; both launch sequences are queued through ekf_queue_fpft and ekf_queue_chol_flow (ctx.h; update.hip compiles
// their kernels).  The buffers belong to the smoother (its own HmOwner); the filter's are only read, and only by the
// copies hm_smooth_record queues.  Of the filter handle (ctx.h) it reads device, N, stream, newton4.stream, tail.stream4, d_X0, d_Wres,
// upd_X0 and flow_wgs, and joins it (ctx_join).
#include "ctx.h"
#include "smooth_kernels.h"
#include <algorithm>
#include <cstring>

struct hm_smooth {
    hm_ctx *ctx;
    int device, cap, K = 0, N, n4, n_bars;
    double kappa, a, s, eps_F;
    HmOwner own{1};
    std::vector<int32_t> bars;
    std::vector<double> l0;
    std::vector<double> hx;          // cap x n4: x_k as given to hm_smooth_record
    std::vector<double> hblk;        // cap x 3 n_bars: the spring blocks (Bxx, Bxy, Byy) at x_k
    double *d_P = nullptr;           // cap slots of n4 x n4: P_k; Ps_k after a run with covariances
    double *d_m = nullptr, *d_x = nullptr, *d_xs = nullptr, *d_var = nullptr;   // cap x n4 each
    double *d_blk = nullptr;         // cap x 3 n_bars
    int *d_off = nullptr, *d_bar = nullptr, *d_other = nullptr;                 // the springs of every vertex (spring_csr)
    // per backward step: F P, Pp, its factor (L, T = L^-1, the diagonal blocks' inverses Lt, the flow launch's scratch),
    // Y = T F P, G, E, and three vectors (d, T d, T^T T d)
    double *d_FP = nullptr, *d_Pp = nullptr, *d_L = nullptr, *d_T = nullptr, *d_Y = nullptr, *d_G = nullptr, *d_E = nullptr;
    double *d_Lt = nullptr, *d_flowP = nullptr, *d_vec = nullptr;
    unsigned *d_ctl = nullptr;       // the factorisation launch's task counter and time-out word
    int *d_flag = nullptr;           // 1 + the first frame whose Pp did not factor
    hipEvent_t ev_mean = nullptr, ev_cov = nullptr;   // behind the copies of m_k / of P_k
    bool smoothed_cov = false;       // the slots hold Ps_k (or, after a failed run, partly): nothing more to record or run
};

extern "C" int hm_smooth_create(hm_ctx_t ctx, int capacity, int n_bars, const int32_t *bars, const double *l0,
                                double kappa, double a, double s, double eps_F, hm_smooth_t *out)
{
    HM_ARG(out != nullptr, "hm_smooth_create: NULL output pointer");
    *out = nullptr;
    HM_ARG(capacity >= 2, "hm_smooth_create: capacity %d: a record needs at least 2 frames", capacity);
    HM_ARG(ctx != nullptr, "hm_smooth_create: NULL filter handle");
    HM_ARG(n_bars >= 0 && (n_bars == 0 || (bars && l0)), "hm_smooth_create: bad springs");
    const int N = ctx->N, n4 = 4 * N;
    for (int i = 0; i < 2 * n_bars; i++)
        HM_ARG(bars[i] >= 0 && bars[i] < N, "hm_smooth_create: spring %d refers to vertex %d (mesh of %d)", i / 2, bars[i], N);
    HM_JOIN(ctx);
    HM_HIP(hipSetDevice(ctx->device));
    hm_smooth *sm = new hm_smooth();
    sm->ctx = ctx; sm->device = ctx->device; sm->cap = capacity; sm->N = N; sm->n4 = n4; sm->n_bars = n_bars;
    sm->kappa = kappa; sm->a = a; sm->s = s; sm->eps_F = eps_F;
    if (n_bars > 0) { sm->bars.assign(bars, bars + 2 * (size_t)n_bars); sm->l0.assign(l0, l0 + n_bars); }
    const size_t nn = (size_t)n4 * n4 * sizeof(double), nv = (size_t)n4 * sizeof(double);
    const int nb = hm_cdiv(n4, DNB);
    int rc = HM_OK;
    auto fail = [&](const char *what, size_t bytes, hipError_t e) {
        hm_set_error("hm_smooth_create: %s: %zu bytes of device memory (%d frames of %d x %d doubles): %s", what, bytes,
                     capacity, n4, n4, hipGetErrorString(e));
        rc = HM_ERR_HIP;
    };
    auto take = [&](auto **p, size_t bytes, const char *what) {
        if (rc) return;
        const hipError_t e = sm->own.alloc(p, bytes);
        if (e != hipSuccess) fail(what, bytes, e);
    };
    take(&sm->d_P, nn * capacity, "the covariance record");
    take(&sm->d_m, nv * capacity, "the prior means");
    take(&sm->d_x, nv * capacity, "the posterior means");
    take(&sm->d_xs, nv * capacity, "the smoothed means");
    take(&sm->d_var, nv * capacity, "the smoothed variances");
    take(&sm->d_blk, std::max<size_t>(1, 3 * (size_t)n_bars * capacity) * sizeof(double), "the spring blocks");
    take(&sm->d_off, (size_t)(N + 1) * sizeof(int), "the spring topology");
    take(&sm->d_bar, std::max<size_t>(1, 2 * (size_t)n_bars) * sizeof(int), "the spring topology");
    take(&sm->d_other, std::max<size_t>(1, 2 * (size_t)n_bars) * sizeof(int), "the spring topology");
    double **work[] = {&sm->d_FP, &sm->d_Pp, &sm->d_L, &sm->d_T, &sm->d_Y, &sm->d_G, &sm->d_E};
    for (double **p : work) take(p, nn, "the work matrices");
    take(&sm->d_Lt, (size_t)nb * DNB * DNB * sizeof(double), "the factorisation");
    take(&sm->d_flowP, (size_t)3 * nb * DNB * DNB * sizeof(double), "the factorisation");
    take(&sm->d_vec, 3 * nv, "the work vectors");
    take(&sm->d_ctl, 4 * sizeof(unsigned), "the factorisation");
    take(&sm->d_flag, sizeof(int), "the status word");
    if (!rc) {
        hipError_t e = sm->own.event(&sm->ev_mean);
        if (e == hipSuccess) e = sm->own.event(&sm->ev_cov);
        std::vector<int> off, bar, other;
        spring_csr(N, n_bars, bars, off, bar, other);
        if (e == hipSuccess) e = hipMemcpy(sm->d_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_bars > 0) e = hipMemcpy(sm->d_bar, bar.data(), bar.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_bars > 0) e = hipMemcpy(sm->d_other, other.data(), other.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) { hm_set_error("hm_smooth_create: %s", hipGetErrorString(e)); rc = HM_ERR_HIP; }
    }
    if (rc) {
        sm->own.release();
        delete sm;
        return rc;
    }
    sm->hx.reserve((size_t)capacity * n4);
    sm->hblk.reserve((size_t)capacity * 3 * n_bars);
    *out = sm;
    return HM_OK;
}

extern "C" int hm_smooth_destroy(hm_smooth_t sm)
{
    if (!sm) return HM_OK;
    (void)hipSetDevice(sm->device);
    sm->own.release();               // (hipFree waits for the device: no copy into the record is still in flight)
    delete sm;
    return HM_OK;
}

extern "C" int hm_smooth_count(hm_smooth_t sm, int *frames, int *capacity)
{
    HM_ARG(sm != nullptr, "hm_smooth_count: NULL handle");
    if (frames) *frames = sm->K;
    if (capacity) *capacity = sm->cap;
    return HM_OK;
}

extern "C" int hm_smooth_record(hm_smooth_t sm, const double *X)
{
    HM_ARG(sm && X, "hm_smooth_record: NULL argument");
    hm_ctx *h = sm->ctx;
    if (sm->smoothed_cov) { hm_set_error("hm_smooth_record: the record has been smoothed with covariances"); return HM_ERR_STATE; }
    if (sm->K >= sm->cap) {
        hm_set_error("hm_smooth_record: the record is full (%d frames)", sm->cap);
        return HM_ERR_STATE;
    }
    HM_JOIN_LAZY(h);                 // (the helper thread has queued the tail of the last update)
    const int n4 = sm->n4, k = sm->K;
    if (!h->d_Wres || h->upd_X0.size() != (size_t)n4) {
        hm_set_error("hm_smooth_record: no update has run on the filter handle");
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    // m_k: the prior mean the update started from, where the update keeps it (d_X0: given to hm_update_begin, or left by
    // the chained projection).  The next chained projection rewrites it on newton4.stream: that stream waits for the copy.
    HM_HIP(hipMemcpyAsync(sm->d_m + (size_t)k * n4, h->d_X0, (size_t)n4 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HM_HIP(hipEventRecord(sm->ev_mean, h->stream));
    if (h->newton4.stream) HM_HIP(hipStreamWaitEvent(h->newton4.stream, sm->ev_mean, 0));
    // P_k: the covariance the update kept, behind the tail that forms it (ctx_join: `stream` waits for tail.stream4), ahead of
    // the next tail (tail.stream4 waits for the copy) and of everything the handle's own stream does next
    HM_JOIN(h);
    HM_HIP(hipMemcpyAsync(sm->d_P + (size_t)k * n4 * n4, h->d_Wres, (size_t)n4 * n4 * sizeof(double), hipMemcpyDeviceToDevice,
                          h->stream));
    HM_HIP(hipEventRecord(sm->ev_cov, h->stream));
    if (h->tail.stream4) HM_HIP(hipStreamWaitEvent(h->tail.stream4, sm->ev_cov, 0));
    sm->hx.insert(sm->hx.end(), X, X + n4);
    sm->hblk.resize((size_t)(k + 1) * 3 * sm->n_bars);
    if (sm->n_bars > 0)
        spring_blocks(sm->n_bars, sm->bars.data(), sm->l0.data(), sm->kappa, X, sm->hblk.data() + (size_t)k * 3 * sm->n_bars);
    sm->K = k + 1;
    return HM_OK;
}

// Pp_{k+1} = F_k P_k F_k^T + Weps into d_Pp, F P into d_FP (slot k must hold P_k)
static void smooth_predict(hm_smooth *sm, int k, hipStream_t st)
{
    SpringTopo tp = {sm->d_off, sm->d_bar, sm->d_other, sm->d_blk + (size_t)k * 3 * sm->n_bars};
    ekf_queue_fpft(st, sm->d_P + (size_t)k * sm->n4 * sm->n4, sm->d_FP, sm->d_Pp, sm->N, tp, sm->a, sm->s, sm->eps_F);
}

static int smooth_upload_blocks(hm_smooth *sm, hipStream_t st)
{
    if (sm->n_bars > 0)
        HM_HIP(hipMemcpyAsync(sm->d_blk, sm->hblk.data(), sm->hblk.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return HM_OK;
}

extern "C" int hm_smooth_prior(hm_smooth_t sm, int k, double *Pp_out)
{
    HM_ARG(sm && Pp_out, "hm_smooth_prior: NULL argument");
    HM_ARG(k >= 1 && k < sm->K, "hm_smooth_prior: frame %d outside 1..%d", k, sm->K - 1);
    if (sm->smoothed_cov) { hm_set_error("hm_smooth_prior: the record has been smoothed with covariances"); return HM_ERR_STATE; }
    hm_ctx *h = sm->ctx;
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = sm->n4;
    HM_TRY(smooth_upload_blocks(sm, h->stream));
    smooth_predict(sm, k - 1, h->stream);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(Pp_out, sm->d_Pp, n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_smooth_fetch(hm_smooth_t sm, int k, double *P_out, double *x_out, double *m_out)
{
    HM_ARG(sm != nullptr, "hm_smooth_fetch: NULL handle");
    HM_ARG(k >= 0 && k < sm->K, "hm_smooth_fetch: frame %d outside 0..%d", k, sm->K - 1);
    hm_ctx *h = sm->ctx;
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = sm->n4;
    if (P_out) HM_HIP(hipMemcpyAsync(P_out, sm->d_P + k * n4 * n4, n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (m_out) HM_HIP(hipMemcpyAsync(m_out, sm->d_m + k * n4, n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    if (x_out) memcpy(x_out, sm->hx.data() + k * n4, n4 * sizeof(double));
    return HM_OK;
}

extern "C" int hm_smooth_run(hm_smooth_t sm, int want_cov, double *xs, double *var)
{
    HM_ARG(sm && xs && (!want_cov || var), "hm_smooth_run: NULL argument");
    if (sm->K < 1) { hm_set_error("hm_smooth_run: nothing recorded"); return HM_ERR_STATE; }
    if (sm->smoothed_cov) { hm_set_error("hm_smooth_run: the record has been smoothed with covariances already"); return HM_ERR_STATE; }
    hm_ctx *h = sm->ctx;
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int n4 = sm->n4, K = sm->K, nb = hm_cdiv(n4, DNB);
    const size_t nn = (size_t)n4 * n4;
    HM_TRY(smooth_upload_blocks(sm, st));
    HM_HIP(hipMemcpyAsync(sm->d_x, sm->hx.data(), (size_t)K * n4 * sizeof(double), hipMemcpyHostToDevice, st));
    HM_HIP(hipMemsetAsync(sm->d_ctl, 0, 4 * sizeof(unsigned), st));
    HM_HIP(hipMemsetAsync(sm->d_flag, 0, sizeof(int), st));
    // the last frame: xs = x, Ps = P
    HM_HIP(hipMemcpyAsync(sm->d_xs + (size_t)(K - 1) * n4, sm->d_x + (size_t)(K - 1) * n4, (size_t)n4 * sizeof(double),
                          hipMemcpyDeviceToDevice, st));
    const int gv = hm_cdiv(n4, 256);
    if (want_cov) {
        sm->smoothed_cov = true;     // (from here on the slots are being overwritten)
        hipLaunchKernelGGL(k_sm_diag, dim3(gv), dim3(256), 0, st, (const double *)(sm->d_P + (K - 1) * nn), sm->d_var + (size_t)(K - 1) * n4, n4);
    }
    double *d = sm->d_vec, *u = sm->d_vec + n4, *w = sm->d_vec + 2 * n4;
    for (int k = K - 2; k >= 0; k--) {
        double *P = sm->d_P + k * nn;
        const double *Ps1 = sm->d_P + (k + 1) * nn;
        smooth_predict(sm, k, st);
        // Pp = L L^T: T = L^-1 (the update's factorisation, one persistent launch)
        FlowArgs fa = {sm->d_Pp, sm->d_L, sm->d_Lt, sm->d_T, sm->d_flowP, n4, n4, nb, nb, sm->d_ctl, 0};
        ekf_queue_chol_flow(st, fa, h->flow_wgs, true);
        hipLaunchKernelGGL(k_sm_check, dim3(gv), dim3(256), 0, st, (const double *)sm->d_T, n4, k + 1, sm->d_flag);
        // xs_k = x_k + (F P)^T T^T T (xs_{k+1} - m_{k+1}): matrix-vector products only
        hipLaunchKernelGGL(k_sm_sub, dim3(gv), dim3(256), 0, st, (const double *)(sm->d_xs + (size_t)(k + 1) * n4),
                           (const double *)(sm->d_m + (size_t)(k + 1) * n4), d, n4);
        hipLaunchKernelGGL(k_sm_trmv, dim3(n4), dim3(256), 0, st, (const double *)sm->d_T, (const double *)d, u, n4);
        hipLaunchKernelGGL(k_sm_mvt, dim3(gv), dim3(256), 0, st, (const double *)sm->d_T, (const double *)u,
                           (const double *)nullptr, w, n4, 1);
        hipLaunchKernelGGL(k_sm_mvt, dim3(gv), dim3(256), 0, st, (const double *)sm->d_FP, (const double *)w,
                           (const double *)(sm->d_x + (size_t)k * n4), sm->d_xs + (size_t)k * n4, n4, 0);
        if (want_cov) {
            // Y = T (F P), G = Y^T T = (F P)^T inv(Pp) through the factor (smooth_kernels.h: not through T^T T),
            // E = G (Ps_{k+1} - Pp), Ps_k = P_k + E G^T in slot k
            hipLaunchKernelGGL(k_sm_gemm<SM_LN>, dim3(nb, nb), dim3(SM_NT), 0, st, (const double *)sm->d_T,
                               (const double *)sm->d_FP, (const double *)nullptr, sm->d_Y, n4);
            hipLaunchKernelGGL(k_sm_gemm<SM_TL>, dim3(nb, nb), dim3(SM_NT), 0, st, (const double *)sm->d_Y,
                               (const double *)sm->d_T, (const double *)nullptr, sm->d_G, n4);
            hipLaunchKernelGGL(k_sm_gemm<SM_NND>, dim3(nb, nb), dim3(SM_NT), 0, st, (const double *)sm->d_G, Ps1,
                               (const double *)sm->d_Pp, sm->d_E, n4);
            hipLaunchKernelGGL(k_sm_gemm<SM_SYM>, dim3(nb, nb), dim3(SM_NT), 0, st, (const double *)sm->d_E,
                               (const double *)sm->d_G, (const double *)P, P, n4);
            hipLaunchKernelGGL(k_sm_diag, dim3(gv), dim3(256), 0, st, (const double *)P, sm->d_var + (size_t)k * n4, n4);
        }
        HM_HIP(hipGetLastError());
    }
    unsigned ctl[4] = {0, 0, 0, 0};
    int flag = 0;
    HM_HIP(hipMemcpyAsync(xs, sm->d_xs, (size_t)K * n4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (want_cov) HM_HIP(hipMemcpyAsync(var, sm->d_var, (size_t)K * n4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HM_HIP(hipMemcpyAsync(ctl, sm->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HM_HIP(hipMemcpyAsync(&flag, sm->d_flag, sizeof flag, hipMemcpyDeviceToHost, st));
    HM_HIP(hipStreamSynchronize(st));
    if (ctl[1]) { hm_set_error("hm_smooth_run: the factorisation launch gave up waiting for a block (chol_flow time-out)"); return HM_ERR_HIP; }
    if (flag) {
        hm_set_error("hm_smooth_run: the predicted covariance Pp of frame %d is not positive definite", flag - 1);   // (k_sm_check: 1 + the frame)
        return HM_ERR_NUMERIC;
    }
    return HM_OK;
}

// The products of the backward step on host arrays (n x n, row-major), for tests: which = SM_TN (out = A^T B),
// SM_NND (out = A (B - C)), SM_SYM (out = C + A B^T from the lower tiles, mirrored), SM_LN (out = tril(A) B),
// SM_TL (out = A^T tril(B)); C is read by SM_NND and SM_SYM only
extern "C" int hm_op_smooth_gemm(int device, int which, int n, const double *A, const double *B, const double *C, double *out)
{
    HM_ARG(which >= SM_TN && which <= SM_TL, "hm_op_smooth_gemm: which %d outside 0..4", which);
    HM_ARG(n >= 1 && n <= 8192, "hm_op_smooth_gemm: n %d outside 1..8192", n);
    HM_ARG(A && B && out && ((which != SM_NND && which != SM_SYM) || C), "hm_op_smooth_gemm: NULL argument");
    HM_HIP(hipSetDevice(device));
    const size_t bytes = (size_t)n * n * sizeof(double);
    double *dA = nullptr, *dB = nullptr, *dC = nullptr, *dO = nullptr;
    const int nb = hm_cdiv(n, DNB);
    auto run = [&]() -> int {
        HM_HIP(hm_malloc((void **)&dA, bytes, 4));
        HM_HIP(hm_malloc((void **)&dB, bytes, 4));
        HM_HIP(hm_malloc((void **)&dO, bytes, 4));
        HM_HIP(hipMemcpy(dA, A, bytes, hipMemcpyHostToDevice));
        HM_HIP(hipMemcpy(dB, B, bytes, hipMemcpyHostToDevice));
        if (which == SM_TN) {
            hipLaunchKernelGGL(k_sm_gemm<SM_TN>, dim3(nb, nb), dim3(SM_NT), 0, 0, (const double *)dA, (const double *)dB,
                               (const double *)nullptr, dO, n);
        } else if (which == SM_LN) {
            hipLaunchKernelGGL(k_sm_gemm<SM_LN>, dim3(nb, nb), dim3(SM_NT), 0, 0, (const double *)dA, (const double *)dB,
                               (const double *)nullptr, dO, n);
        } else if (which == SM_TL) {
            hipLaunchKernelGGL(k_sm_gemm<SM_TL>, dim3(nb, nb), dim3(SM_NT), 0, 0, (const double *)dA, (const double *)dB,
                               (const double *)nullptr, dO, n);
        } else if (which == SM_NND) {
            HM_HIP(hm_malloc((void **)&dC, bytes, 4));
            HM_HIP(hipMemcpy(dC, C, bytes, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_sm_gemm<SM_NND>, dim3(nb, nb), dim3(SM_NT), 0, 0, (const double *)dA, (const double *)dB,
                               (const double *)dC, dO, n);
        } else {                     // in place, as the backward step runs it
            HM_HIP(hipMemcpy(dO, C, bytes, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_sm_gemm<SM_SYM>, dim3(nb, nb), dim3(SM_NT), 0, 0, (const double *)dA, (const double *)dB,
                               (const double *)dO, dO, n);
        }
        HM_HIP(hipGetLastError());
        HM_HIP(hipMemcpy(out, dO, bytes, hipMemcpyDeviceToHost));
        return HM_OK;
    };
    const int rc = run();
    for (double *p : {dA, dB, dC, dO})
        if (p) (void)hipFree(p);
    return rc;
}
