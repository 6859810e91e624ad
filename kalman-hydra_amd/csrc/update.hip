// The dense half of the EKF update on MI355X: host orchestration and C-ABI (include/hydra_mi.h).  In this order: the launch
// sequences the smoother shares (ekf_queue_fpft, ekf_queue_chol_flow), factorisation and solve, the stepwise update
// (hm_update_prefactor / _begin / _step / _cov, hm_cov_fetch), what the next hm_update_run is armed with, hm_update_tail,
// and hm_update_run with its phases.  The kernels are in dense_kernels.h and chol_flow_kernels.h, which this translation unit
// alone compiles.  This is the file that reads across the handle (ctx.h): the measurement is ekf.hip's (render_iter,
// measure_dev, ...), the mask's outline mask.hip's (prepare_mask), the prediction queued ahead predict_dev.hip's
// (queue_predict_ahead), all reached through the hidden functions at the end of ctx.h.  It writes the dense buffers and
// their bookkeeping (d_Wres, upd_*, prefactored, the result blocks), `armed`, `pn`, `tail` and `chain`; of the others'
// state ref / P and d_X / d_Xn (swapped for an iteration), X0 / have_ref, pq.valid / pq.eps_F, newton4.pending (the block
// of a chained prediction has been taken) and last_err*.
#include "ctx.h"
#include "dense_kernels.h"
#include "chol_flow_kernels.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

// the launch sequences the smoother repeats (ctx.h)
void ekf_queue_fpft(hipStream_t st, const double *src, double *FP, double *dst, int N, const SpringTopo &tp, double a, double s,
                    double eps_F)
{
    const dim3 grid(hm_cdiv(4 * N, 256), N);
    hipLaunchKernelGGL(k_fw_rows, grid, dim3(256), 0, st, src, FP, N, tp, a, s);
    hipLaunchKernelGGL(k_pft_cols, grid, dim3(256), 0, st, (const double *)FP, dst, N, tp, a, s, eps_F);
}
void ekf_queue_chol_flow(hipStream_t st, const FlowArgs &a, int wgs, bool fill)
{
    if (fill) hipLaunchKernelGGL(k_flow_fill, dim3(a.nrows + FLOW_FILL_WGS), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_chol_flow, dim3(wgs), dim3(FLOW_NT), 0, st, a);
}

#ifdef HM_STAMP
int update_debug_stamps(long long *dev_ptr)
{
    HM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_chain_stamp), &dev_ptr, sizeof dev_ptr));
    return HM_OK;
}
#endif

// ---- the dense part of the update on the device ----------------------------------------------------
// Layout of a factor buffer d_Af[s]: n4 matrix rows, padding up to a multiple of 32 rows, then one
// 32-row block whose first row carries the right-hand side (see dense_kernels.h).
static int aug_rows(int n) { return hm_cdiv(n, DNB) * DNB + DNB; }

// Cholesky of the n x n matrix in the working copy A (destroyed) into L / Lt, and the inverse of the
// factor into T (M: n x n scratch) -- both from the same launches; with_rhs: the right-hand-side rows
// below the matrix go through the elimination too (dense_kernels.h)
// first_done: Lt[0] is there already (k_assemble)
static void chol_factor(hm_ctx *h, double *A, double *L, double *Lt, double *T, double *M, int n, bool with_rhs,
                        bool first_done = false, hipStream_t st = nullptr)
{
    if (!st) st = h->stream;
    const int nb = hm_cdiv(n, DNB);
    const int nrows = with_rhs ? aug_rows(n) : n;
    const int nbr = hm_cdiv(nrows, DNB);
    if (h->chol_flow) {
        // one persistent launch: the block operations below as tasks that hand their results over through memory
        // (chol_flow_kernels.h); the same bits as the launch-per-step form.  first_done: the caller's assembly pass
        // (k_assemble_flow) has pre-filled the outputs
        ekf_queue_chol_flow(st, FlowArgs{A, L, Lt, T, h->d_flowP, n, nrows, nb, nbr, h->d_flowctl, h->flow_stall}, h->flow_wgs, !first_done);
        return;
    }
    if (!first_done) hipLaunchKernelGGL(k_chol_first, dim3(1), dim3(64), 0, st, A, Lt, n);
    for (int k = 0; k < nb; k++) {
        const int mr = nbr - k - 1, mc = std::max(nb - k - 1, 1);
        // grid: mr block rows below the diagonal (update of A in columns < mc, of the inverse in the k+1
        // columns after them) and one more row that finishes row k of the inverse
        hipLaunchKernelGGL(k_chol_step, dim3((mc + k + 1) * (mr + 1)), dim3(256), 0, st, A, L, Lt, T, M, n, nrows, nb, k, mc, mc + k + 1, mr + 1);
    }
}

// SPD inverse from the inverse T = L^-1 of the factor: inv = T^T T
static void chol_inverse(hm_ctx *h, int n, const double *T, double *out, hipStream_t st = nullptr)
{
    const int nb = hm_cdiv(n, DNB);
    hipLaunchKernelGGL(k_ttt, dim3(nb, nb), dim3(256), 0, st ? st : h->stream, T, n, out);
}

// the time-out word of the persistent factorisation launches since the last hm_update_begin (stream must be idle)
static int flow_status(hm_ctx *h, const char *who)
{
    if (!h->chol_flow) return HM_OK;
    unsigned ctl[2] = {0, 0};
    HM_HIP(hipMemcpyAsync(ctl, h->d_flowctl, sizeof ctl, hipMemcpyDeviceToHost, h->stream));      // (not the null stream: it
    HM_HIP(hipStreamSynchronize(h->stream));                                                         // waits for blocking streams)
    if (ctl[1]) { hm_set_error("%s: the factorisation launch gave up waiting for a block (chol_flow time-out)", who); return HM_ERR_HIP; }
    return HM_OK;
}

// one iteration's worth of launches of the update: system assembly, factorisation, solve.
// d_X holds the iterate the measurement was taken at; returns the step (d_step).
static double *solve_step(hm_ctx *h, int slot, double deltaX)
{
    const int n4 = 4 * h->N;
    double *A = h->d_Awork;
    // A = invW0 + H; the right-hand side Hz - H (X0 - X) as the first row of the block below the
    // matrix; the rows in between and the rest of that block zero
    const int rhs_index = hm_cdiv(n4, DNB) * DNB;
    double *rhs_row = A + (size_t)rhs_index * n4;
    {   // one pass from the job sums of the measurement: A, the right-hand side, Hz / Hzc, and the pre-fill of what
        // the persistent factorisation launch produces (harmless for the launch-per-step form, which overwrites it)
        const int nb = hm_cdiv(n4, DNB), nrows = aug_rows(n4);
        PrepArgs p;
        p.out = h->d_out; p.N = h->N; p.vsplit = h->vsplit; p.esplit = h->esplit;
        p.eZ = h->eps_Z; p.eJ = h->eps_J; p.eM = h->eps_M; p.d = deltaX;
        p.nb_off = h->d_nb_off; p.nb_u = h->d_nb_u; p.nb_e = h->d_nb_e;
        p.invW0 = h->d_invW0; p.X0 = h->d_X0; p.X = h->d_X;
        p.A = A; p.Hz = h->d_Hz; p.Hzc = h->d_Hzc; p.n = n4; p.rhs_row = rhs_index;
        p.f = FlowArgs{A, h->d_Af[slot], h->d_Lt[slot], h->d_T[slot], h->d_flowP, n4, nrows, nb, hm_cdiv(nrows, DNB), h->d_flowctl, 0};
        hipLaunchKernelGGL(k_solve_prep, dim3(nrows + FLOW_FILL_WGS), dim3(256), 0, h->stream, p);
    }
    if (h->d_Wres == h->d_Wtmp) h->d_Wres = nullptr;          // a covariance predicted since hm_update_begin is lost
    chol_factor(h, A, h->d_Af[slot], h->d_Lt[slot], h->d_T[slot], h->d_Wtmp, n4, true, h->chol_flow != 0);
    // y = L^-1 b came out of the factorisation as the extra row and T = L^-1 with it (d_Wtmp was the
    // scratch: it is free between hm_update_begin and the next hm_cov_predict); x = T^T y.  T stays in the
    // slot for hm_update_cov (inv = T^T T).
    const double *yrow = h->d_Af[slot] + (rhs_row - A);
    hipLaunchKernelGGL(k_tvec, dim3(hm_cdiv(n4, TV_COLS)), dim3(TV_COLS * TV_ROWS), 0, h->stream, h->d_T[slot], n4, yrow, h->d_step, h->d_X0,
                       h->d_Xn);                              // also d_Xn = X0 + step
    return h->d_step;
}

// the covariance half of hm_update_begin: the prior into d_Wprior, its factor, inv(W) into d_invW0 (ctx.h)
int prior_inverse(hm_ctx *h, const double *W_prior, hipStream_t st)
{
    if (!st) st = h->stream;
    const int n4 = 4 * h->N;
    // the prior stays in d_Wprior: it is the covariance to keep when no iterate is accepted
    const size_t nnb = (size_t)n4 * n4 * sizeof(double);
    if (W_prior)
        HM_HIP(hipMemcpyAsync(h->d_Wprior, W_prior, nnb, hipMemcpyHostToDevice, st));
    else if (h->d_Wres != h->d_Wprior)
        HM_HIP(hipMemcpyAsync(h->d_Wprior, h->d_Wres, nnb, hipMemcpyDeviceToDevice, st));
    // the launch-per-step factorisation destroys its input: it gets a copy; the persistent launch only reads it
    if (!h->chol_flow) HM_HIP(hipMemcpyAsync(h->d_Awork, h->d_Wprior, nnb, hipMemcpyDeviceToDevice, st));
    h->d_Wres = h->d_Wprior;                     // d_Wtmp is scratch from here on
    HM_HIP(hipMemsetAsync(h->d_flowctl, 0, 4 * sizeof(unsigned), st));      // a new sequence of factorisations
    chol_factor(h, h->chol_flow ? h->d_Wprior : h->d_Awork, h->d_Af[0], h->d_Lt[0], h->d_Wtmp, h->d_invW0, n4, false, false, st);    // T in d_Wtmp
    chol_inverse(h, n4, h->d_Wtmp, h->d_invW0, st);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// Start the covariance half of the next hm_update_begin / hm_update_run(h, NULL, ...) now: the
// factorisation and inversion of the covariance resident on the device are queued and the call
// returns.  They need the predicted covariance only, not the predicted state, so a caller whose
// state prediction runs on the host (hm_ms_newton) overlaps the two.
extern "C" int hm_update_prefactor(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_update_prefactor: NULL handle");
    HM_JOIN(h);
    if (!h->d_Wres) { hm_set_error("hm_update_prefactor: no covariance resident on the device"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    h->pq.valid = false;
    // (launched one by one: replaying this series as a hipGraph saved 0.08 ms of host time per frame, but
    // graph replays proved unreliable next to allocations by the caller -- see hm_brox_tune "graph")
    // With the factorisation as one persistent launch this is a copy, a fill and three launches: queued right here
    // (a helper thread started per call had them reach the device ~0.2 ms later -- thread start-up and the first
    // runtime calls of a new thread -- and the first measurement of the frame waited for them: kernel trace of the
    // bench, tools/frame_gap_timeline.py).
    if (h->chol_flow) {
        const int rc = prior_inverse(h, nullptr);
        if (rc == HM_OK) {
            h->prefactored = true;
            h->upd_open = false;                  // the factor slots are being reused
        }
        return rc;
    }
    // The launch-per-step form: queueing its ~30 launches takes the host about as long as the state prediction the
    // caller does next (hm_ms_newton): a helper thread does it, and whatever is called next on this handle joins it.
    h->worker_active = true;
    h->worker = std::thread([h]() {
        int rc = hipSetDevice(h->device) == hipSuccess ? HM_OK : HM_ERR_HIP;
        if (rc == HM_OK) rc = prior_inverse(h, nullptr);
        if (rc == HM_OK) {
            h->prefactored = true;
            h->upd_open = false;                  // the factor slots are being reused
        } else {
            snprintf(h->worker_err, sizeof h->worker_err, "hm_update_prefactor: %s", hm_last_error());
        }
        h->worker_rc = rc;
    });
    return HM_OK;
}

// hm_update_begin behind its argument checks.  X0 == NULL: the prior mean is being left in d_X0 by hm_chain_project's kernel
// (mask.ev_pm says when)
static int update_begin(hm_ctx *h, const double *W_prior, const double *X0)
{
    if (!W_prior && !h->d_Wres) {
        hm_set_error("hm_update_begin: no prior given and none resident on the device");
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    const int n4 = 4 * h->N;
    h->pq.valid = false;                         // (a prediction queued ahead that nobody took: d_Wres is still the posterior)
    const bool taken = h->prefactored && !W_prior && h->d_Wres == h->d_Wprior;
    if (!taken) {
        HM_TRY(ctx_join(h));                     // (the tail of the last update is rewriting what prior_inverse rewrites)
        HM_TRY(prior_inverse(h, W_prior));
    }
    h->prefactored = false;
    if (X0) {
        h->upd_X0.assign(X0, X0 + n4);
        HM_HIP(hipMemcpyAsync(h->d_X0, h->upd_X0.data(), (size_t)n4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        HM_HIP(hipStreamWaitEvent(h->stream, h->mask.ev_pm, 0));
    }
    h->upd_last = h->upd_prev = -1;
    h->upd_open = true;
    return HM_OK;
}
extern "C" int hm_update_begin(hm_ctx_t h, const double *W_prior, const double *X0)
{
    HM_ARG(h && X0, "hm_update_begin: NULL argument");
    HM_JOIN(h);
    h->chain.pending = false;
    return update_begin(h, W_prior, X0);
}

extern "C" int hm_update_step(hm_ctx_t h, const double *X, double deltaX, int masked, double *step, double *Hzc,
                              double err[4])
{
    HM_ARG(h && X && step, "hm_update_step: NULL argument");
    HM_JOIN(h);
    HM_ARG(deltaX > 0, "hm_update_step: deltaX must be positive");
    if (!h->upd_open) { hm_set_error("hm_update_step: hm_update_begin has not been called"); return HM_ERR_STATE; }
    NEED_TEX(h, "hm_update_step");
    NEED_OBS(h, "hm_update_step");
    HM_HIP(hipSetDevice(h->device));
    const int n4 = 4 * h->N;
    const int slot = h->upd_last == 0 ? 1 : 0;
    HM_TRY(with_pool_retry(h, "hm_update_step", [&]() -> int {
        HM_TRY(measure_on_device(h, X, deltaX, masked, false));   // leaves X in d_X; the job sums go straight into the system
        double *rhs_row = solve_step(h, slot, deltaX);
        HM_HIP(hipGetLastError());
        HM_HIP(hipMemcpyAsync(step, rhs_row, (size_t)n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Hzc) HM_HIP(hipMemcpyAsync(Hzc, h->d_Hzc, (size_t)n4 * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HM_TRY(pool_flag_queue(h));
        if (!err) {
            HM_HIP(hipStreamSynchronize(h->stream));
            return HM_OK;
        }
        // Renderer.error of the new iterate X0 + step, without another host round trip: the launch and the order of
        // additions hm_update_run uses.  Nothing of this call stays in flight when it fails.
        const int rc = render_iter(h, h->d_Xn, h->P, true, masked, false, deltaX);
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
        return render_error_sums(h, "hm_update_step", err);
    }));
    HM_TRY(flow_status(h, "hm_update_step"));
    h->upd_prev = h->upd_last;
    h->upd_last = slot;
    return HM_OK;
}

// hm_update_cov on stream st: hm_update_run's tail queues it on a stream of its own
static int update_cov_on(hm_ctx *h, int which, double *W_out, hipStream_t st)
{
    HM_ARG(which >= -1 && which <= 1, "hm_update_cov: which must be 0 (last step), 1 (the step before) or -1 (the prior)");
    if (!h->upd_open) { hm_set_error("hm_update_cov: hm_update_begin has not been called"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    const int n4 = 4 * h->N;
    if (which < 0) {
        h->d_Wres = h->d_Wprior;
    } else {
        const int slot = which == 0 ? h->upd_last : h->upd_prev;
        if (slot < 0) { hm_set_error("hm_update_cov: no such step"); return HM_ERR_STATE; }
        {   // T of this slot is there since its solve: inv = T^T T
            const int nb = hm_cdiv(n4, DNB);
            hipLaunchKernelGGL(k_ttt, dim3(nb, nb), dim3(256), 0, st, h->d_T[slot], n4, h->d_H);
        }
        HM_HIP(hipGetLastError());
        h->d_Wres = h->d_H;
    }
    if (W_out) {
        HM_HIP(hipMemcpyAsync(W_out, h->d_Wres, (size_t)n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HM_HIP(stream_wait(st));
    }
    return HM_OK;
}
extern "C" int hm_update_cov(hm_ctx_t h, int which, double *W_out)
{
    HM_ARG(h != nullptr, "hm_update_cov: NULL handle");
    HM_JOIN(h);
    return update_cov_on(h, which, W_out, h->stream);
}

// The covariance resident on the device (the result of the last hm_cov_predict, hm_update_cov or
// hm_update_run) copied to the host.
extern "C" int hm_cov_fetch(hm_ctx_t h, double *W_out)
{
    HM_ARG(h && W_out, "hm_cov_fetch: NULL argument");
    HM_JOIN(h);
    if (!h->d_Wres) { hm_set_error("hm_cov_fetch: no covariance resident on the device"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = (size_t)4 * h->N;
    HM_HIP(hipMemcpyAsync(W_out, h->d_Wres, n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// ---- what the next hm_update_run on the handle is armed with (Armed, ctx.h), and the tail block it leaves ------------------
// one-shot: when the next hm_update_run has its final state it starts the next frame's state prediction from it on
// `worker` (hm_ms_newton_start, predict.cpp) with these springs and parameters
extern "C" int hm_update_arm_newton(hm_ctx_t h, void *worker, int n_bars, const int32_t *bars, const double *l0, double kappa,
                                    double M, double dt, int maxiter, double tol)
{
    HM_ARG(h && worker && n_bars >= 0 && bars && l0, "hm_update_arm_newton: bad argument");
    HM_JOIN_LAZY(h);                               // (the tail of the last update still reads what this call replaces)
    h->armed.worker = worker;
    h->pn.bars.assign(bars, bars + 2 * (size_t)n_bars);
    h->pn.l0.assign(l0, l0 + n_bars);
    h->pn.par[0] = kappa; h->pn.par[1] = M; h->pn.par[2] = dt; h->pn.par[3] = tol;
    h->pn.maxiter = maxiter;
    h->armed.newton = true;
    return HM_OK;
}

// With hm_update_arm_newton armed as well: the next hm_update_run also queues the covariance half of the next frame's
// prediction (queue_predict_ahead, predict_dev.hip; eps_F as for hm_cov_predict) behind the covariance of the state it keeps.
// hm_update_cov is not available after such a run (the factor slots are reused); hm_cov_fetch still returns the
// posterior until hm_predict_take.
extern "C" int hm_update_arm_cov(hm_ctx_t h, double eps_F)
{
    HM_ARG(h != nullptr, "hm_update_arm_cov: NULL handle");
    h->armed.cov = true;
    h->pq.eps_F = eps_F;
    return HM_OK;
}


// one-shot: when the next hm_update_run on h has its final state it also queues hm_prepare_mask(h, d_y_m) -- the contour
// pruning and outline of the NEXT frame's mask run beside the state prediction and the update's tail instead of at the
// start of the next frame, where the projection would wait for them
extern "C" int hm_update_arm_mask(hm_ctx_t h, const uint8_t *d_y_m)
{
    HM_ARG(h != nullptr, "hm_update_arm_mask: NULL handle");
    h->armed.mask = d_y_m;
    return HM_OK;
}

// Hz components (4N x 4) and gains (3 x 4N) of the last hm_update_run that was called with Hzc = gains = NULL (such a
// call does not wait for the kernels that form them: the caller gets on with the next frame); either may be NULL.
// Available until the next hm_update_run on h; zeros for an update without iterations.  HM_ERR_STATE when the last
// hm_update_run failed or there was none: its tail is not what the caller asks for.
extern "C" int hm_update_tail(hm_ctx_t h, double *Hzc, double *gains)
{
    HM_ARG(h != nullptr, "hm_update_tail: NULL handle");
    HM_JOIN_LAZY(h);                               // (the helper thread may still be queueing the kernels that form them)
    if (!h->tail.valid) {
        hm_set_error("hm_update_tail: the last hm_update_run on this handle did not succeed (or there was none)");
        return HM_ERR_STATE;
    }
    const size_t n4 = (size_t)4 * h->N;
    if (h->tail.pending) {
        HM_HIP(hipSetDevice(h->device));
        HM_TRY(hb_wait(h->tail.stream, h->pin + 2 * (n4 + RES_HEAD), 0, n4 * 7, hb_stamp(h->tail.ticket), h->tail.v.data(), "hm_update_tail"));
        h->tail.pending = false;
    }
    if (Hzc) memcpy(Hzc, h->tail.v.data(), n4 * 4 * sizeof(double));
    if (gains) memcpy(gains, h->tail.v.data() + n4 * 4, n4 * 3 * sizeof(double));
    return HM_OK;
}

// ---- hm_update_run: the state of one call, its phases, the driver ---------------------------------------------------------
struct UpdateArgs {
    const double *W_prior;
    double *X;
    double deltaX;
    int masked, max_iter;
    double reltol;
    double *errs, *Hzc, *gains, *W_out;
};
struct UpdateRun {
    hm_ctx *const h;
    const UpdateArgs a;
    // What hm_update_arm_newton / _arm_cov / _arm_mask armed is for THIS call only: taken out of the handle before anything
    // can fail (constructing this is the first thing hm_update_run does with a handle that is not NULL), so that an error
    // return never leaves a worker pointer or a mask address behind for a later call to start a job on (the helper thread
    // joined in update_enter touches none of these fields).
    const Armed armed;
    const uint8_t *next_mask;        // the armed mask as long as its outline is still to be queued
    const int n4;
    // hm_chain_project: the prior mean is being left in d_X0 by the kernels of the state path, X is output only; collected:
    // the host has what those kernels report (chain_collect) -- X0 / Xcur / Xold are empty until then
    bool chained = false, collected = false;
    std::vector<double> X0, Xcur, Xold;          // the prior mean, the iterate, the last iterate that was accepted
    int niter = 0, accepted = 0;
    bool reverted = false, conv = false;
    bool ref_ready = false;          // h->ref holds the render of the iterate in d_X
    bool regions_ahead = false;      // the iteration in flight has the star regions of the next measurement computed with its render
    // The measurement at the new iterate has been queued already -- behind k_iter_result, before the host has seen that
    // iteration's result, on the assumption that the loop goes on (it does 7 times out of 8): the device goes from one
    // iteration into the next without the ~14 us it takes the host to notice the result block, decide and launch.  ref / P
    // and d_X / d_Xn are swapped when it is queued (SpecSwap); an iteration that turns out to be the last swaps them back
    // (the wasted measurement only wrote job sums and parked differences nobody reads, and the launches behind it on this
    // stream -- the covariance of the kept state -- are not what the next frame waits for).
    bool measured_ahead = false;
    bool grown = false;              // the pool has been grown for the iteration in flight: it does not overflow twice
    double eold = 0.0;
    int slot = 0;                    // the factor slot of the iteration in flight
    // HYDRA_MI_TRACE, read once per call (update_enter); the stage clock (ms since update_enter had the handle to itself),
    // the moment an iteration's launches were queued
    bool dbg = false;
    std::chrono::steady_clock::time_point t_enter, t_queued;
    double stage[5] = {0, 0, 0, 0, 0};

    UpdateRun(hm_ctx *h, const UpdateArgs &a)
        : h(h), a(a), armed(std::exchange(h->armed, {})), next_mask(armed.mask), n4(4 * h->N) {}
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enter).count(); }
    const double *res() const { return h->resv.data(); }      // this call's copy of an iteration's block, taken when whole
    double *pin_tail() const { return h->pin + 2 * ((size_t)n4 + RES_HEAD); }
};

// ref / P and d_X / d_Xn of the handle swapped for the length of one iteration: set() when the next measurement is queued
// ahead, keep() when the iteration ends in "go on with the next one" -- the new iterate becomes the point of the next
// measurement and its render is already there: swapped once, now or by set(), and left so.  Every other way out of the
// iteration -- converged, reverted, an overflow (undo(), before anything else is queued), any error return -- puts them back.
struct SpecSwap {
    hm_ctx *const h;
    bool swapped = false;
    explicit SpecSwap(hm_ctx *h) : h(h) {}
    SpecSwap(const SpecSwap &) = delete;
    SpecSwap &operator=(const SpecSwap &) = delete;
    ~SpecSwap() { undo(); }
    void flip() { std::swap(h->ref, h->P); std::swap(h->d_X, h->d_Xn); }
    void set() { flip(); swapped = true; }
    void undo() { if (swapped) flip(); swapped = false; }
    void keep() { if (!swapped) flip(); swapped = false; }
};

// chained: what the prediction's and the projection's kernels report (host_block.h), waited for on the host while the
// first iteration runs; leaves X0 / Xcur / Xold and the handle's copies of them.  2: the prediction's inner solve gave up
// (never observed) -- the caller predicts on the host and calls again.
static int chain_collect(UpdateRun &u)
{
    hm_ctx *h = u.h;
    const int n4 = u.n4;
    int r = hb_wait(h->newton4.stream, h->newton4.pin + n4, 0, (size_t)n4 + 2, hb_stamp(h->newton4.ticket), h->newton4.v.data(), "hm_update_run (state prediction)");
    h->newton4.pending = false;
    if (r) return r;
    HM_TRY(hb_wait(h->newton4.stream, h->mask.pin + n4, 0, (size_t)n4 + 1, hb_stamp(h->mask.ticket), h->mask.v.data(), "hm_update_run (projectmask)"));
    h->chain.pred.assign(h->newton4.v.begin(), h->newton4.v.begin() + n4);
    h->chain.proj.assign(h->mask.v.begin(), h->mask.v.begin() + n4);
    h->chain.its = (int)h->newton4.v[n4];
    h->chain.moved = (int)h->mask.v[n4];
    if (h->newton4.v[n4 + 1] != 0.0) return 2;
    u.X0 = h->chain.proj; u.Xcur = u.X0; u.Xold = u.X0;
    h->upd_X0 = u.X0;
    h->X0 = u.X0;
    u.collected = true;
    return HM_OK;
}

// Entry (u.armed is out of the handle already).  Stops the tail block of the last update being handed out, joins the helper
// thread, clears what the last update and the calls since left pending; then queues hm_update_begin's launches and, unless
// chained, the copy of the prior mean into the first iterate.  Waits for nothing on the device.
static int update_enter(UpdateRun &u)
{
    hm_ctx *h = u.h;
    h->tail.valid = false;
    HM_JOIN_LAZY(h);                               // (the tail of the last update: waited for before the first solve)
    HM_ARG(u.a.deltaX > 0 && u.a.max_iter >= 0, "hm_update_run: deltaX must be positive, max_iter >= 0");
    u.chained = h->chain.pending;
    h->chain.pending = false;
    h->last_err_valid = false;
    h->pq.valid = false;                           // (after the join: the last update's tail may have queued a prediction)
    h->tail.pending = false;                       // (the block of the last update is about to be overwritten)
    NEED_TEX(h, "hm_update_run");
    NEED_OBS(h, "hm_update_run");
    u.dbg = getenv("HYDRA_MI_TRACE") != nullptr;
    u.t_enter = std::chrono::steady_clock::now();
    HM_TRY(update_begin(h, u.a.W_prior, u.chained ? nullptr : u.a.X));
    u.stage[0] = u.ms();
    u.collected = !u.chained;
    // (chained: the projection's kernel has written the first iterate, d_X, next to the prior mean)
    if (!u.chained) {
        u.X0.assign(u.a.X, u.a.X + u.n4); u.Xcur = u.X0; u.Xold = u.X0;
        HM_HIP(hipMemcpyAsync(h->d_X, h->d_X0, (size_t)u.n4 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    return HM_OK;
}

// Queues iteration `it` on the handle's stream and waits for nothing: the measurement at d_X unless the last iteration
// queued it ahead; on iteration 0 the ev_m0 record when a mask is armed; the join with the last update's tail; the system
// and its solve (d_Xn = the new iterate); the render of the new iterate with its error sums and the star regions of the
// next measurement; the result block; and, ahead of that block's arrival, the next measurement with the swap.
static int update_queue_iteration(UpdateRun &u, int it, SpecSwap &swap)
{
    hm_ctx *h = u.h;
    if (!u.measured_ahead) HM_TRY(measure_dev(h, h->d_X, u.ref_ready, u.a.deltaX, u.a.masked, u.regions_ahead, false));
    u.measured_ahead = false;
    if (u.next_mask && it == 0) {
        // The next frame's mask (hm_update_arm_mask): its pruning and outline (~0.2 ms of kernels on the second
        // stream) start when this frame's first measurement has run -- beside the first factorisation, which leaves
        // the chip idle -- not beside the first render and measurement, and not in the window between two frames,
        // where they slowed the state prediction's one workgroup down (0.33 instead of 0.27 ms)
        // (the event now; the launches when this iteration's own launches are queued and the host has nothing to do
        // but wait (update_meanwhile): eight launches here kept the first system of the frame waiting for the host,
        // ~17 us per iteration on average in the kernel trace)
        HM_HIP(h->own.event(&h->ev_m0));
        HM_HIP(hipEventRecord(h->ev_m0, h->stream));
    }
    if (u.collected) h->X0 = u.Xcur;               // the state of the reference render (hm_jz / hm_j)
    h->have_ref = true;
    u.slot = h->upd_last == 0 ? 1 : 0;
    HM_TRY(ctx_join(h));                           // the tail of the last update may still be writing inv(W) and the factor slots
    double *rhs_row = solve_step(h, u.slot, u.a.deltaX);
    // the new iterate: its render, the partial sums of Renderer.error (kalman.py:813) and, as extra workgroups of
    // the same launch, the star regions of the next measurement (they need the new iterate only; wasted when the
    // loop ends here)
    u.regions_ahead = it + 1 < u.a.max_iter;
    HM_TRY(render_iter(h, h->d_Xn, h->P, true, u.a.masked, u.regions_ahead, u.a.deltaX));
    hipLaunchKernelGGL(k_iter_result, dim3(1), dim3(256), 0, h->stream, rhs_row, u.n4, h->d_tpart,
                       render_strips(h), h->pool.overflow, (const unsigned *)h->d_flowctl, h->pin, (double)(++h->run_ticket),
                       h->result_delay);
    HM_HIP(hipGetLastError());
    if (h->speculate && u.regions_ahead) {
        swap.set();
        u.measured_ahead = true;
        HM_TRY(measure_dev(h, h->d_X, true, u.a.deltaX, u.a.masked, true, false));
    }
    u.t_queued = std::chrono::steady_clock::now();
    return HM_OK;
}

// What the host does while the device works on iteration `it`: the armed mask's launches on the second stream, behind
// ev_m0 (iteration 0), and the result blocks of a chained prior (chain_collect, which waits for them; when that fails the
// stream is waited for, so that nothing of this call stays in flight).
static int update_meanwhile(UpdateRun &u, int it)
{
    hm_ctx *h = u.h;
    if (u.next_mask && it == 0) {
        HM_TRY(ensure_stream2(h));
        HM_HIP(hipStreamWaitEvent(h->stream2, h->ev_m0, 0));
        HM_TRY(prepare_mask(h, u.next_mask));
        u.next_mask = nullptr;
    }
    if (!u.collected) {
        const int rc = chain_collect(u);
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    }
    return HM_OK;
}

// Waits for the iteration's result block (hb_wait) and counts the iteration -- or, when its star regions did not fit the
// pool of difference images, undoes the swap, waits for the stream, grows the pool and asks for the iteration again
// (nothing of it has been kept; the regions the failed pass computed for its -- meaningless -- next iterate are computed anew).
enum class Taken { go_on, retry };
static int update_take_result(UpdateRun &u, int it, SpecSwap &swap, Taken *out)
{
    hm_ctx *h = u.h;
    const int n4 = u.n4;
    HM_TRY(hb_wait(h->stream, h->pin, 0, (size_t)n4 + RES_HEAD, hb_stamp(h->run_ticket), h->resv.data(), "hm_update_run"));
    if (u.dbg) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u.t_queued).count();
        if (ms > 1.5) fprintf(stderr, "[hydra_mi] hm_update_run: iteration %d waited %.2f ms for its result\n", it, ms);
    }
    if (u.res()[n4 + 4] == 0.0) {
        u.grown = false;
        h->upd_prev = h->upd_last;
        h->upd_last = u.slot;
        u.niter++;
        *out = Taken::go_on;
        return HM_OK;
    }
    swap.undo();
    u.measured_ahead = false;
    if (u.grown) { hm_set_error("hm_update_run: the star regions do not fit the difference-image pool"); return HM_ERR_STATE; }
    if (u.regions_ahead) {
        // d_area no longer describes the measurement that overflowed: this iteration's render launch has put the
        // regions of its (meaningless) new iterate there.  Those of the iterate that was measured, again:
        HM_TRY(queue_star_regions(h, h->d_X, u.a.deltaX, u.a.masked));
    }
    HM_HIP(hipStreamSynchronize(h->stream));
    HM_TRY(pool_grow(h, "hm_update_run"));
    u.grown = true;
    u.regions_ahead = false;
    HM_HIP(hipMemsetAsync(h->d_flowctl, 0, 4 * sizeof(unsigned), h->stream));      // (a NaN system may have timed out)
    *out = Taken::retry;
    return HM_OK;
}

// The reference's acceptance logic on the block just taken (host arithmetic only): the time-out word and the finite check
// (errors), Xcur = X0 + step, errs, a flipped triangle (back to the last good state), the truncated error norm and the
// reltol test.  go_on leaves the new iterate as the point of the next measurement (the caller keeps the swap).
enum class Verdict { go_on, reverted, converged };
static int update_judge(UpdateRun &u, int it, Verdict *out)
{
    hm_ctx *h = u.h;
    const int n4 = u.n4;
    const double *res = u.res();
    if (res[n4 + 7] != 0.0) {
        hm_set_error("hm_update_run: the factorisation launch gave up waiting for a block (chol_flow time-out)");
        return HM_ERR_HIP;
    }
    bool finite = true;
    for (int i = 0; i < n4; i++) finite = finite && std::isfinite(res[i]);
    if (!finite) {
        hm_set_error("hm_update_run: the update system inv(W) + HTH is not positive definite "
                     "(non-finite state, covariance or observation?)");
        return HM_ERR_NUMERIC;
    }
    for (int i = 0; i < n4; i++) u.Xcur[i] = u.X0[i] + res[i];
    if (u.a.errs) for (int k = 0; k < 4; k++) u.a.errs[4 * it + k] = res[n4 + k];
    // a triangle that flipped: back to the last good state (kalman.py:806-811)
    bool flipped = false;
    for (int t = 0; t < h->T && !flipped; t++) {
        const int a = h->tri[3 * t], b = h->tri[3 * t + 1], c = h->tri[3 * t + 2];
        const double ax = u.Xcur[2 * b] - u.Xcur[2 * a], ay = u.Xcur[2 * b + 1] - u.Xcur[2 * a + 1];
        const double bx = u.Xcur[2 * c] - u.Xcur[2 * a], by = u.Xcur[2 * c + 1] - u.Xcur[2 * a + 1];
        flipped = ax * by - ay * bx < 0.0;
    }
    if (flipped) {
        u.Xcur = u.Xold;
        u.reverted = true;
        *out = Verdict::reverted;
        return HM_OK;
    }
    // the error sums of the image and mask terms are whole numbers (the reference truncates
    // them to int before combining, kalman.py:813-816)
    const double e_im = std::trunc(res[n4]), e_m = std::trunc(res[n4 + 3]);
    const double enew = std::sqrt(e_im * e_im + res[n4 + 1] * res[n4 + 1] + res[n4 + 2] * res[n4 + 2] + e_m * e_m);
    u.accepted++;
    if (std::fabs(enew - u.eold) / enew < u.a.reltol) {
        u.conv = true;
        *out = Verdict::converged;
        return HM_OK;
    }
    u.eold = enew;
    u.Xold = u.Xcur;
    u.ref_ready = true;
    h->X0 = u.Xcur;
    *out = Verdict::go_on;
    return HM_OK;
}

// The state is final (Xcur): collects a chained prior that no iteration collected (max_iter = 0), and a caller that armed
// it gets the next frame's state prediction started now, on its worker thread, beside the covariance launches of the tail
// (hm_update_arm_newton).
static int update_state_final(UpdateRun &u)
{
    hm_ctx *h = u.h;
    if (!u.collected) HM_TRY(chain_collect(u));
    u.stage[1] = u.ms();
    if (u.armed.newton)
        HM_TRY(hm_ms_newton_start(u.armed.worker, h->N, (int)h->pn.l0.size(), h->pn.bars.data(), h->pn.l0.data(), h->pn.par[0],
                                  h->pn.par[1], h->pn.par[2], h->pn.maxiter, h->pn.par[3], u.Xcur.data()));
    u.stage[2] = u.ms();
    return HM_OK;
}

// The launches of the tail over a plain struct of values: the helper thread runs them after hm_update_run has returned, so
// its closure holds a copy of this struct and of Xk, the state that is kept, and refers to nothing of the call's frame.
struct TailJob {
    hm_ctx *h;
    const uint8_t *next_mask;        // an armed mask no iteration has queued (an update without iterations)
    int which;                       // hm_update_cov's: -1 the prior, 0 the last step, 1 the step before
    hipStream_t ts;
    int niter, n4;
    double *pin_tail;
    long long ticket;
    double *W_out;
    bool ahead;                      // queue the covariance half of the next frame's prediction (hm_update_arm_cov)
    double eps_F;
};
// On ts: the covariance of the kept state; with iterations the gains and the tail's result block; the copy to W_out; the
// prediction ahead; on tail.stream4 the tail.ev record.  Before them, on the second stream, the next frame's outline.  Waits
// for nothing.
static int tail_launches(const TailJob &j, const std::vector<double> &Xk)
{
    hm_ctx *h = j.h;
    const int n4 = j.n4;
    HM_HIP(hipSetDevice(h->device));
    if (j.next_mask) HM_TRY(prepare_mask(h, j.next_mask));       // the next frame's outline, beside the prediction (hm_update_arm_mask)
    HM_TRY(update_cov_on(h, j.which, nullptr, j.ts));
    if (j.niter > 0) {
        // gains and Hz components go to the host as a result block of their own (host_block.h), as the iterations'
        // results do: two blit launches and the wake-up from a stream synchronisation less per frame
        hipLaunchKernelGGL(k_gains, dim3(n4), dim3(256), 0, j.ts, h->d_Wres, h->d_Hzc, n4, h->d_gain);
        hipLaunchKernelGGL(k_tail_result, dim3(1), dim3(1024), 0, j.ts, h->d_Hzc, h->d_gain, n4, j.pin_tail, (double)j.ticket,
                           h->result_delay);
    }
    if (j.W_out) HM_HIP(hipMemcpyAsync(j.W_out, h->d_Wres, (size_t)n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, j.ts));
    HM_HIP(hipGetLastError());
    if (j.ahead)                                   // behind the launches above (hm_update_arm_cov)
        HM_TRY(queue_predict_ahead(h, Xk.data(), (int)h->pn.l0.size(), h->pn.bars.data(), h->pn.l0.data(), h->pn.par[0],
                                   h->pn.par[1], h->pn.par[2], j.eps_F, j.ts));
    if (j.ts != h->stream) {
        HM_HIP(hipEventRecord(h->tail.ev, j.ts));
        h->tail.on_stream4 = true;
    }
    return HM_OK;
}

// The tail: the covariance of the state that is kept (kalman.py:806-811, 826), the gains, the prediction ahead.  Chooses
// the slot and the stream, takes the ticket, queues the launches (itself or through the helper thread) and hands the
// tail's block out in one of three ways: deferred to hm_update_tail, waited for here (hb_wait), or after the stream has
// been waited for when the caller wants the covariance on the host.
static int update_tail(UpdateRun &u)
{
    hm_ctx *h = u.h;
    const int n4 = u.n4;
    int which = -1;                                // -1: the prior
    if (u.reverted) which = u.accepted == 0 ? -1 : 1;
    else which = u.niter == 0 ? -1 : 0;
    // The tail runs on a stream of its own (tail.stream4) when the caller does not want the covariance on the host: everything
    // it reads is complete -- the host has seen the result block of the last iteration, whose kernel is behind all of
    // them on `stream` -- and what is still queued on `stream` (the measurement of an iteration that does not happen)
    // and what the next frame queues there first (reference render, measurement) touch none of its buffers; `stream` waits
    // for its end (tail.ev, on the device) before the next solve (ctx_join).
    hipStream_t ts = h->stream;
    HM_TRY(ctx_join(h));                           // (a tail nobody has joined since: an update without iterations)
    if (!u.a.W_out && h->tail.split) {
        HM_HIP(h->own.stream(&h->tail.stream4));
        HM_HIP(h->own.event(&h->tail.ev));
        ts = h->tail.stream4;
    }
    const long long ticket = u.niter > 0 ? ++h->run_ticket : h->run_ticket;
    const bool ahead = u.armed.cov && u.armed.newton && h->chol_flow && which >= 0 && u.niter > 0 && !u.a.W_out;
    const TailJob job = {h, u.next_mask, which, ts, u.niter, n4, u.pin_tail(), ticket, u.a.W_out, ahead, h->pq.eps_F};
    u.stage[3] = u.ms();
    if (u.niter > 0 && !u.a.W_out && !u.a.Hzc && !u.a.gains) {
        // nobody wants the gains now: they are taken when asked for (hm_update_tail) and the caller gets on with its next
        // frame -- the tail's ~20 launches are queued by the handle's helper thread (every entry point joins it first)
        h->tail.pending = true;
        h->tail.ticket = ticket;
        h->tail.stream = ts;
        if (h->tail.async) {
            h->helper_used = true;
            h->helper.post([job, Xk = u.Xcur]() { return tail_launches(job, Xk); });
        } else {
            HM_TRY(tail_launches(job, u.Xcur));
        }
    } else if (u.niter > 0 && !u.a.W_out) {
        HM_TRY(tail_launches(job, u.Xcur));
        HM_TRY(hb_wait(ts, job.pin_tail, 0, (size_t)n4 * 7, hb_stamp(ticket), h->tail.v.data(), "hm_update_run"));
    } else {
        HM_TRY(tail_launches(job, u.Xcur));
        HM_HIP(stream_wait(ts));
        if (u.niter > 0 && !hb_take(job.pin_tail, 0, (size_t)n4 * 7, hb_stamp(ticket), h->tail.v.data())) {
            hm_set_error("hm_update_run: the gains did not arrive although the stream has completed");
            return HM_ERR_HIP;
        }
    }
    u.stage[4] = u.ms();
    if (u.dbg && u.stage[4] > 5.0)
        fprintf(stderr, "[hydra_mi] hm_update_run %d iterations: begin %.2f loop-end %.2f newton-started %.2f tail-queued %.2f tail-done %.2f ms\n",
                u.niter, u.stage[0], u.stage[1], u.stage[2], u.stage[3], u.stage[4]);
    return HM_OK;
}

// What the caller gets: Hzc / gains (zeros for an update without iterations), X, info[]; and on the handle the tail block
// marked valid and the error sums of the kept state when it is the last iterate.  Host only.
static void update_finish(UpdateRun &u, int info[4])
{
    hm_ctx *h = u.h;
    const size_t n4 = u.n4;
    if (u.niter > 0) {
        if (u.a.Hzc) memcpy(u.a.Hzc, h->tail.v.data(), n4 * 4 * sizeof(double));
        if (u.a.gains) memcpy(u.a.gains, h->tail.v.data() + n4 * 4, n4 * 3 * sizeof(double));
    } else {
        if (u.a.Hzc) memset(u.a.Hzc, 0, n4 * 4 * sizeof(double));
        if (u.a.gains) memset(u.a.gains, 0, n4 * 3 * sizeof(double));
        std::fill(h->tail.v.begin(), h->tail.v.end(), 0.0);
    }
    h->tail.valid = true;                          // (taken, queued for hm_update_tail, or zeros)
    memcpy(u.a.X, u.Xcur.data(), n4 * sizeof(double));
    info[0] = u.niter; info[1] = u.accepted; info[2] = u.reverted ? 1 : 0; info[3] = u.conv ? 1 : 0;
    if (u.niter > 0 && !u.reverted) {
        // the state that is kept is the last iterate: its render produced Renderer.error against the raw flow as well
        const double *res = u.res();
        h->last_err[0] = res[n4]; h->last_err[1] = res[n4 + 8]; h->last_err[2] = res[n4 + 9]; h->last_err[3] = res[n4 + 3];
        h->last_err_X = u.Xcur;
        h->last_err_valid = true;
    }
}

// IteratedKalmanFilter.update (kalman.py:774-831) in one call: hm_update_begin, up to max_iter
// hm_update_step's with the reference's acceptance logic between them, hm_update_cov of the state
// that is kept.  Per iteration the host sees one small result block (step, the four error sums)
// that the last kernel writes into pinned memory; the iterate itself never leaves the device, and
// the render that gave an iterate's error is the reference render of the next measurement.
extern "C" int hm_update_run(hm_ctx_t h, const double *W_prior, double *X, double deltaX, int masked, int max_iter,
                             double reltol, int info[4], double *errs, double *Hzc, double *gains, double *W_out)
{
    HM_ARG(h && X && info, "hm_update_run: NULL argument");
    UpdateRun u(h, {W_prior, X, deltaX, masked, max_iter, reltol, errs, Hzc, gains, W_out});      // (takes h->armed: first)
    HM_TRY(update_enter(u));
    for (int it = 0; it < max_iter;) {
        SpecSwap swap(h);                          // (put back on every way out of this block but keep())
        HM_TRY(update_queue_iteration(u, it, swap));
        HM_TRY(update_meanwhile(u, it));
        Taken taken = Taken::go_on;
        HM_TRY(update_take_result(u, it, swap, &taken));
        if (taken == Taken::retry) continue;
        Verdict verdict = Verdict::go_on;
        HM_TRY(update_judge(u, it, &verdict));
        if (verdict != Verdict::go_on) break;
        swap.keep();
        it++;
    }
    HM_TRY(update_state_final(u));
    HM_TRY(update_tail(u));
    update_finish(u, info);
    return HM_OK;
}

// Renderer.error (renderer.py:485-501) of the state the last hm_update_run kept, against the observation as given
// (the raw flow), when that state is its last iterate: the sums came out of that iterate's render (k_render_iter).
// Returns HM_OK and fills err, or 1 when they are not at hand (another state, a reverted update, a new observation):
// the caller then asks hm_error.
extern "C" int hm_update_last_error(hm_ctx_t h, const double *X, double err[4])
{
    HM_ARG(h && X && err, "hm_update_last_error: NULL argument");
    if (!h->last_err_valid || h->last_err_X.size() != (size_t)4 * h->N) return 1;
    if (memcmp(X, h->last_err_X.data(), (size_t)4 * h->N * sizeof(double)) != 0) return 1;
    for (int k = 0; k < 4; k++) err[k] = h->last_err[k];
    return HM_OK;
}
