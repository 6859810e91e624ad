// The mask of the observation on MI355X: the reference's contour pruning, the outline of what is left, projectmask onto it,
// and the chained state path between two frames (hm_chain_project).  Host orchestration and C-ABI (include/hydra_mi.h); the
// kernels are in project_kernels.h, which this translation unit alone compiles.  Everything here runs on the handle's second
// stream (or, chained, on the prediction's), beside the filter's own.
// Of the handle (ctx.h) it writes `mask` and stream2; of the others' state chain.pending (hm_chain_project) and, by that
// call's kernel, d_X0 and d_X.  It reads the observation's mask (o_ym, have_obs), newton4 (the prediction in flight) and
// result_delay.
#include "ctx.h"
#include "project_kernels.h"
#include <cstring>

// The second stream (projectmask, hm_ms_predict): short launches beside the first stream's, same dispatch priority.
int ensure_stream2(hm_ctx *h)
{
    HM_HIP(h->own.stream(&h->stream2));
    return HM_OK;
}

// hm_project_mask's buffers, built once
static int project_buffers(hm_ctx *h)
{
    if (h->mask.ready) return HM_OK;
    const size_t n = (size_t)h->W * h->H, n4 = (size_t)4 * h->N;
    HM_HIP(h->own.alloc(&h->mask.d_outline, n * sizeof(int2)));
    HM_HIP(h->own.alloc(&h->mask.d_outline_cnt, 4 * sizeof(int)));
    HM_HIP(h->own.alloc(&h->mask.d_flag, n));
    HM_HIP(h->own.alloc(&h->mask.d_pruned, n));
    HM_HIP(h->own.alloc(&h->mask.ccl.L, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->mask.ccl.cnt, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->mask.ccl.bnd, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->mask.ccl.edge, n));
    HM_HIP(h->own.alloc(&h->mask.ccl.best, sizeof(unsigned long long)));
    h->mask.ccl.W = h->W; h->mask.ccl.H = h->H;
    HM_HIP(h->own.alloc(&h->mask.d_X, n4 * sizeof(double)));
    HM_HIP(h->own.alloc(&h->mask.d_done, sizeof(int)));
    // zeroed on the stream the kernel that counts in it runs on: a hipMemset on the null stream is not ordered with a
    // non-blocking stream and may land in the middle of that kernel -- no workgroup is the last one then, the count of
    // moved vertices never comes and the projection of a context's first frame was silently dropped (seen once in ~10 runs)
    HM_HIP(hipMemsetAsync(h->mask.d_done, 0, sizeof(int), h->stream2));
    HM_HIP(h->own.host_alloc(&h->mask.pin, (n4 + 2 * (n4 + 1)) * sizeof(double), hipHostMallocCoherent));
    memset(h->mask.pin, 0, (n4 + 2 * (n4 + 1)) * sizeof(double));
    h->mask.v.assign(n4 + 1, 0.0);
    HM_HIP(h->own.event(&h->mask.ev_pm));
    HM_HIP(h->own.event(&h->mask.ev_outline));
    h->mask.ready = true;
    return HM_OK;
}
static Outline outline_of(const hm_ctx *h) { return Outline{h->mask.d_outline, h->mask.d_outline_cnt, h->W * h->H, h->mask.d_flag}; }
// the projection's arguments; X: the state in device memory it moves in place (k_project_mask), NULL for k_project_mask_host
static ProjArgs proj_args(const hm_ctx *h, double *X) { return ProjArgs{h->mask.d_pruned, h->W, h->H, h->N, outline_of(h), X}; }

// the reference's contour pruning of the mask in device memory (imgproc.py:198-228: the largest object, its holes of area
// >= 40) into mask.d_pruned, then the border pixels of what is left; queued on the second stream
int queue_outline(hm_ctx *h, const uint8_t *mask)
{
    HM_HIP(hipMemsetAsync(h->mask.d_outline_cnt, 0, 4 * sizeof(int), h->stream2));
    const dim3 cg(hm_cdiv(h->W, 64), hm_cdiv(h->H, CCL_NT / 64)), cb(CCL_NT);
    hipLaunchKernelGGL(k_ccl_local, dim3(hm_cdiv(h->W, CCL_TW), hm_cdiv(h->H, CCL_TH)), cb, 0, h->stream2, mask, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_border, cg, cb, 0, h->stream2, mask, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_roots, cg, cb, 0, h->stream2, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_flatten, cg, cb, 0, h->stream2, mask, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_stats, cg, cb, 0, h->stream2, mask, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_select, cg, cb, 0, h->stream2, mask, h->mask.ccl);
    hipLaunchKernelGGL(k_ccl_write, cg, cb, 0, h->stream2, mask, h->mask.ccl, h->mask.d_pruned);
    hipLaunchKernelGGL(k_outline, dim3(hm_cdiv(h->W, 64), hm_cdiv(h->H, OUTLINE_NT / 64)), dim3(OUTLINE_NT), 0, h->stream2,
                       (const uint8_t *)h->mask.d_pruned, h->W, h->H, outline_of(h));
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->mask.ev_outline, h->stream2));
    h->mask.prepared = nullptr;
    return HM_OK;
}
// the caller's host mask y_m (W*H) into mask.d_mask and its outline queued: the buffers no longer hold the observation's
static int outline_of_host_mask(hm_ctx *h, const uint8_t *y_m)
{
    const size_t n = (size_t)h->W * h->H;
    h->mask.outline_ready = false;
    HM_HIP(h->own.alloc(&h->mask.d_mask, n));
    HM_HIP(hipMemcpyAsync(h->mask.d_mask, y_m, n, hipMemcpyHostToDevice, h->stream2));
    return queue_outline(h, h->mask.d_mask);
}

// KalmanFilter.projectmask (kalman.py:724-742): vertices more than 1 px outside the object are
// walked back onto its outline, their displacement is added to their velocity.  y_m: a W*H host
// mask (object where > 0), or NULL for the mask of the observation in place.  X (4N) is updated in
// place; *moved (may be NULL) receives the number of vertices that were outside.
extern "C" int hm_project_mask(hm_ctx_t h, const uint8_t *y_m, double *X, int *moved)
{
    HM_ARG(h && X, "hm_project_mask: NULL argument");
    HM_JOIN_LAZY(h);
    if (!y_m) { NEED_OBS(h, "hm_project_mask"); }
    HM_HIP(hipSetDevice(h->device));
    // On the handle's second stream, with buffers of its own, and without joining the helper thread: the projection
    // needs the mask and the predicted state only, and in a frame of the filter it comes while the covariance half of
    // the update (hm_update_prefactor: ~0.25 ms of launches) is still being queued and run on the first stream --
    // behind those it would have its caller wait for them.
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    hipStream_t s = h->stream2;
    const size_t n4 = (size_t)4 * h->N, xb = n4 * sizeof(double);
    if (!y_m) {
        // The mask of the resident observation: its outline was queued when the observation was set (or is now, the
        // first time); the state goes through page-locked memory both ways, the result as a block the host takes when
        // it is whole (host_block.h) -- one launch and no copy operations on the way (0.15 -> ~0.03 ms per frame of the streaming pipeline).
        if (!h->mask.outline_ready) {
            HM_TRY(queue_outline(h, h->o_ym));
            h->mask.outline_ready = true;
        }
        memcpy(h->mask.pin, X, xb);
        hipLaunchKernelGGL(k_project_mask_host, dim3(h->N), dim3(PROJ_NT), 0, s, proj_args(h, nullptr), (const double *)h->mask.pin,
                           h->mask.pin + n4, (double *)nullptr, (double *)nullptr, h->mask.d_done, (double)(++h->mask.ticket), h->result_delay);
        HM_HIP(hipGetLastError());
        HM_TRY(hb_wait(s, h->mask.pin + n4, 0, n4 + 1, hb_stamp(h->mask.ticket), h->mask.v.data(), "hm_project_mask"));
        const int nmoved = (int)h->mask.v[n4];
        if (nmoved) memcpy(X, h->mask.v.data(), xb);
        if (moved) *moved = nmoved;
        return HM_OK;
    }
    HM_TRY(outline_of_host_mask(h, y_m));
    HM_HIP(hipMemcpyAsync(h->mask.d_X, X, xb, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_project_mask, dim3(h->N), dim3(PROJ_NT), 0, s, proj_args(h, h->mask.d_X));
    HM_HIP(hipGetLastError());
    int cnt[4] = {0, 0, 0, 0};
    HM_HIP(hipMemcpyAsync(cnt, h->mask.d_outline_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HM_HIP(hipMemcpyAsync(X, h->mask.d_X, xb, hipMemcpyDeviceToHost, s));
    HM_HIP(stream_wait(s));
    if (moved) *moved = cnt[2];
    return HM_OK;
}

// The reference's contour pruning of a mask (imgproc.py:198-228: the largest object and its holes of area >= 40) as
// hm_project_mask applies it -- fine-grained operator for the parity tests.  y_m: W*H host mask (object where > 0);
// out: W*H, 1 where the pruned object is.
extern "C" int hm_prune_mask(hm_ctx_t h, const uint8_t *y_m, uint8_t *out)
{
    HM_ARG(h && y_m && out, "hm_prune_mask: NULL argument");
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    HM_TRY(outline_of_host_mask(h, y_m));
    HM_HIP(hipMemcpyAsync(out, h->mask.d_pruned, (size_t)h->W * h->H, hipMemcpyDeviceToHost, h->stream2));
    HM_HIP(hipStreamSynchronize(h->stream2));
    return HM_OK;
}

// ---- the state path between two frames without host round trips ------------------------------------------------------
// compute() (kalman.py:676-700) is predict -> projectmask -> update.  With the state prediction started on the device
// by the update that precedes it (hm_newton_dev_start) every step's input is in device memory before the host needs
// to know it: hm_chain_project queues projectmask (kalman.py:724-742, mask of the observation in place) of the
// prediction in flight behind its kernel -- k_project_mask_host reads the kernel's device copy of the predicted state
// and leaves the projected state in d_X0, where the update keeps its prior mean -- and marks the handle: the next
// hm_update_run starts from d_X0 as it is (its X argument is output only), waits on the device for the projection
// instead of uploading a state, and collects the two kernels' result blocks (predicted state, Newton iterations,
// projected state, vertices moved: hm_chain_states) while its first iteration runs.  The numbers are those of the
// three separate calls.  Returns 1 when there is nothing to chain (no prediction in flight): the caller takes the
// three calls.
extern "C" int hm_chain_project(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_chain_project: NULL handle");
    HM_JOIN_LAZY(h);
    NEED_OBS(h, "hm_chain_project");
    if (!h->newton4.pending || !h->newton4.d_X) return 1;
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    if (!h->mask.outline_ready) {
        HM_TRY(queue_outline(h, h->o_ym));
        h->mask.outline_ready = true;
    }
    const size_t n4 = (size_t)4 * h->N;
    // on the prediction's own stream, right behind its kernel (no hop between streams there); the outline of the mask was
    // queued on the second stream when the observation was set, or a frame ahead (hm_prepare_mask)
    HM_HIP(hipStreamWaitEvent(h->newton4.stream, h->mask.ev_outline, 0));
    hipLaunchKernelGGL(k_project_mask_host, dim3(h->N), dim3(PROJ_NT), 0, h->newton4.stream, proj_args(h, nullptr), (const double *)h->newton4.d_X, h->mask.pin + n4, h->d_X0,
                       h->d_X, h->mask.d_done, (double)(++h->mask.ticket), h->result_delay);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->mask.ev_pm, h->newton4.stream));
    h->chain.pending = true;
    return HM_OK;
}

// hm_prepare_mask behind its argument checks; hm_update_run queues an armed mask through it (hm_update_arm_mask)
int prepare_mask(hm_ctx *h, const uint8_t *d_y_m)
{
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    // the projection of the CURRENT frame may still be reading the outline buffers on the prediction's stream
    if (h->mask.ev_pm && h->mask.ticket > 0) HM_HIP(hipStreamWaitEvent(h->stream2, h->mask.ev_pm, 0));
    HM_TRY(queue_outline(h, d_y_m));
    h->mask.outline_ready = false;                    // (the buffers no longer hold the outline of the observation in place)
    h->mask.prepared = d_y_m;
    return HM_OK;
}

// The pruning + outline of a mask in device memory queued AHEAD of the hm_set_observation_dev that will name it (a
// streaming caller has the next frame's mask in device memory a frame early): ~0.2 ms of kernels on the second stream
// that would otherwise start when the next frame does and keep its projection waiting.  Queued behind whatever the
// second stream still has to do with the current outline.  The mask must not change until that hm_set_observation_dev;
// any other observation, or a projection onto a host mask, simply discards the preparation.  Only the address is
// compared: d_y_m = NULL discards the preparation, if any, for a caller about to put another mask at that address (a
// frame ring slot reused, a new phase).
extern "C" int hm_prepare_mask(hm_ctx_t h, const uint8_t *d_y_m)
{
    HM_ARG(h != nullptr, "hm_prepare_mask: NULL handle");
    HM_JOIN_LAZY(h);                             // (an update's tail on the helper thread may be preparing an armed mask)
    if (!d_y_m) {
        h->mask.prepared = nullptr;
        return HM_OK;
    }
    return prepare_mask(h, d_y_m);
}

// What the last chained hm_update_run started from: the predicted state, the projected state (its prior mean), the
// Newton iterations of the prediction, the vertices projectmask moved.  Any pointer may be NULL.
extern "C" int hm_chain_states(hm_ctx_t h, double *predicted, double *projected, int *newton_iterations, int *moved)
{
    HM_ARG(h != nullptr, "hm_chain_states: NULL handle");
    const size_t n4 = (size_t)4 * h->N;
    if (h->chain.pred.size() != n4 || h->chain.proj.size() != n4) { hm_set_error("hm_chain_states: no chained update has run"); return HM_ERR_STATE; }
    if (predicted) memcpy(predicted, h->chain.pred.data(), n4 * sizeof(double));
    if (projected) memcpy(projected, h->chain.proj.data(), n4 * sizeof(double));
    if (newton_iterations) *newton_iterations = h->chain.its;
    if (moved) *moved = h->chain.moved;
    return HM_OK;
}
