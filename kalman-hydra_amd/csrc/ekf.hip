// EKF measurement model on MI355X: host orchestration and C-ABI (include/hydra_mi.h).
// Replaces reference renderer.py (OpenGL rasteriser), cuda.py and cuda_multi.py
// (reduction kernels + PBO plumbing).  In this order: handle lifetime and tuning, render and measure, the dense update,
// hm_update_run, covariance prediction, the Newton launches and the chained state path, mask projection.  The smoother
// is in smooth.hip; it queues the two launch sequences it shares with the filter through ekf_queue_fpft and
// ekf_queue_chol_flow, defined here (ctx.h).
#include "ctx.h"
#include "ekf_kernels.h"
#include "dense_kernels.h"
#include "chol_flow_kernels.h"
#include "project_kernels.h"
#include "predict_kernels.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <set>
#include <thread>
#include <utility>
#include <vector>

// (struct hm_ctx, ctx_join / HM_JOIN, stream_wait, upload: ctx.h)

// Take values [first, first + n) of a result block in page-locked host memory (host_block.h) into `out` once every one of
// their pairs carries the launch's stamp.  The last pair is looked at first (one pair of loads per poll while nothing is
// there yet); a block of which some words are still missing is simply looked at again -- no order of arrival is assumed.
// A couple of microseconds against ~20 for waking up from a stream synchronisation, which remains as the fallback: after
// 20 ms the stream is waited for (everything queued behind the block's kernel included) and a block that is not whole
// then is an error.
static int hb_wait(hipStream_t st, const double *blk, size_t first, size_t n, unsigned long long stamp, double *out, const char *who)
{
    const volatile unsigned long long *canary = (const volatile unsigned long long *)blk + 2 * (first + n - 1);
    const auto t_start = std::chrono::steady_clock::now();
    const auto t_yield = t_start + std::chrono::microseconds(700), t_give_up = t_start + std::chrono::milliseconds(20);
    bool polite = false;
    for (int spin = 0;; spin++) {
        if ((canary[0] ^ canary[1]) == stamp && hb_take(blk, first, n, stamp, out)) return HM_OK;
        if (polite) std::this_thread::yield();
        else __builtin_ia32_pause();
        if ((spin & 255) == 255) {
            const auto now = std::chrono::steady_clock::now();
            if (now > t_give_up) break;
            polite = now > t_yield;
        }
    }
    HM_HIP(hipStreamSynchronize(st));
    if (hb_take(blk, first, n, stamp, out)) return HM_OK;
    hm_set_error("%s: a result block of the device is not whole although its stream has completed (stamp %016llx)", who, stamp);
    return HM_ERR_HIP;
}

// ---- the pool of parked difference images (DPool, ekf_kernels.h) -------------------------------------------------
static hipError_t pool_alloc(hm_ctx *h, long long cap)
{
    const size_t pc = (size_t)cap;
    h->pool.cap = 0;
    hipError_t e = h->own.grow(&h->pool.live, (pc / 64 + 1) * sizeof(int));
    for (short2 **q : {&h->pool.xi, &h->pool.yi})
        if (e == hipSuccess) e = h->own.grow(q, pc * sizeof(short2));
    for (float **q : {&h->pool.xfx, &h->pool.xfy, &h->pool.yfx, &h->pool.yfy, &h->pool.vxfx, &h->pool.vyfy})
        if (e == hipSuccess) e = h->own.grow(q, pc * sizeof(float));
    if (e == hipSuccess) h->pool.cap = cap;
    return e;
}
// A measurement reported that its star regions do not fit (the reference has no such limit: its renders are whole
// frames): make room for them -- the region areas are on the device -- plus a quarter.  The stream must be idle.
static int pool_grow(hm_ctx *h, const char *who)
{
    std::vector<int> area(h->N);
    HM_HIP(hipMemcpyAsync(area.data(), h->d_area, (size_t)h->N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    long long total = 0;
    for (int a : area) total += a;
    if (total <= h->pool.cap) { hm_set_error("%s: the difference-image pool reported an overflow it does not have", who); return HM_ERR_STATE; }
    const long long want = total + total / 4;
    if (want > ((long long)1 << 32)) {              // 128 GB of planes: not a mesh this path is meant for
        hm_set_error("%s: the star regions need %lld pixels of difference images, more than the pool may hold", who, total);
        return HM_ERR_STATE;
    }
    if (getenv("HYDRA_MI_TRACE")) fprintf(stderr, "[hydra_mi] %s: difference-image pool %lld -> %lld pixels\n", who, h->pool.cap, want);
    const hipError_t e = pool_alloc(h, want);
    if (e != hipSuccess) {
        hm_set_error("%s: cannot grow the difference-image pool to %lld pixels: %s", who, want, hipGetErrorString(e));
        return HM_ERR_HIP;
    }
    return HM_OK;
}

static int ctx_free(hm_ctx *h)
{
    if (!h) return HM_OK;
    (void)ctx_join(h);
    if (h->helper_used) h->helper.stop();
    (void)hipSetDevice(h->device);
    // every stream of the handle drained before anything is freed: a state prediction started ahead is always pending after
    // the last frame (it writes into pin_n4), and so may be launches of an update that ended in an error
    h->own.drain();
    h->own.release();
    delete h;
    return HM_OK;
}


extern "C" int hm_ctx_create(int device, int W, int H, int N, int T, const int32_t *tri, const float *uv, double eps_Z,
                             double eps_J, double eps_M, hm_ctx_t *out)
{
    HM_ARG(out != nullptr, "hm_ctx_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 4096 && H <= 4096, "hm_ctx_create: frame size %dx%d outside 1..4096", W, H);
    HM_ARG(N >= 3 && T >= 1 && T <= EKF_MAX_TRI, "hm_ctx_create: need N >= 3 vertices and 1..%d triangles (N=%d, T=%d)",
           EKF_MAX_TRI, N, T);
    HM_ARG(tri && uv, "hm_ctx_create: NULL mesh arrays");
    HM_ARG(eps_Z > 0 && eps_J > 0 && eps_M > 0, "hm_ctx_create: eps_Z, eps_J, eps_M must be positive");
    std::vector<std::vector<int>> star(N);
    std::set<std::pair<int, int>> eset;
    for (int t = 0; t < T; t++) {
        int v[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        for (int k = 0; k < 3; k++) {
            HM_ARG(v[k] >= 0 && v[k] < N, "hm_ctx_create: triangle %d refers to vertex %d (N=%d)", t, v[k], N);
            star[v[k]].push_back(t);
            int a = v[k], b = v[(k + 1) % 3];
            if (a != b) eset.insert(std::make_pair(std::min(a, b), std::max(a, b)));
        }
    }
    std::vector<int> off(N + 1, 0), flat;
    for (int v = 0; v < N; v++) {
        // a vertex listed twice in one (degenerate) triangle would be listed twice here
        std::sort(star[v].begin(), star[v].end());
        star[v].erase(std::unique(star[v].begin(), star[v].end()), star[v].end());
        HM_ARG((int)star[v].size() <= EKF_MAX_STAR, "hm_ctx_create: vertex %d has %d triangles, limit %d", v,
               (int)star[v].size(), EKF_MAX_STAR);
        off[v + 1] = off[v] + (int)star[v].size();
        flat.insert(flat.end(), star[v].begin(), star[v].end());
    }
    HM_HIP(hipSetDevice(device));
    hm_ctx *h = new hm_ctx();
    h->device = device; h->W = W; h->H = H; h->N = N; h->T = T;
    h->eps_Z = eps_Z; h->eps_J = eps_J; h->eps_M = eps_M;
    h->tri.assign(tri, tri + (size_t)3 * T);
    for (const auto &e : eset) { h->edges.push_back(e.first); h->edges.push_back(e.second); }
    h->E = (int)eset.size();
    h->njobs = N + h->E;
    // two workgroups per edge job as long as they are ONE round of the chip (122 VGPRs: four workgroups per CU, 1 024 slots),
    // else one: at 201 vertices 556 edges x 2 = 1 112 workgroups had 88 of them wait for a slot and the launch take a second
    // round (308.6 -> 305.1 us per iteration with one; the sums of an edge are then added in another order: rounding-level
    // differences); small meshes keep the parallelism of two
    h->esplit = 2 * h->E > 1024 ? 1 : 2;
    const size_t n = (size_t)W * H;
    int rc = HM_OK;
    auto step = [&](int r) { if (rc == HM_OK) rc = r; };
    step(upload(h->own, &h->d_tri, tri, (size_t)3 * T));
    step(upload(h->own, &h->d_uv, uv, (size_t)2 * N));
    step(upload(h->own, &h->d_star_off, off.data(), off.size()));
    step(upload(h->own, &h->d_star_tri, flat.data(), flat.size()));
    step(upload(h->own, &h->d_edges, h->edges.data(), h->edges.size()));
    {   // neighbours of every vertex with the edge job that holds their block of HTH
        std::vector<std::vector<std::pair<int, int>>> nb(N);
        for (int e = 0; e < h->E; e++) {
            const int a = h->edges[2 * e], b = h->edges[2 * e + 1];
            nb[a].push_back(std::make_pair(b, e));
            nb[b].push_back(std::make_pair(a, e));
        }
        std::vector<int> noff(N + 1, 0), nu, ne;
        for (int v = 0; v < N; v++) {
            std::sort(nb[v].begin(), nb[v].end());
            noff[v + 1] = noff[v] + (int)nb[v].size();
            for (const auto &q : nb[v]) { nu.push_back(q.first); ne.push_back(q.second); }
            if (rc == HM_OK && 4 * ((int)nb[v].size() + 1) > PREP_MAX_ENTRIES) {
                hm_set_error("hm_ctx_create: vertex %d has %d neighbours, limit %d", v, (int)nb[v].size(), PREP_MAX_ENTRIES / 4 - 1);
                rc = HM_ERR_ARG;
            }
        }
        step(upload(h->own, &h->d_nb_off, noff.data(), noff.size()));
        step(upload(h->own, &h->d_nb_u, nu.data(), nu.size()));
        step(upload(h->own, &h->d_nb_e, ne.data(), ne.size()));
    }
    // the device set-up: it ends at the first failure, and ctx_free releases whatever it made
    hipError_t e = hipSuccess;
    auto dev = [&](auto **p, size_t bytes) { if (e == hipSuccess) e = h->own.alloc(p, bytes); };
    if (rc == HM_OK) {
        // the filter's launches are a dependent chain of short kernels beside the flow's long ones on another stream:
        // its queue gets the highest dispatch priority the device offers (HYDRA_MI_EKF_PRIORITY=0 turns that off)
        const char *pe = getenv("HYDRA_MI_EKF_PRIORITY");
        e = h->own.stream(&h->stream, !(pe && atoi(pe) == 0));
        dev(&h->d_tex, n);
        dev(&h->d_yim, n);
        dev(&h->d_ym, n);
        dev(&h->d_yfx, n * sizeof(float));
        dev(&h->d_yfy, n * sizeof(float));
        dev(&h->d_yfxm, n * sizeof(float));
        dev(&h->d_yfym, n * sizeof(float));
        dev(&h->d_setup, (size_t)T * sizeof(TriSetup));
        dev(&h->d_cfgs, (size_t)N * MEAS_NCFG * (EKF_MAX_STAR + 1) * sizeof(TriSetup));
        dev(&h->d_ubox, (size_t)N * UBOX_STRIDE * sizeof(int4));
        dev(&h->d_tmask, (size_t)N * TMASK_STRIDE * sizeof(unsigned));
        dev(&h->d_tlist, (size_t)N * TMASK_STRIDE * sizeof(int));
        dev(&h->d_tcount, (size_t)N * sizeof(int));
        dev(&h->d_X, (size_t)4 * N * sizeof(double));
        dev(&h->d_out, (size_t)h->njobs * MEAS_VSPLIT_MAX * MEAS_OUT * sizeof(double));
        dev(&h->d_partial, (size_t)h->red_blocks * 4 * sizeof(double));
        h->ntiles = hm_cdiv(W, RI_W) * hm_cdiv(H, 8);           // most strips of k_render_iter (render_rows 8)
        dev(&h->d_tpart, (size_t)h->ntiles * RI_NV * sizeof(double));
        dev(&h->d_im8, n);
        dev(&h->d_m8, n);
        const size_t n4 = (size_t)4 * N, nn = n4 * n4 * sizeof(double);
        dev(&h->d_H, nn);
        dev(&h->d_HTH, nn);
        if (e == hipSuccess) e = hipMemsetAsync(h->d_HTH, 0, nn, h->stream);
        dev(&h->d_invW0, nn);
        const size_t nn_aug = (size_t)(hm_cdiv((int)n4, DNB) * DNB + DNB) * n4 * sizeof(double);
        dev(&h->d_Af[0], nn_aug);
        dev(&h->d_Af[1], nn_aug);
        dev(&h->d_Awork, nn_aug);
        const size_t ld_bytes = (size_t)hm_cdiv((int)n4, DNB) * DNB * DNB * sizeof(double);
        dev(&h->d_T[0], nn);       // L^-1 of the factor in the same slot
        dev(&h->d_T[1], nn);
        dev(&h->d_step, n4 * sizeof(double));
        dev(&h->d_Lt[0], ld_bytes);  // inverses of the factored diagonal blocks
        dev(&h->d_Lt[1], ld_bytes);
        dev(&h->d_Wtmp, nn);
        dev(&h->d_flowP, 3 * ld_bytes);      // P, Q and Y blocks of k_chol_flow
        dev(&h->d_flowctl, 4 * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(h->d_flowctl, 0, 4 * sizeof(unsigned), h->stream);
        dev(&h->d_Hz, n4 * sizeof(double));
        dev(&h->d_Hzc, n4 * 4 * sizeof(double));
        dev(&h->d_Wprior, nn);
        dev(&h->d_gain, n4 * 3 * sizeof(double));
        h->pin_n = 2 * (n4 + RES_HEAD + n4 * 4 + n4 * 3) + 2;
        if (e == hipSuccess) e = h->own.host_alloc(&h->pin, h->pin_n * sizeof(double), hipHostMallocCoherent);
        if (e == hipSuccess) memset(h->pin, 0, h->pin_n * sizeof(double));
        h->pin_scratch = (int *)(h->pin + h->pin_n - 2);
        h->resv.assign(n4 + RES_HEAD, 0.0);
        h->tailv.assign(n4 * 7, 0.0);
        dev(&h->d_X0, n4 * sizeof(double));
        dev(&h->pool.hdr, (size_t)4 * N * sizeof(int));
        dev(&h->pool.overflow, sizeof(int));
        dev(&h->d_area, (size_t)N * sizeof(int));
        h->pool.area = h->d_area;
        // pool of parked difference images (32 B per pixel): the star regions overlap about six times, so a mesh that
        // covers the whole frame needs about six frames' worth of pixels plus the padding of every region to whole 8x8
        // tiles (the bench's disk, a third of the frame: 1.6); it starts at 8 frames' worth = 268 MB at 1024^2 and grows
        // when a measurement reports that its regions do not fit (pool_grow)
        if (e == hipSuccess) e = pool_alloc(h, (long long)8 * W * H);
        dev(&h->d_Xn, n4 * sizeof(double));
        for (Targets *t : {&h->ref, &h->P, &h->Q})
            if (e == hipSuccess) e = alloc_targets(h->own, *t, n);
    }
    if (e != hipSuccess) {
        hm_set_error("hm_ctx_create: device allocation failed: %s", hipGetErrorString(e));
        step(HM_ERR_HIP);
    }
    if (rc != HM_OK) {
        ctx_free(h);
        return rc;
    }
    h->h_partial.resize((size_t)h->red_blocks * 4);
    h->h_tpart.resize((size_t)h->ntiles * RI_NV);
    *out = h;
    return HM_OK;
}

extern "C" int hm_ctx_destroy(hm_ctx_t h) { return ctx_free(h); }

// the launches of the filter's kernels that readout.hip queues (ctx.h)
void ekf_queue_setup_all(hipStream_t st, const Mesh &m, const double *d_X, TriSetup *d_setup)
{
    hipLaunchKernelGGL(k_setup_all, dim3(hm_cdiv(m.T, 64)), dim3(64), 0, st, m, d_X, d_setup);
}
void ekf_queue_render(hipStream_t st, const Mesh &m, const double *d_X, const TriSetup *d_setup, const Targets &out,
                      const int *d_labels, int *d_ids)
{
    const dim3 grid(hm_cdiv(m.W, EKF_TILE), hm_cdiv(m.H, EKF_TILE)), block(EKF_TILE, EKF_TILE);
    if (d_ids) hipLaunchKernelGGL((k_render<1>), grid, block, 0, st, m, d_X, d_setup, out, d_labels, d_ids);
    else hipLaunchKernelGGL((k_render<0>), grid, block, 0, st, m, d_X, d_setup, out, (const int *)nullptr, (int *)nullptr);
}

#ifdef HM_STAMP
// development builds only: where k_render_iter writes its per-workgroup time stamps (device pointer, 8 words per workgroup)
extern "C" int hm_debug_stamps(void *dev_ptr)
{
    long long *p = (long long *)dev_ptr;
    HM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), &p, sizeof p));
    return HM_OK;
}
#endif

// The keys of hm_ctx_tune: a value is admitted when it is lo, lo + step, ... up to hi; `must` is the clause of the message
// after "hm_ctx_tune: <key> " (NULL: "must be in lo..hi").
#define TUNE_SET(field) [](hm_ctx *h, long long v) { h->field = (decltype(h->field))v; }
static const struct TuneKey {
    const char *key;
    long long lo, hi;
    int step;
    void (*set)(hm_ctx *, long long);
    const char *must;
} tune_keys[] = {
    {"measure_split", 1, MEAS_VSPLIT_MAX, 1, TUNE_SET(vsplit), nullptr},
    {"edge_split", 1, MEAS_VSPLIT_MAX, 1, TUNE_SET(esplit), nullptr},
    {"chol_flow", 0, 1, 1, TUNE_SET(chol_flow), "must be 0 (one launch per block step) or 1 (one persistent launch)"},
    // at least two: the first workgroup becomes the chain of the diagonal blocks and waits for blocks that only the task
    // workgroups produce
    {"chol_flow_wgs", 2, 2048, 1, TUNE_SET(flow_wgs), "must be in 2..2048 (the chain workgroup and at least one task workgroup)"},
    {"render_rows", 8, 16, 8, TUNE_SET(render_rows), "must be 8 or 16"},
    {"chol_flow_stall", 0, 100000, 1, TUNE_SET(flow_stall), nullptr},          // tests only: results must not depend on it
    {"result_delay", 0, 5000, 1, TUNE_SET(result_delay), "must be in 0..5000 (microseconds)"},   // tests only: likewise (host_block.h)
    {"tail_async", 0, 1, 1, TUNE_SET(tail_async), "must be 0 or 1"},          // same results either way
    {"tail_split", 0, 1, 1, TUNE_SET(tail_split), "must be 0 or 1"},          // same results either way
    {"newton_fail", 0, 1, 1, TUNE_SET(newton_fail), "must be 0 or 1"},        // tests only: the device predictions report a failed inner solve
    {"speculate", 0, 1, 1, TUNE_SET(speculate), "must be 0 or 1"},            // same results either way
    {"body_stats_cap", 1, BODY_STATS_CAP, 1, TUNE_SET(body.stats_cap), nullptr},   // tests only: frames one hm_body_stats accumulation takes
    {"body_rec_chunk", 0, INT32_MAX, 1, TUNE_SET(rec.chunk), "must be >= 0 (0: the default size)"},   // tests only: frames per chunk of the next hm_body_rec_begin
    {"rec_tp_frames", 1, REC_TP_MAX, 1, TUNE_SET(rec.tp_frames), nullptr},     // frames per workgroup of hm_body_rec_trace_products
    // frames per run of the running baseline, the residual planes, the trace maps, the surrogate reduction (same results for every value)
    {"rec_bl_frames", 1, REC_BL_MAX, 1, TUNE_SET(rec.bl_frames), nullptr},
    {"rec_res_frames", 1, REC_RES_MAX, 1, TUNE_SET(rec.res_frames), nullptr},
    {"rec_map_frames", 1, REC_MAP_MAX, 1, TUNE_SET(rec.map_frames), nullptr},
    {"rec_null_frames", 1, REC_NULL_MAX, 1, TUNE_SET(rec.null_frames), nullptr},
    {"rec_tm_frames", 1, REC_TM_MAX, 1, TUNE_SET(rec.tm_frames), nullptr},      // likewise: the maps against the pixel's own triangle
    // bytes per run of k_rec_gram (same results for every value)
    {"rec_gram_bytes", 64, REC_GRAM_BYTES_MAX, 64, TUNE_SET(rec.gram_bytes), "must be a multiple of 64 in 64..131008"},
    {"rec_scratch_bytes", 1, 1 << 30, 1, TUNE_SET(rec.scr_bytes), nullptr},    // tests only: the most scratch of a hm_body_rec_* call (same results for every value)
    // the most bytes of the pool stack of a pass of hm_body_rec_event_* (same results for every value); past 2^31: hm_ctx_tune64
    {"rec_ev_bytes", 1, 1ll << 34, 1, TUNE_SET(rec.ev_bytes), nullptr},
};
#undef TUNE_SET
static const TuneKey *tune_find(const char *key)
{
    for (const TuneKey &k : tune_keys)
        if (!strcmp(key, k.key)) return &k;
    return nullptr;
}
// both entry points end here (the handle joined)
static int tune_set(hm_ctx *h, const char *key, long long value)
{
    const TuneKey *k = tune_find(key);
    HM_ARG(k != nullptr, "hm_ctx_tune: unknown key '%s'", key);
    if (value < k->lo || value > k->hi || (value - k->lo) % k->step) {
        if (k->must) hm_set_error("hm_ctx_tune: %s %s", key, k->must);
        else hm_set_error("hm_ctx_tune: %s must be in %lld..%lld", key, k->lo, k->hi);
        return HM_ERR_ARG;
    }
    k->set(h, value);
    return HM_OK;
}

extern "C" int hm_ctx_tune(hm_ctx_t h, const char *key, int value)
{
    HM_ARG(h != nullptr && key != nullptr, "hm_ctx_tune: NULL argument");
    HM_JOIN(h);
    return tune_set(h, key, value);
}
// the keys whose values pass 2^31 ("rec_ev_bytes"); every other key as hm_ctx_tune takes it
extern "C" int hm_ctx_tune64(hm_ctx_t h, const char *key, int64_t value)
{
    HM_ARG(h != nullptr && key != nullptr, "hm_ctx_tune: NULL argument");
    const TuneKey *k = tune_find(key);
    if (!k || k->hi <= INT32_MAX)
        HM_ARG(value >= INT32_MIN && value <= INT32_MAX, "hm_ctx_tune: %s = %lld does not fit 32 bits", key, (long long)value);
    HM_JOIN(h);
    return tune_set(h, key, value);
}
extern "C" void *hm_ctx_stream(hm_ctx_t h)
{
    (void)ctx_join(h);
    return h ? (void *)h->stream : nullptr;
}
extern "C" int hm_ctx_sync(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_ctx_sync: NULL handle");
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_set_texture(hm_ctx_t h, const uint8_t *tex)
{
    HM_ARG(h && tex, "hm_set_texture: NULL argument");
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipMemcpyAsync(h->d_tex, tex, (size_t)h->W * h->H, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    h->last_err_valid = false;
    h->have_tex = true;
    return HM_OK;
}

// The second stream (projectmask, hm_ms_predict): short launches beside the first stream's, same dispatch priority.
static int ensure_stream2(hm_ctx *h)
{
    HM_HIP(h->own.stream(&h->stream2));
    return HM_OK;
}

// hm_project_mask's buffers and the outline of a mask in device memory, queued on the second stream
static int project_buffers(hm_ctx *h)
{
    if (h->pm_ready) return HM_OK;
    const size_t n = (size_t)h->W * h->H, n4 = (size_t)4 * h->N;
    HM_HIP(h->own.alloc(&h->d_outline, n * sizeof(int2)));
    HM_HIP(h->own.alloc(&h->d_outline_cnt, 4 * sizeof(int)));
    HM_HIP(h->own.alloc(&h->d_pm_flag, n));
    HM_HIP(h->own.alloc(&h->d_pm_pruned, n));
    HM_HIP(h->own.alloc(&h->ccl.L, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->ccl.cnt, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->ccl.bnd, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->ccl.edge, n));
    HM_HIP(h->own.alloc(&h->ccl.best, sizeof(unsigned long long)));
    h->ccl.W = h->W; h->ccl.H = h->H;
    HM_HIP(h->own.alloc(&h->d_pm_X, n4 * sizeof(double)));
    HM_HIP(h->own.alloc(&h->d_pm_done, sizeof(int)));
    // zeroed on the stream the kernel that counts in it runs on: a hipMemset on the null stream is not ordered with a
    // non-blocking stream and may land in the middle of that kernel -- no workgroup is the last one then, the count of
    // moved vertices never comes and the projection of a context's first frame was silently dropped (seen once in ~10 runs)
    HM_HIP(hipMemsetAsync(h->d_pm_done, 0, sizeof(int), h->stream2));
    HM_HIP(h->own.host_alloc(&h->pin_pm, (n4 + 2 * (n4 + 1)) * sizeof(double), hipHostMallocCoherent));
    memset(h->pin_pm, 0, (n4 + 2 * (n4 + 1)) * sizeof(double));
    h->pmv.assign(n4 + 1, 0.0);
    HM_HIP(h->own.event(&h->ev_pm));
    HM_HIP(h->own.event(&h->ev_outline));
    h->pm_ready = true;
    return HM_OK;
}
// the reference's contour pruning of the mask (imgproc.py:198-228: the largest object, its holes of area >= 40) into
// d_pm_pruned, then the border pixels of what is left
static int queue_outline(hm_ctx *h, const uint8_t *mask)
{
    HM_HIP(hipMemsetAsync(h->d_outline_cnt, 0, 4 * sizeof(int), h->stream2));
    const dim3 cg(hm_cdiv(h->W, 64), hm_cdiv(h->H, CCL_NT / 64)), cb(CCL_NT);
    hipLaunchKernelGGL(k_ccl_local, dim3(hm_cdiv(h->W, CCL_TW), hm_cdiv(h->H, CCL_TH)), cb, 0, h->stream2, mask, h->ccl);
    hipLaunchKernelGGL(k_ccl_border, cg, cb, 0, h->stream2, mask, h->ccl);
    hipLaunchKernelGGL(k_ccl_roots, cg, cb, 0, h->stream2, h->ccl);
    hipLaunchKernelGGL(k_ccl_flatten, cg, cb, 0, h->stream2, mask, h->ccl);
    hipLaunchKernelGGL(k_ccl_stats, cg, cb, 0, h->stream2, mask, h->ccl);
    hipLaunchKernelGGL(k_ccl_select, cg, cb, 0, h->stream2, mask, h->ccl);
    hipLaunchKernelGGL(k_ccl_write, cg, cb, 0, h->stream2, mask, h->ccl, h->d_pm_pruned);
    Outline o = {h->d_outline, h->d_outline_cnt, h->W * h->H, h->d_pm_flag};
    hipLaunchKernelGGL(k_outline, dim3(hm_cdiv(h->W, 64), hm_cdiv(h->H, OUTLINE_NT / 64)), dim3(OUTLINE_NT), 0, h->stream2,
                       (const uint8_t *)h->d_pm_pruned, h->W, h->H, o);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->ev_outline, h->stream2));
    h->prepared_mask = nullptr;
    return HM_OK;
}

static int finish_observation(hm_ctx *h)
{
    h->last_err_valid = false;
    const int n = h->W * h->H;
    hipLaunchKernelGGL(k_mask_flow, dim3(hm_cdiv(n, 256)), dim3(256), 0, h->stream, h->o_ym, h->o_yfx, h->o_yfy,
                       h->d_yfxm, h->d_yfym, n);
    HM_HIP(hipGetLastError());
    h->have_obs = true;
    return HM_OK;
}

extern "C" int hm_set_observation(hm_ctx_t h, const uint8_t *y_im, const float *y_fx, const float *y_fy,
                                  const uint8_t *y_m)
{
    HM_ARG(h && y_im && y_fx && y_fy && y_m, "hm_set_observation: NULL argument");
    HM_JOIN(h);
    HM_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(hipMemcpyAsync(h->d_yim, y_im, n, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(h->d_ym, y_m, n, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(h->d_yfx, y_fx, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(h->d_yfy, y_fy, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    h->o_yim = h->d_yim; h->o_ym = h->d_ym; h->o_yfx = h->d_yfx; h->o_yfy = h->d_yfy;
    HM_TRY(finish_observation(h));
    HM_HIP(hipStreamSynchronize(h->stream));
    h->outline_ready = false;
    if (h->d_outline) {              // a tracker that projects onto the mask: its outline, ahead of hm_project_mask
        HM_TRY(queue_outline(h, h->o_ym));
        h->outline_ready = true;
    }
    return HM_OK;
}

extern "C" int hm_set_observation_dev(hm_ctx_t h, const uint8_t *d_y_im, const float *d_y_fx, const float *d_y_fy,
                                      const uint8_t *d_y_m)
{
    HM_ARG(h && d_y_im && d_y_fx && d_y_fy && d_y_m, "hm_set_observation_dev: NULL argument");
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    h->o_yim = d_y_im; h->o_ym = d_y_m; h->o_yfx = d_y_fx; h->o_yfy = d_y_fy;
    HM_TRY(finish_observation(h));
    h->outline_ready = false;
    if (h->d_outline && h->prepared_mask == d_y_m) {      // hm_prepare_mask queued the outline of exactly this mask ahead
        h->outline_ready = true;
    } else if (h->d_outline) {       // as in hm_set_observation: the caller's mask is complete in device memory by contract
        HM_TRY(queue_outline(h, h->o_ym));
        h->outline_ready = true;
    }
    h->prepared_mask = nullptr;
    return HM_OK;
}

// render state X (host, 4N doubles) into target t on the handle's stream
// render the device-resident state dX into target t
static int render_dev(hm_ctx *h, const double *dX, Targets t)
{
    Mesh m = {h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    hipLaunchKernelGGL(k_setup_all, dim3(hm_cdiv(h->T, 64)), dim3(64), 0, h->stream, m, dX, h->d_setup);
    hipLaunchKernelGGL((k_render<0>), dim3(hm_cdiv(h->W, EKF_TILE), hm_cdiv(h->H, EKF_TILE)), dim3(EKF_TILE, EKF_TILE), 0,
                       h->stream, m, dX, h->d_setup, t, (const int *)nullptr, (int *)nullptr);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

static int render_into(hm_ctx *h, const double *X, Targets t)
{
    HM_HIP(hipMemcpyAsync(h->d_X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return render_dev(h, h->d_X, t);
}

static void measure_args(hm_ctx *h, const double *dX, double deltaX, int masked, MeasureArgs &a);
static int render_strips(const hm_ctx *h) { return hm_cdiv(h->W, RI_W) * hm_cdiv(h->H, h->render_rows); }

// The render of the device-resident state dX into target t as ONE launch (k_render_iter): triangle setups made per
// tile, optionally the per-tile partial sums of Renderer.error against the observation (d_tpart) and, riding along
// as extra workgroups, the star regions of the measurement at dX (they read nothing but the state).
static int render_iter(hm_ctx *h, const double *dX, Targets t, bool with_err, int masked, bool regions, double deltaX)
{
    IterRenderArgs r;
    r.m = Mesh{h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    r.X = dX;
    r.out = t;
    r.o = Obs{h->o_yim, masked ? h->d_yfxm : h->o_yfx, masked ? h->d_yfym : h->o_yfy, h->o_ym};
    r.raw_fx = h->o_yfx; r.raw_fy = h->o_yfy;
    r.partial = h->d_tpart;
    r.tiles_x = hm_cdiv(h->W, RI_W); r.tiles_y = hm_cdiv(h->H, h->render_rows);
    const int nstrips = r.tiles_x * r.tiles_y;
    r.with_err = with_err ? 1 : 0;
    r.n_regions = regions ? h->N : 0;
    MeasureArgs a;
    measure_args(h, dX, deltaX, masked, a);
    if (h->render_rows == 8) hipLaunchKernelGGL((k_render_iter<8>), dim3(r.n_regions + nstrips), dim3(256), 0, h->stream, r, a, h->d_area);
    else hipLaunchKernelGGL((k_render_iter<16>), dim3(r.n_regions + nstrips), dim3(256), 0, h->stream, r, a, h->d_area);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// the RI_NV sums of Renderer.error from the per-strip partials, added in the order of d_tile_partial_sums
static void hm_tile_partial_sums(const double *p, int ntiles, double s[RI_NV])
{
    static thread_local double g[RI_GROUPS][RI_NV];
    for (int t = 0; t < RI_GROUPS; t++) {
        double a[RI_NV];
        for (int k = 0; k < RI_NV; k++) a[k] = 0.0;
        for (int i = t; i < ntiles; i += RI_GROUPS)
            for (int k = 0; k < RI_NV; k++) a[k] += p[RI_NV * (size_t)i + k];
        for (int k = 0; k < RI_NV; k++) g[t][k] = a[k];
    }
    for (int k = 0; k < RI_NV; k++) {
        double v = 0.0;
        for (int t = 0; t < RI_GROUPS; t++) v += g[t][k];
        s[k] = v;
    }
}

#define NEED_TEX(h, who) \
    if (!(h)->have_tex) { hm_set_error(who ": hm_set_texture has not been called"); return HM_ERR_STATE; }
#define NEED_OBS(h, who) \
    if (!(h)->have_obs) { hm_set_error(who ": hm_set_observation has not been called"); return HM_ERR_STATE; }
#define NEED_REF(h, who) \
    if (!(h)->have_ref) { hm_set_error(who ": hm_initjacobian has not been called"); return HM_ERR_STATE; }

extern "C" int hm_render(hm_ctx_t h, const double *X, uint8_t *im, float *fx, float *fy, uint8_t *mk)
{
    HM_ARG(h && X, "hm_render: NULL argument");
    HM_JOIN(h);
    NEED_TEX(h, "hm_render");
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(render_into(h, X, h->P));
    const int n = h->W * h->H;
    hipLaunchKernelGGL(k_resolve, dim3(hm_cdiv(n, 256)), dim3(256), 0, h->stream, h->P, h->d_im8, h->d_m8, n);
    if (im) HM_HIP(hipMemcpyAsync(im, h->d_im8, n, hipMemcpyDeviceToHost, h->stream));
    if (mk) HM_HIP(hipMemcpyAsync(mk, h->d_m8, n, hipMemcpyDeviceToHost, h->stream));
    if (fx) HM_HIP(hipMemcpyAsync(fx, h->P.fx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (fy) HM_HIP(hipMemcpyAsync(fy, h->P.fy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

static Obs obs_of(hm_ctx *h, int masked)
{
    Obs o = {h->o_yim, masked ? h->d_yfxm : h->o_yfx, masked ? h->d_yfym : h->o_yfy, h->o_ym};
    return o;
}

extern "C" int hm_initjacobian(hm_ctx_t h, const double *X, int masked)
{
    HM_ARG(h && X, "hm_initjacobian: NULL argument");
    HM_JOIN(h);
    (void)masked;
    NEED_TEX(h, "hm_initjacobian");
    NEED_OBS(h, "hm_initjacobian");
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(render_into(h, X, h->ref));
    HM_HIP(hipStreamSynchronize(h->stream));
    h->X0.assign(X, X + 4 * h->N);
    h->have_ref = true;
    return HM_OK;
}

// sum the per-workgroup partials in index order
static int collect4(hm_ctx *h, double s[4])
{
    HM_HIP(hipMemcpyAsync(h->h_partial.data(), h->d_partial, (size_t)h->red_blocks * 4 * sizeof(double),
                          hipMemcpyDeviceToHost, h->stream));
    HM_HIP(stream_wait(h->stream));
    for (int k = 0; k < 4; k++) s[k] = 0.0;
    for (int b = 0; b < h->red_blocks; b++)
        for (int k = 0; k < 4; k++) s[k] += h->h_partial[(size_t)4 * b + k];
    return HM_OK;
}

extern "C" int hm_jz(hm_ctx_t h, const double *Xp, int masked, double *jz, double jzc[4])
{
    HM_ARG(h && Xp, "hm_jz: NULL argument");
    HM_JOIN(h);
    NEED_REF(h, "hm_jz");
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(render_into(h, Xp, h->P));
    hipLaunchKernelGGL(k_jz, dim3(h->red_blocks), dim3(RED_NT), 0, h->stream, h->ref, h->P, obs_of(h, masked),
                       h->W * h->H, h->d_partial);
    double s[4];
    HM_TRY(collect4(h, s));
    double c[4] = {s[0] / h->eps_Z, s[1] / h->eps_J, -s[2] / h->eps_J, s[3] / h->eps_M};
    if (jzc) for (int k = 0; k < 4; k++) jzc[k] = c[k];
    if (jz) *jz = ((c[0] + c[1]) + c[2]) + c[3];
    return HM_OK;
}

extern "C" int hm_j(hm_ctx_t h, const double *X, double deltaX, int i, int j, double *out)
{
    HM_ARG(h && X && out, "hm_j: NULL argument");
    HM_JOIN(h);
    HM_ARG(i >= 0 && i < 4 * h->N && j >= 0 && j < 4 * h->N, "hm_j: state index outside 0..%d", 4 * h->N - 1);
    NEED_REF(h, "hm_j");
    HM_HIP(hipSetDevice(h->device));
    std::vector<double> Xp(X, X + 4 * h->N), Xq(X, X + 4 * h->N);
    Xp[i] += deltaX;
    Xq[j] += deltaX;
    HM_TRY(render_into(h, Xp.data(), h->P));
    HM_HIP(hipStreamSynchronize(h->stream));     // d_X is reused by the second render
    HM_TRY(render_into(h, Xq.data(), h->Q));
    hipLaunchKernelGGL(k_j, dim3(h->red_blocks), dim3(RED_NT), 0, h->stream, h->ref, h->P, h->Q, h->W * h->H,
                       h->d_partial);
    double s[4];
    HM_TRY(collect4(h, s));
    *out = ((s[0] / h->eps_Z + s[1] / h->eps_J) + s[2] / h->eps_J) + s[3] / h->eps_M;
    return HM_OK;
}

// ---- the reference's multi-perturbation operators (cuda_multi.py:81-248, 721-845, 979-1129) ---------------------
// label palette, id images and per-label boxes of the renders involved; states: host copies of the 2 or 3 states
static int multi_setup(hm_ctx *h, const int32_t *labels, int n_labels, const double *const states[], int n_states)
{
    const size_t n = (size_t)h->W * h->H;
    for (int k = 0; k < 3; k++) HM_HIP(h->own.alloc(&h->d_ids[k], n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->d_labels, (size_t)h->T * sizeof(int)));
    HM_HIP(h->own.grow(&h->d_lbox, (size_t)n_labels * sizeof(int4)));
    HM_HIP(h->own.grow(&h->d_lout, (size_t)n_labels * 5 * sizeof(double)));
    std::vector<int4> box(n_labels, make_int4(1, 0, 1, 0));
    for (int t = 0; t < h->T; t++) {
        const int lab = labels[t];
        if (lab < 0) continue;
        HM_ARG(lab < n_labels && lab < 65535, "multi-perturbation label %d of triangle %d outside 0..%d", lab, t, n_labels - 1);
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (int sidx = 0; sidx < n_states; sidx++)
            for (int k = 0; k < 3; k++) {
                const int v = h->tri[3 * t + k];
                const double x = states[sidx][2 * v], y = states[sidx][2 * v + 1];
                x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            }
        if (!(x0 <= x1 && y0 <= y1)) continue;                              // non-finite state: nothing is drawn
        // pixel (c, r) is drawn iff its centre (c + .5, r + .5) is inside: one pixel of margin each way
        const int c0 = (int)std::max(0.0, std::floor(std::min(x0, (double)h->W)) - 1.0);
        const int c1 = (int)std::min((double)h->W - 1.0, std::ceil(std::max(x1, -1.0)) + 1.0);
        const int r0 = (int)std::max(0.0, std::floor(std::min(y0, (double)h->H)) - 1.0);
        const int r1 = (int)std::min((double)h->H - 1.0, std::ceil(std::max(y1, -1.0)) + 1.0);
        int4 &b = box[lab];
        if (b.x > b.y) b = make_int4(c0, c1, r0, r1);
        else b = make_int4(std::min(b.x, c0), std::max(b.y, c1), std::min(b.z, r0), std::max(b.w, r1));
    }
    HM_HIP(hipMemcpyAsync(h->d_labels, labels, (size_t)h->T * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(h->d_lbox, box.data(), (size_t)n_labels * sizeof(int4), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));                                   // box is a local
    return HM_OK;
}

// render state X (host) into target t with its id image (MODE 1), or the id image only (MODE 2)
static int render_ids(hm_ctx *h, const double *X, Targets t, int *ids, bool ids_only)
{
    HM_HIP(hipMemcpyAsync(h->d_X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    Mesh m = {h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    hipLaunchKernelGGL(k_setup_all, dim3(hm_cdiv(h->T, 64)), dim3(64), 0, h->stream, m, h->d_X, h->d_setup);
    const dim3 grid(hm_cdiv(h->W, EKF_TILE), hm_cdiv(h->H, EKF_TILE)), block(EKF_TILE, EKF_TILE);
    if (ids_only) hipLaunchKernelGGL((k_render<2>), grid, block, 0, h->stream, m, h->d_X, h->d_setup, t, (const int *)h->d_labels, ids);
    else hipLaunchKernelGGL((k_render<1>), grid, block, 0, h->stream, m, h->d_X, h->d_setup, t, (const int *)h->d_labels, ids);
    HM_HIP(hipGetLastError());
    HM_HIP(hipStreamSynchronize(h->stream));                                   // d_X is reused by the next render
    return HM_OK;
}

extern "C" int hm_jz_multi(hm_ctx_t h, const double *Xp, int masked, const int32_t *labels, int n_labels, double *hz,
                           double *hzc)
{
    HM_ARG(h && Xp && labels && hz && n_labels >= 1, "hm_jz_multi: bad argument");
    HM_JOIN(h);
    NEED_REF(h, "hm_jz_multi");
    HM_HIP(hipSetDevice(h->device));
    const double *states[2] = {h->X0.data(), Xp};
    HM_TRY(multi_setup(h, labels, n_labels, states, 2));
    int rc = render_ids(h, h->X0.data(), h->ref, h->d_ids[0], true);               // the reference render's ids (its targets stand)
    if (rc == HM_OK) rc = render_ids(h, Xp, h->P, h->d_ids[1], false);
    if (rc) return rc;
    MultiArgs a = {h->ref, h->P, h->P, h->d_ids[0], h->d_ids[1], h->d_ids[1], obs_of(h, masked), h->W, h->d_lbox, h->d_lout};
    hipLaunchKernelGGL(k_jz_multi, dim3(n_labels), dim3(RED_NT), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    h->h_lout.resize((size_t)n_labels * 5);
    HM_HIP(hipMemcpyAsync(h->h_lout.data(), h->d_lout, (size_t)n_labels * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    for (int l = 0; l < n_labels; l++) {
        const double *s = h->h_lout.data() + 4 * l;
        const double c[4] = {s[0] / h->eps_Z, s[1] / h->eps_J, -s[2] / h->eps_J, s[3] / h->eps_M};
        hz[l] = ((c[0] + c[1]) + c[2]) + c[3];
        if (hzc) for (int k = 0; k < 4; k++) hzc[4 * l + k] = c[k];
    }
    return HM_OK;
}

extern "C" int hm_j_multi(hm_ctx_t h, const double *X, double deltaX, int n_pairs, const int32_t *ee, const int32_t *labels,
                          int n_labels, double *hsum, double *nz, double *hcomp)
{
    HM_ARG(h && X && ee && labels && hsum && nz && n_pairs >= 1 && n_labels >= 1, "hm_j_multi: bad argument");
    HM_JOIN(h);
    NEED_REF(h, "hm_j_multi");
    HM_HIP(hipSetDevice(h->device));
    const int n4 = 4 * h->N;
    std::vector<double> Xp(X, X + n4), Xq(X, X + n4);
    for (int k = 0; k < n_pairs; k++) {
        HM_ARG(ee[2 * k] >= 0 && ee[2 * k] < n4 && ee[2 * k + 1] >= 0 && ee[2 * k + 1] < n4, "hm_j_multi: state index outside 0..%d", n4 - 1);
        Xp[ee[2 * k]] += deltaX;                                            // all first indices at once (cuda_multi.py:987-990)
        Xq[ee[2 * k + 1]] += deltaX;                                        // all second indices at once (:1004-1007)
    }
    const double *states[3] = {h->X0.data(), Xp.data(), Xq.data()};
    HM_TRY(multi_setup(h, labels, n_labels, states, 3));
    int rc = render_ids(h, h->X0.data(), h->ref, h->d_ids[0], true);
    if (rc == HM_OK) rc = render_ids(h, Xp.data(), h->P, h->d_ids[1], false);
    if (rc == HM_OK) rc = render_ids(h, Xq.data(), h->Q, h->d_ids[2], false);
    if (rc) return rc;
    MultiArgs a = {h->ref, h->P, h->Q, h->d_ids[0], h->d_ids[1], h->d_ids[2], obs_of(h, 0), h->W, h->d_lbox, h->d_lout};
    hipLaunchKernelGGL(k_j_multi, dim3(n_labels), dim3(RED_NT), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    h->h_lout.resize((size_t)n_labels * 5);
    HM_HIP(hipMemcpyAsync(h->h_lout.data(), h->d_lout, (size_t)n_labels * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    for (int l = 0; l < n_labels; l++) {
        const double *s = h->h_lout.data() + 5 * l;
        const double c[4] = {s[0] / h->eps_Z, s[1] / h->eps_J, s[2] / h->eps_J, s[3] / h->eps_M};
        hsum[l] = ((c[0] + c[1]) + c[2]) + c[3];
        nz[l] = s[4];
        if (hcomp) for (int k = 0; k < 4; k++) hcomp[4 * l + k] = c[k];
    }
    return HM_OK;
}

extern "C" int hm_error(hm_ctx_t h, const double *X, int masked, double err[4], float *fx, float *fy)
{
    HM_ARG(h && X && err, "hm_error: NULL argument");
    HM_JOIN(h);
    NEED_TEX(h, "hm_error");
    NEED_OBS(h, "hm_error");
    HM_HIP(hipSetDevice(h->device));
    // the launch and the order of additions of the update loop (k_render_iter, strip partials in the fixed two-level
    // order): the error of a state is the same number whether an iteration of hm_update_run reports it or this call
    HM_HIP(hipMemcpyAsync(h->d_X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HM_TRY(render_iter(h, h->d_X, h->P, true, masked, false, 2.0));
    const int n = h->W * h->H;
    if (fx) HM_HIP(hipMemcpyAsync(fx, h->P.fx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (fy) HM_HIP(hipMemcpyAsync(fy, h->P.fy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipMemcpyAsync(h->h_tpart.data(), h->d_tpart, (size_t)render_strips(h) * RI_NV * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(stream_wait(h->stream));
    double s6[RI_NV];
    hm_tile_partial_sums(h->h_tpart.data(), render_strips(h), s6);
    for (int k = 0; k < 4; k++) err[k] = s6[k];
    return HM_OK;
}

// render X as the reference, run the fused perturb-and-reduce kernel, unpack into d_H / d_Hz / d_Hzc
// the measurement at the device-resident state dX, whose render is (ref_ready) or is to be put in h->ref
// scatter: the job sums go to the dense HTH / Hz / Hzc (hm_measure); the update loop forms its system from the job
// sums directly (k_solve_prep) and leaves that launch out
static int measure_dev(hm_ctx *h, const double *dX, bool ref_ready, double deltaX, int masked, bool regions_ready = false,
                       bool scatter = true)
{
    if (!ref_ready) {                             // the reference render, and the star regions with it when they are wanted too
        HM_TRY(render_iter(h, dX, h->ref, false, masked, !regions_ready, deltaX));
        regions_ready = true;
    }
    MeasureArgs a;
    measure_args(h, dX, deltaX, masked, a);
    if (!regions_ready) hipLaunchKernelGGL(k_star_regions, dim3(h->N), dim3(REGION_NT), 0, h->stream, a, h->d_area);
    hipLaunchKernelGGL(k_measure_vertex, dim3(h->N, h->vsplit), dim3(MEAS_NT), 0, h->stream, a,
                       (const TriSetup *)h->d_cfgs, (const int4 *)h->d_ubox, (const unsigned *)h->d_tmask);
    if (h->E > 0) hipLaunchKernelGGL(k_measure_edge, dim3(h->E, h->esplit), dim3(MEAS_NT), 0, h->stream, a);
    if (scatter) {
        ScatterArgs s = {h->d_out, h->d_edges, h->N, h->E, h->vsplit, h->esplit, h->eps_Z, h->eps_J, h->eps_M, deltaX, h->d_HTH, h->d_Hz, h->d_Hzc};
        hipLaunchKernelGGL(k_hth_scatter, dim3(hm_cdiv(h->njobs, 4)), dim3(256), 0, h->stream, s);
    }
    HM_HIP(hipGetLastError());
    return HM_OK;
}

static void measure_args(hm_ctx *h, const double *dX, double deltaX, int masked, MeasureArgs &a)
{
    a.m = Mesh{h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    a.topo = StarTopo{h->d_star_off, h->d_star_tri, h->d_edges, h->E};
    a.ref = h->ref;
    a.obs = obs_of(h, masked);
    a.X = dX;
    a.delta = deltaX;
    a.out = h->d_out;
    a.pool = h->pool;
    a.vsplit = h->vsplit;
    a.esplit = h->esplit;
    a.iZ = 1.0 / h->eps_Z; a.iJ = 1.0 / h->eps_J; a.iM = 1.0 / h->eps_M;
    a.cfgs = h->d_cfgs;
    a.ubox = h->d_ubox;
    a.tmask = h->d_tmask;
    a.tlist = h->d_tlist;
    a.tcount = h->d_tcount;
    a.tmask_stride = TMASK_STRIDE;
}

static int measure_on_device(hm_ctx *h, const double *X, double deltaX, int masked, bool scatter = true)
{
    HM_HIP(hipMemcpyAsync(h->d_X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->X0.assign(X, X + 4 * h->N);
    h->have_ref = true;
    return measure_dev(h, h->d_X, false, deltaX, masked, false, scatter);
}

extern "C" int hm_measure(hm_ctx_t h, const double *X, double deltaX, int masked, double *Hz, double *Hzc, double *HTH)
{
    HM_ARG(h && X && Hz && HTH, "hm_measure: NULL argument");
    HM_JOIN(h);
    HM_ARG(deltaX > 0, "hm_measure: deltaX must be positive");
    NEED_TEX(h, "hm_measure");
    NEED_OBS(h, "hm_measure");
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = (size_t)4 * h->N;
    int *ovf = h->pin_scratch;
    for (int attempt = 0;; attempt++) {              // (once more after the pool has been grown)
        HM_TRY(measure_on_device(h, X, deltaX, masked));
        // the flag lands in the handle's pinned block, not in this frame: an error return below must not leave a
        // copy in flight towards a dead stack slot
        *ovf = 0;
        HM_HIP(hipMemcpyAsync(ovf, h->pool.overflow, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipStreamSynchronize(h->stream));
        if (!*ovf) break;
        if (attempt) { hm_set_error("hm_measure: the star regions do not fit the difference-image pool"); return HM_ERR_STATE; }
        HM_TRY(pool_grow(h, "hm_measure"));
    }
    HM_HIP(hipMemcpyAsync(Hz, h->d_Hz, n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Hzc) HM_HIP(hipMemcpyAsync(Hzc, h->d_Hzc, n4 * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipMemcpyAsync(HTH, h->d_HTH, n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

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

// the covariance half of hm_update_begin: the prior into d_Wprior, its factor, inv(W) into d_invW0
static int prior_inverse(hm_ctx *h, const double *W_prior, hipStream_t st = nullptr)
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
    h->pq_valid = false;
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

static int update_begin(hm_ctx *h, const double *W_prior, const double *X0);
extern "C" int hm_update_begin(hm_ctx_t h, const double *W_prior, const double *X0)
{
    HM_ARG(h && X0, "hm_update_begin: NULL argument");
    HM_JOIN(h);
    h->chain_pending = false;
    return update_begin(h, W_prior, X0);
}
// X0 == NULL: the prior mean is being left in d_X0 by hm_chain_project's kernel on the second stream
static int update_begin(hm_ctx *h, const double *W_prior, const double *X0)
{
    if (!W_prior && !h->d_Wres) {
        hm_set_error("hm_update_begin: no prior given and none resident on the device");
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    const int n4 = 4 * h->N;
    h->pq_valid = false;                         // (a prediction queued ahead that nobody took: d_Wres is still the posterior)
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
        HM_HIP(hipStreamWaitEvent(h->stream, h->ev_pm, 0));
    }
    h->upd_last = h->upd_prev = -1;
    h->upd_open = true;
    return HM_OK;
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
    int rc = HM_OK;
    const int slot = h->upd_last == 0 ? 1 : 0;
    for (int attempt = 0;; attempt++) {              // (once more after the pool of difference images has been grown)
    HM_TRY(measure_on_device(h, X, deltaX, masked, false));   // leaves X in d_X; the job sums go straight into the system
    double *rhs_row = solve_step(h, slot, deltaX);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(step, rhs_row, (size_t)n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Hzc) HM_HIP(hipMemcpyAsync(Hzc, h->d_Hzc, (size_t)n4 * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int *ovf = h->pin_scratch;                               // pinned, lives with the handle (see hm_measure)
    *ovf = 0;
    HM_HIP(hipMemcpyAsync(ovf, h->pool.overflow, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (err) {
        // Renderer.error of the new iterate X0 + step, without another host round trip: the launch and the order of
        // additions hm_update_run uses
        rc = render_iter(h, h->d_Xn, h->P, true, masked, false, deltaX);
        if (rc == HM_OK) {
            hipError_t e = hipMemcpyAsync(h->h_tpart.data(), h->d_tpart, (size_t)render_strips(h) * RI_NV * sizeof(double), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = stream_wait(h->stream);
            if (e != hipSuccess) { hm_set_error("hm_update_step: %s", hipGetErrorString(e)); rc = HM_ERR_HIP; }
            else { double s6[RI_NV]; hm_tile_partial_sums(h->h_tpart.data(), render_strips(h), s6); for (int k = 0; k < 4; k++) err[k] = s6[k]; }
        }
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }   // nothing of this call stays in flight
    } else {
        HM_HIP(hipStreamSynchronize(h->stream));
    }
    if (!*ovf) break;
    if (attempt) { hm_set_error("hm_update_step: the star regions do not fit the difference-image pool"); return HM_ERR_STATE; }
    HM_TRY(pool_grow(h, "hm_update_step"));
    }
    HM_TRY(flow_status(h, "hm_update_step"));
    h->upd_prev = h->upd_last;
    h->upd_last = slot;
    return HM_OK;
}

static int update_cov_on(hm_ctx *h, int which, double *W_out, hipStream_t st);
extern "C" int hm_update_cov(hm_ctx_t h, int which, double *W_out)
{
    HM_ARG(h != nullptr, "hm_update_cov: NULL handle");
    HM_JOIN(h);
    return update_cov_on(h, which, W_out, h->stream);
}
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
    const size_t n = (size_t)h->W * h->H;
    const size_t n4 = (size_t)4 * h->N, xb = n4 * sizeof(double);
    Outline o = {h->d_outline, h->d_outline_cnt, (int)n, h->d_pm_flag};
    if (!y_m) {
        // The mask of the resident observation: its outline was queued when the observation was set (or is now, the
        // first time); the state goes through page-locked memory both ways, the result as a block the host takes when
        // it is whole (host_block.h) -- one launch and no copy operations on the way (0.15 -> ~0.03 ms per frame of the streaming pipeline).
        if (!h->outline_ready) {
            HM_TRY(queue_outline(h, h->o_ym));
            h->outline_ready = true;
        }
        memcpy(h->pin_pm, X, xb);
        ProjArgs a = {h->d_pm_pruned, h->W, h->H, h->N, o, nullptr};
        hipLaunchKernelGGL(k_project_mask_host, dim3(h->N), dim3(PROJ_NT), 0, s, a, (const double *)h->pin_pm, h->pin_pm + n4, (double *)nullptr,
                           (double *)nullptr, h->d_pm_done, (double)(++h->pm_ticket), h->result_delay);
        HM_HIP(hipGetLastError());
        HM_TRY(hb_wait(s, h->pin_pm + n4, 0, n4 + 1, hb_stamp(h->pm_ticket), h->pmv.data(), "hm_project_mask"));
        const int nmoved = (int)h->pmv[n4];
        if (nmoved) memcpy(X, h->pmv.data(), xb);
        if (moved) *moved = nmoved;
        return HM_OK;
    }
    h->outline_ready = false;                    // the buffers are about to hold the outline of the caller's mask
    HM_HIP(h->own.alloc(&h->d_pm_mask, n));
    HM_HIP(hipMemcpyAsync(h->d_pm_mask, y_m, n, hipMemcpyHostToDevice, s));
    const uint8_t *mask = h->d_pm_mask;
    HM_TRY(queue_outline(h, mask));
    HM_HIP(hipMemcpyAsync(h->d_pm_X, X, xb, hipMemcpyHostToDevice, s));
    ProjArgs a = {h->d_pm_pruned, h->W, h->H, h->N, o, h->d_pm_X};
    hipLaunchKernelGGL(k_project_mask, dim3(h->N), dim3(PROJ_NT), 0, s, a);
    HM_HIP(hipGetLastError());
    int cnt[4] = {0, 0, 0, 0};
    HM_HIP(hipMemcpyAsync(cnt, h->d_outline_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HM_HIP(hipMemcpyAsync(X, h->d_pm_X, xb, hipMemcpyDeviceToHost, s));
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
    const size_t n = (size_t)h->W * h->H;
    h->outline_ready = false;                    // the buffers are about to hold the outline of the caller's mask
    HM_HIP(h->own.alloc(&h->d_pm_mask, n));
    HM_HIP(hipMemcpyAsync(h->d_pm_mask, y_m, n, hipMemcpyHostToDevice, h->stream2));
    HM_TRY(queue_outline(h, h->d_pm_mask));
    HM_HIP(hipMemcpyAsync(out, h->d_pm_pruned, n, hipMemcpyDeviceToHost, h->stream2));
    HM_HIP(hipStreamSynchronize(h->stream2));
    return HM_OK;
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

// IteratedKalmanFilter.update (kalman.py:774-831) in one call: hm_update_begin, up to max_iter
// hm_update_step's with the reference's acceptance logic between them, hm_update_cov of the state
// that is kept.  Per iteration the host sees one small result block (step, the four error sums)
// that the last kernel writes into pinned memory; the iterate itself never leaves the device, and
// the render that gave an iterate's error is the reference render of the next measurement.
extern "C" int hm_update_arm_newton(hm_ctx_t h, void *worker, int n_bars, const int32_t *bars, const double *l0, double kappa,
                                    double M, double dt, int maxiter, double tol)
{
    HM_ARG(h && worker && n_bars >= 0 && bars && l0, "hm_update_arm_newton: bad argument");
    HM_JOIN_LAZY(h);                               // (the tail of the last update still reads what this call replaces)
    h->armed.worker = worker;
    h->pn_bars.assign(bars, bars + 2 * (size_t)n_bars);
    h->pn_l0.assign(l0, l0 + n_bars);
    h->pn_par[0] = kappa; h->pn_par[1] = M; h->pn_par[2] = dt; h->pn_par[3] = tol;
    h->pn_maxiter = maxiter;
    h->armed.newton = true;
    return HM_OK;
}

// With hm_update_arm_newton armed as well: the next hm_update_run also queues the covariance half of the next frame's
// prediction (queue_predict_ahead above; eps_F as for hm_cov_predict) behind the covariance of the state it keeps.
// hm_update_cov is not available after such a run (the factor slots are reused); hm_cov_fetch still returns the
// posterior until hm_predict_take.
extern "C" int hm_update_arm_cov(hm_ctx_t h, double eps_F)
{
    HM_ARG(h != nullptr, "hm_update_arm_cov: NULL handle");
    h->armed.cov = true;
    h->pq_eps_F = eps_F;
    return HM_OK;
}

static int queue_predict_ahead(hm_ctx *h, const double *X, int n_bars, const int32_t *bars, const double *l0, double kappa,
                               double M, double dt, double eps_F, hipStream_t st);
static int prepare_mask(hm_ctx *h, const uint8_t *d_y_m);

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
    if (!h->tail_valid) {
        hm_set_error("hm_update_tail: the last hm_update_run on this handle did not succeed (or there was none)");
        return HM_ERR_STATE;
    }
    const size_t n4 = (size_t)4 * h->N;
    if (h->tail_pending) {
        HM_HIP(hipSetDevice(h->device));
        HM_TRY(hb_wait(h->tail_stream, h->pin + 2 * (n4 + RES_HEAD), 0, n4 * 7, hb_stamp(h->tail_ticket), h->tailv.data(), "hm_update_tail"));
        h->tail_pending = false;
    }
    if (Hzc) memcpy(Hzc, h->tailv.data(), n4 * 4 * sizeof(double));
    if (gains) memcpy(gains, h->tailv.data() + n4 * 4, n4 * 3 * sizeof(double));
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
    int r = hb_wait(h->stream3, h->pin_n4 + n4, 0, (size_t)n4 + 2, hb_stamp(h->n4_ticket), h->n4v.data(), "hm_update_run (state prediction)");
    h->n4_pending = false;
    if (r) return r;
    HM_TRY(hb_wait(h->stream3, h->pin_pm + n4, 0, (size_t)n4 + 1, hb_stamp(h->pm_ticket), h->pmv.data(), "hm_update_run (projectmask)"));
    h->chain_pred.assign(h->n4v.begin(), h->n4v.begin() + n4);
    h->chain_proj.assign(h->pmv.begin(), h->pmv.begin() + n4);
    h->chain_its = (int)h->n4v[n4];
    h->chain_moved = (int)h->pmv[n4];
    if (h->n4v[n4 + 1] != 0.0) return 2;
    u.X0 = h->chain_proj; u.Xcur = u.X0; u.Xold = u.X0;
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
    h->tail_valid = false;
    HM_JOIN_LAZY(h);                               // (the tail of the last update: waited for before the first solve)
    HM_ARG(u.a.deltaX > 0 && u.a.max_iter >= 0, "hm_update_run: deltaX must be positive, max_iter >= 0");
    u.chained = h->chain_pending;
    h->chain_pending = false;
    h->last_err_valid = false;
    h->pq_valid = false;                           // (after the join: the last update's tail may have queued a prediction)
    h->tail_pending = false;                       // (the block of the last update is about to be overwritten)
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
        MeasureArgs a;
        measure_args(h, h->d_X, u.a.deltaX, u.a.masked, a);
        hipLaunchKernelGGL(k_star_regions, dim3(h->N), dim3(REGION_NT), 0, h->stream, a, h->d_area);
        HM_HIP(hipGetLastError());
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
        HM_TRY(hm_ms_newton_start(u.armed.worker, h->N, (int)h->pn_l0.size(), h->pn_bars.data(), h->pn_l0.data(), h->pn_par[0],
                                  h->pn_par[1], h->pn_par[2], h->pn_maxiter, h->pn_par[3], u.Xcur.data()));
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
// prediction ahead; on stream4 the ev_tail record.  Before them, on the second stream, the next frame's outline.  Waits
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
        HM_TRY(queue_predict_ahead(h, Xk.data(), (int)h->pn_l0.size(), h->pn_bars.data(), h->pn_l0.data(), h->pn_par[0],
                                   h->pn_par[1], h->pn_par[2], j.eps_F, j.ts));
    if (j.ts != h->stream) {
        HM_HIP(hipEventRecord(h->ev_tail, j.ts));
        h->tail_on_stream4 = true;
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
    // The tail runs on a stream of its own (stream4) when the caller does not want the covariance on the host: everything
    // it reads is complete -- the host has seen the result block of the last iteration, whose kernel is behind all of
    // them on `stream` -- and what is still queued on `stream` (the measurement of an iteration that does not happen)
    // and what the next frame queues there first (reference render, measurement) touch none of its buffers; `stream` waits
    // for its end (ev_tail, on the device) before the next solve (ctx_join).
    hipStream_t ts = h->stream;
    HM_TRY(ctx_join(h));                           // (a tail nobody has joined since: an update without iterations)
    if (!u.a.W_out && h->tail_split) {
        HM_HIP(h->own.stream(&h->stream4));
        HM_HIP(h->own.event(&h->ev_tail));
        ts = h->stream4;
    }
    const long long ticket = u.niter > 0 ? ++h->run_ticket : h->run_ticket;
    const bool ahead = u.armed.cov && u.armed.newton && h->chol_flow && which >= 0 && u.niter > 0 && !u.a.W_out;
    const TailJob job = {h, u.next_mask, which, ts, u.niter, n4, u.pin_tail(), ticket, u.a.W_out, ahead, h->pq_eps_F};
    u.stage[3] = u.ms();
    if (u.niter > 0 && !u.a.W_out && !u.a.Hzc && !u.a.gains) {
        // nobody wants the gains now: they are taken when asked for (hm_update_tail) and the caller gets on with its next
        // frame -- the tail's ~20 launches are queued by the handle's helper thread (every entry point joins it first)
        h->tail_pending = true;
        h->tail_ticket = ticket;
        h->tail_stream = ts;
        if (h->tail_async) {
            h->helper_used = true;
            h->helper.post([job, Xk = u.Xcur]() { return tail_launches(job, Xk); });
        } else {
            HM_TRY(tail_launches(job, u.Xcur));
        }
    } else if (u.niter > 0 && !u.a.W_out) {
        HM_TRY(tail_launches(job, u.Xcur));
        HM_TRY(hb_wait(ts, job.pin_tail, 0, (size_t)n4 * 7, hb_stamp(ticket), h->tailv.data(), "hm_update_run"));
    } else {
        HM_TRY(tail_launches(job, u.Xcur));
        HM_HIP(stream_wait(ts));
        if (u.niter > 0 && !hb_take(job.pin_tail, 0, (size_t)n4 * 7, hb_stamp(ticket), h->tailv.data())) {
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
        if (u.a.Hzc) memcpy(u.a.Hzc, h->tailv.data(), n4 * 4 * sizeof(double));
        if (u.a.gains) memcpy(u.a.gains, h->tailv.data() + n4 * 4, n4 * 3 * sizeof(double));
    } else {
        if (u.a.Hzc) memset(u.a.Hzc, 0, n4 * 4 * sizeof(double));
        if (u.a.gains) memset(u.a.gains, 0, n4 * 3 * sizeof(double));
        std::fill(h->tailv.begin(), h->tailv.end(), 0.0);
    }
    h->tail_valid = true;                          // (taken, queued for hm_update_tail, or zeros)
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

// (spring_csr, spring_blocks: ctx.h)
// Covariance prediction W' = F W F^T + Weps (kalman.py:717, 863) on the device.
//   W_in   : the covariance to propagate (host), or NULL to use the one hm_update_cov returned last,
//            which is still on the device;
//   bars / blocks : the springs and, per spring, the symmetric 2x2 block (Bxx, Bxy, Byy) of the force
//            Jacobian at the state before the step; n_bars = 0 gives the constant-velocity F (A = 0);
//   a, s   : F = [[I, a I], [s dfdy, I]];  eps_F : Weps = eps_F [[I/4, I/2], [I/2, I]].
// The result is copied to W_out and stays on the device as the prior of the next hm_update_begin(NULL).
// ahead: called by hm_update_run for the NEXT frame, behind launches that are still running -- nothing here may wait for
// the stream: the spring blocks go through page-locked memory (`blocks` is h->pin_blk), the result goes straight to
// d_Wprior (where prior_inverse wants it) and the resident covariance (d_Wres, the posterior the caller may still
// fetch) is left alone.
static int cov_predict_core(hm_ctx *h, const double *W_in, int n_bars, const int32_t *bars, const double *blocks,
                            double a, double s, double eps_F, double *W_out, bool ahead, hipStream_t st = nullptr)
{
    if (!st) st = h->stream;
    const int N = h->N, n4 = 4 * N;
    const size_t nn = (size_t)n4 * n4 * sizeof(double);
    std::vector<int> &off = h->sp_h_off, &bar = h->sp_h_bar, &other = h->sp_h_other;   // live until the copies ran
    if (!ahead) HM_HIP(stream_wait(st));      // ... of the previous call
    // the springs' topology rarely changes between frames: its device copy is kept and only the per-spring blocks go up
    const bool same_topo = h->d_sp_off && h->sp_bars_cached.size() == 2 * (size_t)n_bars &&
                           (n_bars == 0 || memcmp(h->sp_bars_cached.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0);
    if (!same_topo) {
        for (int i = 0; i < n_bars; i++)
            HM_ARG(bars[2 * i] >= 0 && bars[2 * i] < N && bars[2 * i + 1] >= 0 && bars[2 * i + 1] < N,
                   "hm_cov_predict: spring %d refers to a vertex outside 0..%d", i, N - 1);
        spring_csr(N, n_bars, bars, off, bar, other);
        HM_HIP(h->own.alloc(&h->d_sp_off, (size_t)(N + 1) * sizeof(int)));
        HM_HIP(h->own.grow(&h->d_sp_bar, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->d_sp_other, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->d_sp_blk, 3 * (size_t)n_bars * sizeof(double)));
        HM_HIP(hipMemcpyAsync(h->d_sp_off, off.data(), (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
        if (n_bars > 0) {
            HM_HIP(hipMemcpyAsync(h->d_sp_bar, bar.data(), bar.size() * sizeof(int), hipMemcpyHostToDevice, st));
            HM_HIP(hipMemcpyAsync(h->d_sp_other, other.data(), other.size() * sizeof(int), hipMemcpyHostToDevice, st));
        }
        h->sp_bars_cached.assign(bars, bars + 2 * (size_t)n_bars);
    }
    if (n_bars > 0) {
        const double *from = blocks;
        if (!ahead) {
            h->sp_h_blk.assign(blocks, blocks + 3 * (size_t)n_bars);
            from = h->sp_h_blk.data();
        }
        HM_HIP(hipMemcpyAsync(h->d_sp_blk, from, 3 * (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const double *src = h->d_Wres;
    if (W_in) {
        HM_HIP(hipMemcpyAsync(h->d_H, W_in, nn, hipMemcpyHostToDevice, st));
        src = h->d_H;
    } else if (src == h->d_Wtmp) {               // the output buffer: move the input out of the way
        HM_HIP(hipMemcpyAsync(h->d_H, h->d_Wtmp, nn, hipMemcpyDeviceToDevice, st));
        src = h->d_H;
    }
    SpringTopo tp = {h->d_sp_off, h->d_sp_bar, h->d_sp_other, h->d_sp_blk};
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
    h->pq_valid = false;                         // a prediction queued ahead (hm_update_arm_cov) is not what this caller wants
    return cov_predict_core(h, W_in, n_bars, bars, blocks, a, s, eps_F, W_out, false);
}

// hm_update_run, armed by hm_update_arm_newton + hm_update_arm_cov, when its state is final and the covariance of that
// state (d_Wres) is queued: the covariance half of the NEXT frame's prediction -- W' = F W F^T + Weps with F at this
// state (hm_cov_predict) and the factorisation / inverse of W' the next update starts with (hm_update_prefactor) --
// goes onto the stream right behind it, ~0.3 ms before the caller could ask for it (it first has to get back to
// IteratedMSKalmanFilter.predict).  Nothing is made current: hm_predict_take does that when the caller's inputs turn
// out to be the ones used here; otherwise the caller's own hm_cov_predict starts from the posterior, which is intact.
static int queue_predict_ahead(hm_ctx *h, const double *X, int n_bars, const int32_t *bars, const double *l0, double kappa,
                               double M, double dt, double eps_F, hipStream_t st)
{
    for (int i = 0; i < 2 * n_bars; i++)
        if (bars[i] < 0 || bars[i] >= h->N) return HM_OK;                 // the caller's own hm_cov_predict reports it
    HM_HIP(h->own.host_grow(&h->pin_blk, 3 * (size_t)n_bars * sizeof(double), hipHostMallocDefault));
    spring_blocks(n_bars, bars, l0, kappa, X, h->pin_blk);
    double *const post = h->d_Wres;
    HM_TRY(cov_predict_core(h, nullptr, n_bars, bars, h->pin_blk, dt, dt / M, eps_F, nullptr, true, st));
    h->d_Wres = h->d_Wprior;                     // (prior_inverse: the prior is where it belongs already)
    const int rc = prior_inverse(h, nullptr, st);
    h->d_Wres = post;
    if (rc) return rc;
    h->upd_open = false;                         // the factor slots and d_Wprior belong to the next update now
    h->pq_X.assign(X, X + 4 * (size_t)h->N);
    h->pq_bars.assign(bars, bars + 2 * (size_t)n_bars);
    h->pq_l0.assign(l0, l0 + n_bars);
    h->pq_par[0] = kappa; h->pq_par[1] = dt; h->pq_par[2] = dt / M; h->pq_par[3] = eps_F;
    h->pq_valid = true;
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
    if (!h->pq_valid) return 1;
    h->pq_valid = false;
    const size_t n4 = (size_t)4 * h->N;
    const bool same = h->pq_X.size() == n4 && memcmp(h->pq_X.data(), X, n4 * sizeof(double)) == 0 &&
                      h->pq_l0.size() == (size_t)n_bars &&
                      (n_bars == 0 || (memcmp(h->pq_bars.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0 &&
                                       memcmp(h->pq_l0.data(), l0, (size_t)n_bars * sizeof(double)) == 0)) &&
                      h->pq_par[0] == kappa && h->pq_par[1] == a && h->pq_par[2] == s && h->pq_par[3] == eps_F;
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
        if (!h->newton_ready) {
            HM_HIP(h->own.alloc(&h->d_nX, (size_t)n4 * sizeof(double)));
            HM_HIP(h->own.alloc(&h->d_nvoff, (size_t)(N + 1) * sizeof(int)));
            HM_HIP(h->own.alloc(&h->d_ninfo, 2 * sizeof(int)));
            HM_HIP(hipFuncSetAttribute((const void *)k_ms_newton, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            h->newton_ready = true;
        }
        HM_HIP(h->own.grow(&h->d_nbars, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->d_nvbar, 2 * (size_t)n_bars * sizeof(int)));
        HM_HIP(h->own.grow(&h->d_nl0, (size_t)n_bars * sizeof(double)));
        std::vector<int> off(N + 1, 0), vbar(2 * (size_t)n_bars);
        for (int i = 0; i < n_bars; i++) { off[bars[2 * i] + 1]++; off[bars[2 * i + 1] + 1]++; }
        for (int v = 0; v < N; v++) off[v + 1] += off[v];
        {
            std::vector<int> fill(off.begin(), off.end() - 1);
            for (int i = 0; i < n_bars; i++) { vbar[fill[bars[2 * i]]++] = i; vbar[fill[bars[2 * i + 1]]++] = i; }   // ascending per vertex
        }
        HM_HIP(hipMemcpyAsync(h->d_nbars, bars, 2 * (size_t)n_bars * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->d_nl0, l0, (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->d_nvoff, off.data(), (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->d_nvbar, vbar.data(), vbar.size() * sizeof(int), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipMemcpyAsync(h->d_nX, X, (size_t)n4 * sizeof(double), hipMemcpyHostToDevice, h->stream2));
        HM_HIP(hipStreamSynchronize(h->stream2));            // off / vbar are locals (pageable copies have returned anyway)
        NewtonArgs a = {N, n_bars, h->d_nbars, h->d_nl0, h->d_nvoff, h->d_nvbar, kappa, M, dt, tol, maxiter,
                        (int)std::ceil(1.0 / dt), h->d_nX, h->d_ninfo};
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
        hipError_t e = hipMemcpyAsync(X, h->d_nX, (size_t)n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream2);
        if (e == hipSuccess) e = hipMemcpyAsync(info, h->d_ninfo, sizeof info, hipMemcpyDeviceToHost, h->stream2);
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
    if (h->n4_pending) {                          // a prediction nobody fetched: let it finish (its result block is dropped)
        HM_HIP(hipStreamSynchronize(h->stream3));
        h->n4_pending = false;
    }
    if (!h->n4_ready) {
        HM_HIP(h->own.stream(&h->stream3));
        // page-locked and coherent (hipHostMalloc without flags already is: the flag states the intent, it was not the
        // cause of round 3's wrong tracks -- host_block.h has that story): [X in (4N) | a result block of 4N + 2 values]
        const size_t words = (size_t)4 * N + 2 * ((size_t)4 * N + 2);
        HM_HIP(h->own.host_alloc(&h->pin_n4, words * sizeof(double), hipHostMallocCoherent));
        memset(h->pin_n4, 0, words * sizeof(double));
        HM_HIP(h->own.alloc(&h->d_n4X, ((size_t)4 * N + 2) * sizeof(double)));
        h->n4v.assign((size_t)4 * N + 2, 0.0);
        HM_HIP(h->own.event(&h->ev_n4));
        h->n4_ready = true;
    }
    const bool same = h->n4_bars.size() == 2 * (size_t)n_bars && memcmp(h->n4_bars.data(), bars, 2 * (size_t)n_bars * sizeof(int32_t)) == 0;
    if (!same) {
        for (int i = 0; i < 2 * n_bars; i++) HM_ARG(bars[i] >= 0 && bars[i] < N, "hm_newton_dev_start: bar refers to vertex %d", bars[i]);
        std::vector<int> deg(N, 0);
        for (int i = 0; i < 2 * n_bars; i++) deg[bars[i]]++;
        const int maxdeg = *std::max_element(deg.begin(), deg.end());
        h->n4_bars.clear();                       // (the springs of the table once it is on the device)
        h->n4_l0.clear();
        h->n4deg = maxdeg <= 8 ? 8 : maxdeg <= 12 ? 12 : 0;
        if (h->n4deg) {
            const int D = h->n4deg;
            std::vector<int> nbr((size_t)N * D), nbb((size_t)N * D, n_bars), fill(N, 0);
            for (int v = 0; v < N; v++)
                for (int q = 0; q < D; q++) nbr[(size_t)v * D + q] = v;             // padding: the vertex itself, bar I (zero terms)
            for (int i = 0; i < n_bars; i++) {                                        // ascending bar order per vertex
                const int a = bars[2 * i], b = bars[2 * i + 1];
                nbr[(size_t)a * D + fill[a]] = b; nbb[(size_t)a * D + fill[a]++] = i;
                nbr[(size_t)b * D + fill[b]] = a; nbb[(size_t)b * D + fill[b]++] = i;
            }
            HM_HIP(h->own.alloc(&h->d_n4nbr, (size_t)N * 12 * sizeof(int)));
            HM_HIP(h->own.alloc(&h->d_n4nbb, (size_t)N * 12 * sizeof(int)));
            HM_HIP(h->own.grow(&h->d_n4bars, 2 * (size_t)n_bars * sizeof(int)));
            HM_HIP(h->own.grow(&h->d_n4l0, (size_t)n_bars * sizeof(double)));
            // on the kernel's own stream and waited for (nbr / nbb are locals): ordered before the launch by the stream
            // itself rather than by hipMemcpy's return (that was not the cause of round 3's wrong tracks either -- a track
            // uploads these tables once, the wrong predictions came at frame 13 -- but it is the form that needs no argument)
            HM_HIP(hipMemcpyAsync(h->d_n4nbr, nbr.data(), nbr.size() * sizeof(int), hipMemcpyHostToDevice, h->stream3));
            HM_HIP(hipMemcpyAsync(h->d_n4nbb, nbb.data(), nbb.size() * sizeof(int), hipMemcpyHostToDevice, h->stream3));
            HM_HIP(hipMemcpyAsync(h->d_n4bars, bars, 2 * (size_t)n_bars * sizeof(int), hipMemcpyHostToDevice, h->stream3));
            HM_HIP(hipStreamSynchronize(h->stream3));            // (nbr / nbb are locals)
        }
        h->n4_bars.assign(bars, bars + 2 * (size_t)n_bars);
    }
    if (!h->n4deg) return 1;
    if (h->n4_l0.size() != (size_t)n_bars || memcmp(h->n4_l0.data(), l0, (size_t)n_bars * sizeof(double)) != 0) {
        h->n4_l0.assign(l0, l0 + n_bars);
        HM_HIP(hipMemcpyAsync(h->d_n4l0, h->n4_l0.data(), (size_t)n_bars * sizeof(double), hipMemcpyHostToDevice, h->stream3));
        HM_HIP(hipStreamSynchronize(h->stream3));
    }
    const size_t n4 = (size_t)4 * N;
    memcpy(h->pin_n4, X, n4 * sizeof(double));
    Newton4Args a;
    a.N = N; a.I = n_bars; a.deg_stride = h->n4deg;
    a.bars = h->d_n4bars; a.l0 = h->d_n4l0; a.nbr = h->d_n4nbr; a.nbb = h->d_n4nbb;
    a.kappa = kappa; a.M = M; a.dt = dt; a.tol = tol; a.maxiter = maxiter; a.steps = (int)std::ceil(1.0 / dt);
    a.Xin = h->pin_n4; a.out = h->pin_n4 + n4; a.dev_out = h->d_n4X; a.ticket = (double)(++h->n4_ticket);
    a.delay_us = h->result_delay; a.force_bad = h->newton_fail;
    const size_t lds = ((size_t)6 * NEWTON4_NT + 4 * ((size_t)n_bars + 1) + 4 * (NEWTON4_NT / 64)) * sizeof(double) + 2 * (size_t)n_bars * sizeof(int);
    if (lds > 64 * 1024) return 1;
    if (h->n4deg == 8) hipLaunchKernelGGL((k_ms_newton4<8>), dim3(1), dim3(NEWTON4_NT), lds, h->stream3, a);
    else hipLaunchKernelGGL((k_ms_newton4<12>), dim3(1), dim3(NEWTON4_NT), lds, h->stream3, a);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->ev_n4, h->stream3));
    h->n4_pending = true;
    h->chain_pending = false;
    return HM_OK;
}

// Waits for the launch of hm_newton_dev_start; X (4N) receives the advanced state.  Returns 1 when the kernel's inner solve
// did not converge (never observed): the caller repeats the prediction on the host.
extern "C" int hm_newton_dev_finish(hm_ctx_t h, double *X, int *newton_iterations)
{
    HM_ARG(h && X, "hm_newton_dev_finish: bad argument");
    if (!h->n4_pending) { hm_set_error("hm_newton_dev_finish: no prediction was started"); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    const size_t n4 = (size_t)4 * h->N;
    // the kernel's result block, taken when it is whole (host_block.h); the kernel is usually long done when this is
    // called (it was started at the end of the previous update)
    const int rc = hb_wait(h->stream3, h->pin_n4 + n4, 0, n4 + 2, hb_stamp(h->n4_ticket), h->n4v.data(), "hm_newton_dev_finish");
    h->n4_pending = false;
    h->chain_pending = false;
    if (rc) return rc;
    if (h->n4v[n4 + 1] != 0.0) return 1;
    memcpy(X, h->n4v.data(), n4 * sizeof(double));
    if (newton_iterations) *newton_iterations = (int)h->n4v[n4];
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
    if (!h->n4_pending || !h->d_n4X) return 1;
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    if (!h->outline_ready) {
        HM_TRY(queue_outline(h, h->o_ym));
        h->outline_ready = true;
    }
    const size_t n4 = (size_t)4 * h->N;
    Outline o = {h->d_outline, h->d_outline_cnt, h->W * h->H, h->d_pm_flag};
    ProjArgs a = {h->d_pm_pruned, h->W, h->H, h->N, o, nullptr};
    // on the prediction's own stream, right behind its kernel (no hop between streams there); the outline of the mask was
    // queued on the second stream when the observation was set, or a frame ahead (hm_prepare_mask)
    HM_HIP(hipStreamWaitEvent(h->stream3, h->ev_outline, 0));
    hipLaunchKernelGGL(k_project_mask_host, dim3(h->N), dim3(PROJ_NT), 0, h->stream3, a, (const double *)h->d_n4X, h->pin_pm + n4, h->d_X0,
                       h->d_X, h->d_pm_done, (double)(++h->pm_ticket), h->result_delay);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->ev_pm, h->stream3));
    h->chain_pending = true;
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
        h->prepared_mask = nullptr;
        return HM_OK;
    }
    return prepare_mask(h, d_y_m);
}
static int prepare_mask(hm_ctx *h, const uint8_t *d_y_m)
{
    HM_HIP(hipSetDevice(h->device));
    HM_TRY(ensure_stream2(h));
    HM_TRY(project_buffers(h));
    // the projection of the CURRENT frame may still be reading the outline buffers on the prediction's stream
    if (h->ev_pm && h->pm_ticket > 0) HM_HIP(hipStreamWaitEvent(h->stream2, h->ev_pm, 0));
    HM_TRY(queue_outline(h, d_y_m));
    h->outline_ready = false;                    // (the buffers no longer hold the outline of the observation in place)
    h->prepared_mask = d_y_m;
    return HM_OK;
}

// What the last chained hm_update_run started from: the predicted state, the projected state (its prior mean), the
// Newton iterations of the prediction, the vertices projectmask moved.  Any pointer may be NULL.
extern "C" int hm_chain_states(hm_ctx_t h, double *predicted, double *projected, int *newton_iterations, int *moved)
{
    HM_ARG(h != nullptr, "hm_chain_states: NULL handle");
    const size_t n4 = (size_t)4 * h->N;
    if (h->chain_pred.size() != n4 || h->chain_proj.size() != n4) { hm_set_error("hm_chain_states: no chained update has run"); return HM_ERR_STATE; }
    if (predicted) memcpy(predicted, h->chain_pred.data(), n4 * sizeof(double));
    if (projected) memcpy(projected, h->chain_proj.data(), n4 * sizeof(double));
    if (newton_iterations) *newton_iterations = h->chain_its;
    if (moved) *moved = h->chain_moved;
    return HM_OK;
}
