// EKF measurement model on MI355X: host orchestration and C-ABI (include/hydra_mi.h).
// Replaces reference renderer.py (OpenGL rasteriser), cuda.py and cuda_multi.py
// (reduction kernels + PBO plumbing).  In this order: the pool of difference images, handle lifetime and tuning, texture and
// observation, the renders, the measurement operators.  The kernels are in ekf_kernels.h, which this translation unit alone
// compiles; readout.hip queues two of them through ekf_queue_setup_all and ekf_queue_render, and update.hip reaches the
// measurement through the hidden functions declared at the end of ctx.h.  The filter's other translation units: update.hip
// (the dense update, hm_update_run), mask.hip (pruning, outline, projection), predict_dev.hip (covariance and state
// prediction); the smoother is in smooth.hip.
// Of the handle (ctx.h) it writes the flat fields of the mesh, the observation, the renders and the measurement, the pool
// and `multi`; of the others' only d_X, last_err_valid (cleared) and, when the observation changes, mask.outline_ready /
// mask.prepared.
#include "ctx.h"
#include "ekf_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

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
int pool_grow(hm_ctx *h, const char *who)
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
    // the last frame (it writes into newton4.pin), and so may be launches of an update that ended in an error
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
        h->tail.v.assign(n4 * 7, 0.0);
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
// and k_chol_flow those of its chain -- each translation unit has a pointer of its own
extern "C" int hm_debug_stamps(void *dev_ptr)
{
    long long *p = (long long *)dev_ptr;
    HM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), &p, sizeof p));
    return update_debug_stamps(p);                // (the factorisation chain's stamps go behind the render's, same buffer)
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
    {"tail_async", 0, 1, 1, TUNE_SET(tail.async), "must be 0 or 1"},          // same results either way
    {"tail_split", 0, 1, 1, TUNE_SET(tail.split), "must be 0 or 1"},          // same results either way
    {"newton_fail", 0, 1, 1, TUNE_SET(newton4.fail), "must be 0 or 1"},        // tests only: the device predictions report a failed inner solve
    {"speculate", 0, 1, 1, TUNE_SET(speculate), "must be 0 or 1"},            // same results either way
    {"body_stats_cap", 1, BODY_STATS_CAP, 1, TUNE_SET(body.stats_cap), nullptr},   // tests only: frames one hm_body_stats accumulation takes
    // entries of a column per wave of k_deep_cols (hm_deep_body_run; same bytes for every value)
    {"deep_col_entries", DEEP_COL_ENTRIES_MIN, DEEP_COL_ENTRIES_MAX, 1, TUNE_SET(body.deep_col_entries), nullptr},
    {"body_rec_chunk", 0, INT32_MAX, 1, TUNE_SET(rec.chunk), "must be >= 0 (0: the default size)"},   // tests only: frames per chunk of the next hm_body_rec_begin
    {"rec_tp_frames", 1, REC_TP_MAX, 1, TUNE_SET(rec.tp_frames), nullptr},     // frames per workgroup of hm_body_rec_trace_products
    // frames per run of the running baseline, the residual planes, the trace maps, the surrogate reduction (same results for every value)
    {"rec_bl_frames", 1, REC_BL_MAX, 1, TUNE_SET(rec.bl_frames), nullptr},
    {"rec_res_frames", 1, REC_RES_MAX, 1, TUNE_SET(rec.res_frames), nullptr},
    {"rec_map_frames", 1, REC_MAP_MAX, 1, TUNE_SET(rec.map_frames), nullptr},
    {"rec_null_frames", 1, REC_NULL_MAX, 1, TUNE_SET(rec.null_frames), nullptr},
    {"rec_tm_frames", 1, REC_TM_MAX, 1, TUNE_SET(rec.tm_frames), nullptr},      // likewise: the maps against the pixel's own triangle
    {"rec_wv_frames", 1, REC_WV_MAX, 1, TUNE_SET(rec.wv_frames), nullptr},      // events per launch of hm_body_rec_waves (same bytes for every value)
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
    h->mask.outline_ready = false;
    if (h->mask.d_outline) {              // a tracker that projects onto the mask: its outline, ahead of hm_project_mask
        HM_TRY(queue_outline(h, h->o_ym));
        h->mask.outline_ready = true;
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
    h->mask.outline_ready = false;
    if (h->mask.d_outline && h->mask.prepared == d_y_m) {      // hm_prepare_mask queued the outline of exactly this mask ahead
        h->mask.outline_ready = true;
    } else if (h->mask.d_outline) {       // as in hm_set_observation: the caller's mask is complete in device memory by contract
        HM_TRY(queue_outline(h, h->o_ym));
        h->mask.outline_ready = true;
    }
    h->mask.prepared = nullptr;
    return HM_OK;
}

// ---- what the launches below are given: mesh, observation, the measurement's arguments; a host state into d_X ------------------
static Mesh mesh_of(const hm_ctx *h) { return Mesh{h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex}; }

static Obs obs_of(const hm_ctx *h, int masked)
{
    return Obs{h->o_yim, masked ? h->d_yfxm : h->o_yfx, masked ? h->d_yfym : h->o_yfy, h->o_ym};
}

static void measure_args(hm_ctx *h, const double *dX, double deltaX, int masked, MeasureArgs &a)
{
    a.m = mesh_of(h);
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

// the host state X (4N doubles) into d_X on the handle's stream; d_X is free again when that copy has run
static int state_upload(hm_ctx *h, const double *X)
{
    HM_HIP(hipMemcpyAsync(h->d_X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return HM_OK;
}

// render the device-resident state dX into target t (k_setup_all + k_render<0>)
static int render_dev(hm_ctx *h, const double *dX, Targets t)
{
    const Mesh m = mesh_of(h);
    hipLaunchKernelGGL(k_setup_all, dim3(hm_cdiv(h->T, 64)), dim3(64), 0, h->stream, m, dX, h->d_setup);
    hipLaunchKernelGGL((k_render<0>), dim3(hm_cdiv(h->W, EKF_TILE), hm_cdiv(h->H, EKF_TILE)), dim3(EKF_TILE, EKF_TILE), 0,
                       h->stream, m, dX, h->d_setup, t, (const int *)nullptr, (int *)nullptr);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// render state X (host, 4N doubles) into target t on the handle's stream
static int render_into(hm_ctx *h, const double *X, Targets t)
{
    HM_TRY(state_upload(h, X));
    return render_dev(h, h->d_X, t);
}

int render_strips(const hm_ctx *h) { return hm_cdiv(h->W, RI_W) * hm_cdiv(h->H, h->render_rows); }

// The render of the device-resident state dX into target t as ONE launch (k_render_iter): triangle setups made per
// tile, optionally the per-tile partial sums of Renderer.error against the observation (d_tpart) and, riding along
// as extra workgroups, the star regions of the measurement at dX (they read nothing but the state).
int render_iter(hm_ctx *h, const double *dX, Targets t, bool with_err, int masked, bool regions, double deltaX)
{
    IterRenderArgs r;
    r.m = mesh_of(h);
    r.X = dX;
    r.out = t;
    r.o = obs_of(h, masked);
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

// The four sums of Renderer.error of the last render_iter(..., with_err) on the stream: its strip partials copied to the
// host, waited for and added up in that fixed order.  When it fails the stream is waited for: nothing stays in flight.
int render_error_sums(hm_ctx *h, const char *who, double err[4])
{
    const int strips = render_strips(h);
    hipError_t e = hipMemcpyAsync(h->h_tpart.data(), h->d_tpart, (size_t)strips * RI_NV * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = stream_wait(h->stream);
    if (e != hipSuccess) {
        hm_set_error("%s: %s", who, hipGetErrorString(e));
        (void)hipStreamSynchronize(h->stream);
        return HM_ERR_HIP;
    }
    double s6[RI_NV];
    hm_tile_partial_sums(h->h_tpart.data(), strips, s6);
    for (int k = 0; k < 4; k++) err[k] = s6[k];
    return HM_OK;
}

// Four sums weighted as the reference weights the terms of H^T z and H^T H: c = s0 / eps_Z, s1 / eps_J, +-s2 / eps_J,
// s3 / eps_M (negate2: the third term enters with a minus sign), and their sum from left to right.
static inline double weighted_terms(const hm_ctx *h, const double s[4], bool negate2, double c[4])
{
    c[0] = s[0] / h->eps_Z;
    c[1] = s[1] / h->eps_J;
    c[2] = (negate2 ? -s[2] : s[2]) / h->eps_J;
    c[3] = s[3] / h->eps_M;
    return ((c[0] + c[1]) + c[2]) + c[3];
}

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
    double c[4];
    const double sum = weighted_terms(h, s, true, c);
    if (jzc) for (int k = 0; k < 4; k++) jzc[k] = c[k];
    if (jz) *jz = sum;
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
    double c[4];
    *out = weighted_terms(h, s, false, c);
    return HM_OK;
}

// ---- the reference's multi-perturbation operators (cuda_multi.py:81-248, 721-845, 979-1129) ---------------------
// label palette, id images and per-label boxes of the renders involved; states: host copies of the 2 or 3 states
static int multi_setup(hm_ctx *h, const int32_t *labels, int n_labels, const double *const states[], int n_states)
{
    const size_t n = (size_t)h->W * h->H;
    for (int k = 0; k < 3; k++) HM_HIP(h->own.alloc(&h->multi.d_ids[k], n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->multi.d_labels, (size_t)h->T * sizeof(int)));
    HM_HIP(h->own.grow(&h->multi.d_lbox, (size_t)n_labels * sizeof(int4)));
    HM_HIP(h->own.grow(&h->multi.d_lout, (size_t)n_labels * 5 * sizeof(double)));
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
    HM_HIP(hipMemcpyAsync(h->multi.d_labels, labels, (size_t)h->T * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(h->multi.d_lbox, box.data(), (size_t)n_labels * sizeof(int4), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));                                   // box is a local
    return HM_OK;
}

// render state X (host) into target t with its id image (MODE 1), or the id image only (MODE 2)
static int render_ids(hm_ctx *h, const double *X, Targets t, int *ids, bool ids_only)
{
    HM_TRY(state_upload(h, X));
    const Mesh m = mesh_of(h);
    hipLaunchKernelGGL(k_setup_all, dim3(hm_cdiv(h->T, 64)), dim3(64), 0, h->stream, m, h->d_X, h->d_setup);
    const dim3 grid(hm_cdiv(h->W, EKF_TILE), hm_cdiv(h->H, EKF_TILE)), block(EKF_TILE, EKF_TILE);
    if (ids_only) hipLaunchKernelGGL((k_render<2>), grid, block, 0, h->stream, m, h->d_X, h->d_setup, t, (const int *)h->multi.d_labels, ids);
    else hipLaunchKernelGGL((k_render<1>), grid, block, 0, h->stream, m, h->d_X, h->d_setup, t, (const int *)h->multi.d_labels, ids);
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
    int rc = render_ids(h, h->X0.data(), h->ref, h->multi.d_ids[0], true);               // the reference render's ids (its targets stand)
    if (rc == HM_OK) rc = render_ids(h, Xp, h->P, h->multi.d_ids[1], false);
    if (rc) return rc;
    MultiArgs a = {h->ref, h->P, h->P, h->multi.d_ids[0], h->multi.d_ids[1], h->multi.d_ids[1], obs_of(h, masked), h->W, h->multi.d_lbox, h->multi.d_lout};
    hipLaunchKernelGGL(k_jz_multi, dim3(n_labels), dim3(RED_NT), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    h->multi.h_lout.resize((size_t)n_labels * 5);
    HM_HIP(hipMemcpyAsync(h->multi.h_lout.data(), h->multi.d_lout, (size_t)n_labels * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    for (int l = 0; l < n_labels; l++) {
        double c[4];
        hz[l] = weighted_terms(h, h->multi.h_lout.data() + 4 * l, true, c);
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
    int rc = render_ids(h, h->X0.data(), h->ref, h->multi.d_ids[0], true);
    if (rc == HM_OK) rc = render_ids(h, Xp.data(), h->P, h->multi.d_ids[1], false);
    if (rc == HM_OK) rc = render_ids(h, Xq.data(), h->Q, h->multi.d_ids[2], false);
    if (rc) return rc;
    MultiArgs a = {h->ref, h->P, h->Q, h->multi.d_ids[0], h->multi.d_ids[1], h->multi.d_ids[2], obs_of(h, 0), h->W, h->multi.d_lbox, h->multi.d_lout};
    hipLaunchKernelGGL(k_j_multi, dim3(n_labels), dim3(RED_NT), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    h->multi.h_lout.resize((size_t)n_labels * 5);
    HM_HIP(hipMemcpyAsync(h->multi.h_lout.data(), h->multi.d_lout, (size_t)n_labels * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    for (int l = 0; l < n_labels; l++) {
        const double *s = h->multi.h_lout.data() + 5 * l;
        double c[4];
        hsum[l] = weighted_terms(h, s, false, c);
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
    HM_TRY(state_upload(h, X));
    HM_TRY(render_iter(h, h->d_X, h->P, true, masked, false, 2.0));
    const int n = h->W * h->H;
    if (fx) HM_HIP(hipMemcpyAsync(fx, h->P.fx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (fy) HM_HIP(hipMemcpyAsync(fy, h->P.fy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return render_error_sums(h, "hm_error", err);
}

// k_star_regions at the device-resident state dX alone (the regions otherwise ride along with that state's render_iter)
int queue_star_regions(hm_ctx *h, const double *dX, double deltaX, int masked)
{
    MeasureArgs a;
    measure_args(h, dX, deltaX, masked, a);
    hipLaunchKernelGGL(k_star_regions, dim3(h->N), dim3(REGION_NT), 0, h->stream, a, h->d_area);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// The measurement at the device-resident state dX: its render is in h->ref (ref_ready) or is put there, its star regions
// are there (regions_ready) or are computed, then the fused perturb-and-reduce kernels.  scatter: the job sums go to the
// dense HTH / Hz / Hzc (hm_measure); the update loop forms its system from the job sums directly (k_solve_prep) and leaves
// that launch out.
int measure_dev(hm_ctx *h, const double *dX, bool ref_ready, double deltaX, int masked, bool regions_ready, bool scatter)
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

// the measurement at the host state X: it goes into d_X and is the state of the reference render from here on
int measure_on_device(hm_ctx *h, const double *X, double deltaX, int masked, bool scatter)
{
    HM_TRY(state_upload(h, X));
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
    HM_TRY(with_pool_retry(h, "hm_measure", [&]() -> int {
        HM_TRY(measure_on_device(h, X, deltaX, masked));
        HM_TRY(pool_flag_queue(h));
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }));
    HM_HIP(hipMemcpyAsync(Hz, h->d_Hz, n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Hzc) HM_HIP(hipMemcpyAsync(Hzc, h->d_Hzc, n4 * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipMemcpyAsync(HTH, h->d_HTH, n4 * n4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}
