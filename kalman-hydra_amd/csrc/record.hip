// The registered video kept on the device (hm_body_rec_*): the record itself, the reductions over it, its residual motion
// (match, shift, field, warp), the running baseline, the events per pixel, the residual of the cells' model and the activity waves.  Host orchestration and C-ABI
// (include/hydra_mi.h); the kernels are in roi_kernels.h, stab_kernels.h, detrend_kernels.h, events_kernels.h, residual_kernels.h and
// network_kernels.h, network_null_kernels.h, deform_kernels.h, gram_kernels.h and waves_kernels.h, which this translation unit alone compiles.  Of the handle (ctx.h) it uses
// rec, the body map (body.tri, body.h_tri), the
// registered plane (body.reg) and the statistics' counters, and reads W, H, device, own and stream.  readout.hip queues the
// warp: it reserves a frame's slot and queues the copy into it through body_rec_slot and body_rec_queue_copy, and this file
// reaches the body map and the statistics through body_map_build and body_stats_queue_add (ctx.h).
#include "ctx.h"
#include "roi_kernels.h"
#include "stab_kernels.h"
#include "detrend_kernels.h"
#include "events_kernels.h"
#include "residual_kernels.h"
#include "network_kernels.h"
#include "network_null_kernels.h"
#include "deform_kernels.h"
#include "gram_kernels.h"
#include "waves_kernels.h"
#include <cmath>
#include <algorithm>
#include <cstring>

#define REC_CHUNK_BYTES ((size_t)64 << 20)
#define REC_MAX_FRAMES (1 << 24)

// ---- what the calls below are made of ---------------------------------------------------------------------------------
// frame k of the record (device)
static uint8_t *rec_frame(const hm_ctx *h, int k)
{
    const RecBox &b = h->rec.box;
    const int ch = k / b.fpc;
    return h->rec.chunks[ch] + (size_t)(k - ch * b.fpc) * b.fs;
}

static int rec_range_ok(const hm_ctx *h, const char *who, int k0, int n)
{
    HM_ARG(k0 >= 0 && n >= 0 && k0 <= h->rec.frames && n <= h->rec.frames - k0, "%s: frames %d .. %d of a record of %d", who, k0,
           k0 + n - 1, h->rec.frames);
    return HM_OK;
}

// one box frame on the device -> a full W x H plane of the caller's, 0 outside the box
static int rec_expand(const hm_ctx *h, const uint8_t *d_src, uint8_t *out_plane)
{
    const RecBox &b = h->rec.box;
    memset(out_plane, 0, (size_t)h->W * h->H);
    HM_HIP(hipMemcpy2D(out_plane + (size_t)b.r0 * h->W + b.c0, (size_t)h->W, d_src, (size_t)b.pitch, (size_t)b.bw, (size_t)b.bh,
                       hipMemcpyDeviceToHost));
    return HM_OK;
}

// the patches of B x B pixels that cover the box
struct RecGrid { int npx, npy, np; };
static RecGrid rec_grid(const RecBox &b, int B)
{
    const int npx = hm_cdiv(b.bw, B), npy = hm_cdiv(b.bh, B);
    return RecGrid{npx, npy, npx * npy};
}

static int stab_patch_ok(const char *who, int B)
{
    HM_ARG(B >= STAB_BMIN && B <= STAB_BMAX, "%s: patch size %d outside %d..%d", who, B, STAB_BMIN, STAB_BMAX);
    return HM_OK;
}

// a dword per thread of `frames` box frames
static dim3 rec_dword_grid(const RecBox &b, int frames = 1) { return dim3(hm_cdiv((b.pitch >> 2) * b.bh, 256), std::min(frames, 65535)); }

// Scratch for `want` frames in the record's layout -- as many of them as rec.scr_bytes hold, one at least -- around
// body(per): rec.scr is there while it runs and freed when it returns, on the error paths too, once nothing queued reads
// it any more.  The first error is the one reported.
template <typename Body>
static int rec_with_scratch(hm_ctx *h, int want, Body body)
{
    const RecBox &b = h->rec.box;
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(want, 1), h->rec.scr_bytes / b.fs));
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    const int rc = body(per);
    if (rc) (void)hipStreamSynchronize(h->stream);
    const hipError_t fe = h->own.free(&h->rec.scr);
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

// The frames k0 .. k0 + n - 1 as planes of some kind, in runs of at most `per`: fill(k, m, dst) queues the planes of frames
// k .. k + m - 1 into the scratch, take(j, d_frame) gets the plane of frame k0 + j -- once the run is there if `wait`,
// else take queues behind it.
template <typename Fill, typename Take>
static int rec_runs(hm_ctx *h, int per, int k0, int n, bool wait, Fill fill, Take take)
{
    for (int k = 0; k < n;) {
        const int m = std::min(per, n - k);
        HM_TRY(fill(k0 + k, m, h->rec.scr));
        if (wait) HM_HIP(hipStreamSynchronize(h->stream));
        for (int j = 0; j < m; j++) HM_TRY(take(k + j, (const uint8_t *)(h->rec.scr + (size_t)j * h->rec.box.fs)));
        k += m;
    }
    return HM_OK;
}

// The whole record rewritten in place, in runs of at most `per` frames within a chunk: a run is copied aside as it is, then
// launch(grid, src, dst, k, m) queues the kernel that writes frames k .. k + m - 1 (at dst) from the copy (src).
template <typename Launch>
static int rec_rewrite(hm_ctx *h, int per, Launch launch)
{
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    for (int k = 0; k < F;) {
        const int m = std::min(per, std::min(F, (k / b.fpc + 1) * b.fpc) - k);
        uint8_t *dst = rec_frame(h, k);
        HM_HIP(hipMemcpyAsync(h->rec.scr, dst, (size_t)m * b.fs, hipMemcpyDeviceToDevice, h->stream));
        launch(rec_dword_grid(b, m), (const uint8_t *)h->rec.scr, dst, k, m);
        HM_HIP(hipGetLastError());
        k += m;
    }
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// the statistics are on and have room for every frame of the record
static int rec_stats_open(hm_ctx *h, const char *who)
{
    if (!h->body.stats_on) { hm_set_error("%s: no statistics (hm_body_stats_begin first)", who); return HM_ERR_STATE; }
    if (h->body.stats_frames + h->rec.frames > h->body.stats_cap) {
        hm_set_error("%s: the statistics hold %d frames and the record %d, their capacity is %d (sums of 32 bits are exact up to %d "
                     "frames): nothing added", who, h->body.stats_frames, h->rec.frames, h->body.stats_cap, BODY_STATS_CAP);
        return HM_ERR_STATE;
    }
    return HM_OK;
}

// a box frame pasted into the registered plane, then added to the statistics as a warp's frame is
static int rec_stats_add_plane(hm_ctx *h, const uint8_t *d_box_frame)
{
    const int n = h->W * h->H;
    hipLaunchKernelGGL(k_rec_paste, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W, h->rec.box, d_box_frame,
                       h->body.reg);
    return body_stats_queue_add(h, h->body.reg);
}

// ---- the record: begin, end, the slot and the copy of every warp, fetch (roi_kernels.h) -------------------------------
// stop recording and free the record (the caller has checked that there is one)
static int body_rec_drop(hm_ctx *h)
{
    h->rec.on = false;
    h->rec.frames = 0;
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipStreamSynchronize(h->stream));
    hipError_t e = hipSuccess;
    for (uint8_t *&c : h->rec.chunks) {
        const hipError_t e1 = h->own.free(&c);
        if (e == hipSuccess) e = e1;
    }
    h->rec.chunks.clear();
    if (e == hipSuccess) e = h->own.free(&h->rec.tab);
    if (e == hipSuccess) e = h->own.free(&h->rec.tmp);       // (rec.scr: no call leaves it behind)
    if (e == hipSuccess && !h->body.stats_on) e = h->own.free(&h->body.reg);     // (BodyState::reg has the rule)
    HM_HIP(e);
    return HM_OK;
}

extern "C" int hm_body_rec_begin(hm_ctx_t h, uint64_t max_bytes)
{
    HM_ARG(h != nullptr, "hm_body_rec_begin: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_map_build(h));
    if (h->rec.on) HM_TRY(body_rec_drop(h));
    const size_t n = (size_t)h->W * h->H;
    if (h->body.h_tri.empty()) {
        h->body.h_tri.resize(n);
        HM_HIP(hipMemcpyAsync(h->body.h_tri.data(), h->body.tri, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipStreamSynchronize(h->stream));
    }
    int c0 = h->W, c1 = -1, r0 = h->H, r1 = -1;
    for (int r = 0; r < h->H; r++)
        for (int c = 0; c < h->W; c++)
            if (h->body.h_tri[(size_t)r * h->W + c] >= 0) {
                c0 = std::min(c0, c); c1 = std::max(c1, c);
                r0 = std::min(r0, r); r1 = std::max(r1, r);
            }
    if (c1 < 0) c0 = c1 = r0 = r1 = 0;          // (an empty map: one pixel, registered as 0)
    RecBox &b = h->rec.box;
    b.c0 = c0; b.r0 = r0; b.bw = c1 - c0 + 1; b.bh = r1 - r0 + 1;
    b.pitch = (b.bw + 3) & ~3;
    b.fs = ((size_t)b.pitch * b.bh + 15) & ~(size_t)15;
    b.fpc = h->rec.chunk > 0 ? h->rec.chunk : (int)std::max<size_t>(1, REC_CHUNK_BYTES / b.fs);
    h->rec.max = max_bytes;
    h->rec.cap = (int)std::min<unsigned long long>(max_bytes / b.fs, REC_MAX_FRAMES);
    HM_HIP(h->own.alloc(&h->body.reg, n));
    h->rec.frames = 0;
    h->rec.on = true;
    return HM_OK;
}

extern "C" int hm_body_rec_end(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_body_rec_end: NULL handle");
    HM_JOIN_LAZY(h);
    if (!h->rec.on) return HM_OK;
    return body_rec_drop(h);
}

extern "C" int hm_body_rec_count(hm_ctx_t h, int *frames)
{
    HM_ARG(h && frames, "hm_body_rec_count: NULL argument");
    HM_JOIN_LAZY(h);
    *frames = h->rec.on ? h->rec.frames : 0;
    return HM_OK;
}

int body_rec_slot(hm_ctx *h, const char *who, uint8_t **dst)
{
    const RecBox &b = h->rec.box;
    if (h->rec.frames >= h->rec.cap) {
        hm_set_error("%s: the record holds %d frames of %zu bytes (a box of %d x %d pixels) and its budget of %llu bytes holds "
                     "%d: nothing appended", who, h->rec.frames, b.fs, b.bw, b.bh, h->rec.max, h->rec.cap);
        return HM_ERR_STATE;
    }
    const int ch = h->rec.frames / b.fpc;
    if (ch == (int)h->rec.chunks.size()) {
        const int frames = std::min(b.fpc, h->rec.cap - ch * b.fpc);
        uint8_t *p = nullptr;
        HM_HIP(h->own.alloc(&p, (size_t)frames * b.fs));
        h->rec.chunks.push_back(p);
    }
    *dst = rec_frame(h, h->rec.frames);
    return HM_OK;
}

int body_rec_queue_copy(hm_ctx *h, uint8_t *dst)
{
    hipLaunchKernelGGL(k_rec_copy, rec_dword_grid(h->rec.box), dim3(256), 0, h->stream, h->W, h->rec.box,
                       (const uint8_t *)h->body.reg, dst);
    HM_HIP(hipGetLastError());
    h->rec.frames++;
    return HM_OK;
}

static int body_rec_begun(hm_ctx *h, const char *who)
{
    if (!h->rec.on) { hm_set_error("%s: no record (hm_body_rec_begin first)", who); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    return HM_OK;
}

extern "C" int hm_body_rec_fetch(hm_ctx_t h, int k0, int n, uint8_t *out)
{
    HM_ARG(h != nullptr, "hm_body_rec_fetch: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_begun(h, "hm_body_rec_fetch"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_fetch", k0, n));
    HM_ARG(out || n == 0, "hm_body_rec_fetch: NULL output");
    HM_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < n; k++) HM_TRY(rec_expand(h, rec_frame(h, k0 + k), out + (size_t)k * h->W * h->H));
    return HM_OK;
}

// ---- the reductions over the record (roi_kernels.h) -------------------------------------------------------------------
// a reduction may start: there are frames, and the chunks' addresses are on the device
static int body_rec_ready(hm_ctx *h, const char *who)
{
    HM_TRY(body_rec_begun(h, who));
    if (h->rec.frames < 1) { hm_set_error("%s: no frame recorded since hm_body_rec_begin", who); return HM_ERR_STATE; }
    const size_t bytes = h->rec.chunks.size() * sizeof(uint8_t *);
    HM_HIP(h->own.grow(&h->rec.tab, bytes));       // (every reduction waits for its results: nothing in flight reads it)
    HM_HIP(hipMemcpyAsync(h->rec.tab, h->rec.chunks.data(), bytes, hipMemcpyHostToDevice, h->stream));
    return HM_OK;
}

// the reductions' buffers, carved from one allocation (16-byte aligned pieces)
struct RecCarve {
    uint8_t *base;
    size_t off;
    template <typename T> T *take(size_t count)
    {
        off = (off + 15) & ~(size_t)15;
        T *p = base ? (T *)(base + off) : nullptr;      // (no allocation yet: the pieces are only measured)
        off += count * sizeof(T);
        return p;
    }
};
// Lay a reduction's buffers out in rec.tmp: `lay` takes its pieces from the RecCarve it is given, first to measure them,
// then, once the allocation holds them all, for their addresses.
template <typename Lay>
static int body_rec_carve(hm_ctx *h, Lay lay)
{
    RecCarve cv = {nullptr, 0};
    lay(cv);
    HM_HIP(h->own.grow(&h->rec.tmp, cv.off));
    cv = {h->rec.tmp, 0};
    lay(cv);
    return HM_OK;
}

extern "C" int hm_body_rec_label_sums(hm_ctx_t h, const int32_t *labels, int L, uint64_t *out)
{
    HM_ARG(labels && out && L >= 1, "hm_body_rec_label_sums: NULL argument or %d labels", L);
    HM_ARG(h != nullptr, "hm_body_rec_label_sums: NULL handle");
    const size_t n = (size_t)h->W * h->H;
    HM_TRY(hm_labels_ok("hm_body_rec_label_sums", 0, labels, n, L));
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_label_sums"));
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames, nb = b.pitch * b.bh;
    int *d_img = nullptr, *d_lab = nullptr;
    unsigned long long *d_sum = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_img = cv.take<int>(n);
        d_lab = cv.take<int>(nb);
        d_sum = cv.take<unsigned long long>((size_t)F * L);
    }));
    HM_HIP(hipMemcpyAsync(d_img, labels, n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(d_sum, 0, (size_t)F * L * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_rec_box_labels, dim3(hm_cdiv(nb, 256)), dim3(256), 0, h->stream, h->W, b, (const int *)h->body.tri,
                       (const int *)d_img, d_lab);
    hipLaunchKernelGGL(k_rec_label_sums, dim3(hm_cdiv(nb >> 2, 256), std::min(F, 1024)), dim3(256), 0, h->stream, b,
                       (const uint8_t *const *)h->rec.tab, F, (const int *)d_lab, L, d_sum);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, d_sum, (size_t)F * L * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// What the reductions over seeds open with, in this order: the helper joined, a record with frames whose chunk table is on
// the device (body_rec_ready), every seed a pixel of the map, and F P below 2^30 (the kernels index frame x seed in an int).
static int body_rec_seeded(hm_ctx *h, int P, const int32_t *seeds, const char *who)
{
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, who));
    for (int s = 0; s < P; s++) {
        const int c = seeds[2 * s], r = seeds[2 * s + 1];
        if (!(c >= 0 && c < h->W && r >= 0 && r < h->H && h->body.h_tri[(size_t)r * h->W + c] >= 0)) {
            hm_set_error("%s: seed %d (column %d, row %d) is not a pixel of the body map", who, s, c, r);
            return HM_ERR_ARG;
        }
    }
    HM_ARG((long long)h->rec.frames * P < (1ll << 30), "%s: %d frames x %d seeds", who, h->rec.frames, P);
    return HM_OK;
}

extern "C" int hm_body_rec_seed_sums(hm_ctx_t h, int P, const int32_t *seeds, double r_disc, double r_in, double r_out, int R,
                                     uint32_t *n_T, uint32_t *n_G, uint64_t *T, uint64_t *G, int64_t *U, uint64_t *w1,
                                     uint64_t *w2, int64_t *c, int64_t *u1, int64_t *u2)
{
    HM_ARG(P >= 1 && seeds, "hm_body_rec_seed_sums: %d seeds", P);
    HM_ARG(r_disc >= 0.0 && r_disc <= REC_RMAX && r_in >= 0.0 && r_in <= r_out && r_out <= REC_RMAX,
           "hm_body_rec_seed_sums: radii %g, %g, %g (need 0 <= r_disc <= %d and 0 <= r_in <= r_out <= %d)", r_disc, r_in, r_out,
           REC_RMAX, REC_RMAX);
    HM_ARG(R >= 0 && R <= REC_WIN_RMAX, "hm_body_rec_seed_sums: window radius %d outside 0..%d", R, REC_WIN_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_seed_sums: NULL handle");
    HM_TRY(body_rec_seeded(h, P, seeds, "hm_body_rec_seed_sums"));
    const int F = h->rec.frames;
    // the pixels of every disc and ring, and the bound that keeps sum U^2 exact: |U| <= 255 n_T n_G
    const double rd2 = r_disc * r_disc, ri2 = r_in * r_in, ro2 = r_out * r_out;
    const int Rg = (int)std::max(r_disc, r_out);
    std::vector<unsigned> cnt(2 * (size_t)P, 0);
    for (int s = 0; s < P; s++) {
        for (int dy = -Rg; dy <= Rg; dy++)
            for (int dx = -Rg; dx <= Rg; dx++) {
                const int x = seeds[2 * s] + dx, y = seeds[2 * s + 1] + dy;
                if (x < 0 || x >= h->W || y < 0 || y >= h->H || h->body.h_tri[(size_t)y * h->W + x] < 0) continue;
                const double d2 = (double)(dx * dx + dy * dy);
                if (d2 <= rd2) cnt[s]++;
                if (d2 >= ri2 && d2 <= ro2) cnt[P + s]++;
            }
        const unsigned __int128 m = (unsigned __int128)255 * cnt[s] * cnt[P + s];
        HM_ARG(m * m * (unsigned __int128)F < ((unsigned __int128)1 << 63),
               "hm_body_rec_seed_sums: seed %d: F (255 n_T n_G)^2 = %d (255 x %u x %u)^2 could pass 2^63", s, F, cnt[s], cnt[P + s]);
    }
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    RecSeeds g;
    RecWin q;
    int2 *d_seeds = nullptr;
    unsigned *d_cnt = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_cnt = cv.take<unsigned>(2 * (size_t)P);
        g.T = cv.take<unsigned long long>(fp);
        g.G = cv.take<unsigned long long>(fp);
        g.U = cv.take<long long>(fp);
        q.w1 = cv.take<unsigned long long>(P * nw);
        q.w2 = cv.take<unsigned long long>(P * nw);
        q.c = cv.take<long long>(P * nw);
        q.u1 = cv.take<long long>(P);
        q.u2 = cv.take<long long>(P);
    }));
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_cnt, cnt.data(), 2 * (size_t)P * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.P = P; g.R = Rg;
    g.seeds = d_seeds; g.rd2 = rd2; g.ri2 = ri2; g.ro2 = ro2; g.nT = d_cnt; g.nG = d_cnt + P;
    hipLaunchKernelGGL(k_rec_seed_traces, dim3(hm_cdiv((int)fp, 4)), dim3(256), 0, h->stream, g);
    q.b = h->rec.box; q.chunks = g.chunks; q.F = F; q.P = P; q.R = R; q.seeds = d_seeds; q.U = g.U;
    hipLaunchKernelGGL(k_rec_window_sums, dim3(hm_cdiv((int)nw, 256), P), dim3(256), 0, h->stream, q);
    HM_HIP(hipGetLastError());
    if (n_T) memcpy(n_T, cnt.data(), (size_t)P * sizeof(uint32_t));
    if (n_G) memcpy(n_G, cnt.data() + P, (size_t)P * sizeof(uint32_t));
    if (T) HM_HIP(hipMemcpyAsync(T, g.T, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (G) HM_HIP(hipMemcpyAsync(G, g.G, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (U) HM_HIP(hipMemcpyAsync(U, g.U, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (w1) HM_HIP(hipMemcpyAsync(w1, q.w1, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (w2) HM_HIP(hipMemcpyAsync(w2, q.w2, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (c) HM_HIP(hipMemcpyAsync(c, q.c, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (u1) HM_HIP(hipMemcpyAsync(u1, q.u1, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
    if (u2) HM_HIP(hipMemcpyAsync(u2, q.u2, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_weighted_sums(hm_ctx_t h, int P, const int32_t *seeds, int R, const uint16_t *weights, uint64_t *out)
{
    HM_ARG(P >= 1 && seeds && weights && out, "hm_body_rec_weighted_sums: NULL argument or %d seeds", P);
    HM_ARG(R >= 0 && R <= REC_RMAX, "hm_body_rec_weighted_sums: window radius %d outside 0..%d", R, REC_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_weighted_sums: NULL handle");
    HM_TRY(body_rec_seeded(h, P, seeds, "hm_body_rec_weighted_sums"));
    const int F = h->rec.frames;
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    int2 *d_seeds = nullptr;
    uint16_t *d_w = nullptr;
    unsigned long long *d_out = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_w = cv.take<uint16_t>(P * nw);
        d_out = cv.take<unsigned long long>(fp);
    }));
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_w, weights, P * nw * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_rec_weighted_sums, dim3(hm_cdiv((int)fp, 4)), dim3(256), 0, h->stream, h->rec.box,
                       (const uint8_t *const *)h->rec.tab, F, P, R, (const int2 *)d_seeds, (const uint16_t *)d_w, d_out);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, d_out, fp * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_trace_products(hm_ctx_t h, int P, const int32_t *seeds, int R, const int32_t *q, int64_t *out)
{
    HM_ARG(P >= 1 && seeds && q && out, "hm_body_rec_trace_products: NULL argument or %d seeds", P);
    HM_ARG(R >= 0 && R <= REC_WIN_RMAX, "hm_body_rec_trace_products: window radius %d outside 0..%d", R, REC_WIN_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_trace_products: NULL handle");
    HM_TRY(body_rec_seeded(h, P, seeds, "hm_body_rec_trace_products"));
    const int F = h->rec.frames;
    // |v q| <= 255 x 2^31 per frame
    HM_ARG((unsigned __int128)F * 255u * ((unsigned __int128)1 << 31) < ((unsigned __int128)1 << 63),
           "hm_body_rec_trace_products: F x 255 x 2^31 = %d x 255 x 2^31 could pass 2^63", F);
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    const int tiles = hm_cdiv((int)nw, 64);
    HM_ARG((long long)P * tiles < (1ll << 31), "hm_body_rec_trace_products: %d seeds x %d tiles of the window", P, tiles);
    RecTP g;
    int2 *d_seeds = nullptr;
    int *d_q = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_q = cv.take<int>(fp);
        g.out = cv.take<unsigned long long>(P * nw);
    }));
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_q, q, fp * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, P * nw * sizeof(unsigned long long), h->stream));
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.P = P; g.R = R;
    g.tpf = h->rec.tp_frames; g.seeds = d_seeds; g.q = d_q;
    const int runs = hm_cdiv(F, g.tpf);
    hipLaunchKernelGGL(k_rec_trace_products, dim3(P * tiles, std::min(runs, 65535)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, P * nw * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// ---- every trace against every pixel of the record (network_kernels.h) ------------------------------------------------
// planes of the box on the device (rows of b.pitch values of 8 or 4 bytes) -> full W x H planes of the caller's, 0 outside the box
template <typename T>
static int rec_expand_planes(const hm_ctx *h, const T *d_src, int planes, void *out)
{
    const RecBox &b = h->rec.box;
    const size_t n = (size_t)h->W * h->H, nb = (size_t)b.pitch * b.bh, es = sizeof(T);
    memset(out, 0, (size_t)planes * n * es);
    for (int s = 0; s < planes; s++)
        HM_HIP(hipMemcpy2D((T *)out + (size_t)s * n + (size_t)b.r0 * h->W + b.c0, (size_t)h->W * es, d_src + (size_t)s * nb,
                           (size_t)b.pitch * es, (size_t)b.bw * es, (size_t)b.bh, hipMemcpyDeviceToHost));
    return HM_OK;
}

extern "C" int hm_body_rec_trace_maps(hm_ctx_t h, int L, const int32_t *q, int64_t *c, uint64_t *w1, uint64_t *w2)
{
    HM_ARG(L >= 1 && L <= REC_MAP_LMAX, "hm_body_rec_trace_maps: %d traces outside 1..%d", L, REC_MAP_LMAX);
    HM_ARG(h && q, "hm_body_rec_trace_maps: NULL handle or traces");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_trace_maps"));
    const int F = h->rec.frames;
    // |F c| and |w1 u1| <= F^2 x 255 x 32767
    HM_ARG((unsigned __int128)F * F * 255u * (unsigned)REC_MAP_QMAX < ((unsigned __int128)1 << 63),
           "hm_body_rec_trace_maps: F x F x 255 x 32767 = %d x %d x 255 x 32767 could pass 2^63", F, F);
    const size_t fl = (size_t)F * L;
    for (size_t i = 0; i < fl; i++)
        HM_ARG(q[i] >= -REC_MAP_QMAX && q[i] <= REC_MAP_QMAX, "hm_body_rec_trace_maps: q %d (frame %zu, trace %zu) outside -%d..%d",
               (int)q[i], i / (size_t)L, i % (size_t)L, REC_MAP_QMAX, REC_MAP_QMAX);
    if (!(c || w1 || w2)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const RecBox &b = h->rec.box;
    const size_t nb = (size_t)b.pitch * b.bh;
    const int groups = c ? hm_cdiv(L, REC_MAP_GROUP) : 1, runs = hm_cdiv(F, h->rec.map_frames);
    RecMaps g;
    int *d_q = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_q = cv.take<int>(c ? fl : 0);
        g.c = c ? cv.take<unsigned long long>((size_t)L * nb) : nullptr;
        g.w1 = w1 || w2 ? cv.take<unsigned long long>(nb) : nullptr;
        g.w2 = w1 || w2 ? cv.take<unsigned long long>(nb) : nullptr;
    }));
    if (c) {
        HM_HIP(hipMemcpyAsync(d_q, q, fl * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HM_HIP(hipMemsetAsync(g.c, 0, (size_t)L * nb * 8, h->stream));
    }
    if (g.w1) {
        HM_HIP(hipMemsetAsync(g.w1, 0, nb * 8, h->stream));
        HM_HIP(hipMemsetAsync(g.w2, 0, nb * 8, h->stream));
    }
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.L = L; g.run = h->rec.map_frames; g.q = d_q;
    hipLaunchKernelGGL(k_rec_trace_maps, dim3(hm_cdiv((int)(nb >> 2), 256), std::min(runs, 65535), groups), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipStreamSynchronize(h->stream));
    if (c) HM_TRY(rec_expand_planes(h, g.c, L, c));
    if (w1) HM_TRY(rec_expand_planes(h, g.w1, 1, w1));
    if (w2) HM_TRY(rec_expand_planes(h, g.w2, 1, w2));
    return HM_OK;
}

extern "C" int hm_body_rec_trace_null(hm_ctx_t h, int L, const int32_t *q, const double *vb, double *tmax, double *tmin,
                                      uint32_t *ge, uint32_t *le)
{
    HM_ARG(L >= 2 && L <= REC_NULL_LMAX, "hm_body_rec_trace_null: %d traces outside 2..%d", L, REC_NULL_LMAX);
    HM_ARG(h && q && vb, "hm_body_rec_trace_null: NULL handle, traces or variances");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_trace_null"));
    const int F = h->rec.frames;
    // |F c| and |w1 u1| <= F^2 x 255 x 32767
    HM_ARG((unsigned __int128)F * F * 255u * (unsigned)REC_MAP_QMAX < ((unsigned __int128)1 << 63),
           "hm_body_rec_trace_null: F x F x 255 x 32767 = %d x %d x 255 x 32767 could pass 2^63", F, F);
    const size_t fl = (size_t)F * L;
    std::vector<long long> u1((size_t)L, 0);
    std::vector<int> q0((size_t)F);
    for (size_t i = 0; i < fl; i++) {
        HM_ARG(q[i] >= -REC_MAP_QMAX && q[i] <= REC_MAP_QMAX, "hm_body_rec_trace_null: q %d (frame %zu, trace %zu) outside -%d..%d",
               (int)q[i], i / (size_t)L, i % (size_t)L, REC_MAP_QMAX, REC_MAP_QMAX);
        u1[i % (size_t)L] += q[i];
    }
    for (int k = 0; k < F; k++) q0[(size_t)k] = q[(size_t)k * L];
    for (int s = 0; s < L; s++)
        HM_ARG(vb[s] >= 0.0 && std::isfinite(vb[s]), "hm_body_rec_trace_null: vb %g (trace %d) is negative or not finite", vb[s], s);
    if (!(tmax || tmin || ge || le)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const RecBox &b = h->rec.box;
    const size_t nb = (size_t)b.pitch * b.bh;
    const bool keys = tmax || tmin;
    RecMaps g;
    RecNull a;
    int *d_q = nullptr, *d_q0 = nullptr;
    long long *d_u1 = nullptr;
    double *d_vb = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_q = cv.take<int>(fl);
        d_q0 = cv.take<int>((size_t)F);
        d_u1 = cv.take<long long>((size_t)L);
        d_vb = cv.take<double>((size_t)L);
        g.c = cv.take<unsigned long long>(nb);
        g.w1 = cv.take<unsigned long long>(nb);
        g.w2 = cv.take<unsigned long long>(nb);
        a.kmax = keys ? cv.take<unsigned long long>((size_t)L) : nullptr;
        a.kmin = keys ? cv.take<unsigned long long>((size_t)L) : nullptr;
        a.ge = ge ? cv.take<unsigned>(nb) : nullptr;
        a.le = le ? cv.take<unsigned>(nb) : nullptr;
    }));
    HM_HIP(hipMemcpyAsync(d_q, q, fl * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_q0, q0.data(), (size_t)F * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_u1, u1.data(), (size_t)L * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_vb, vb, (size_t)L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.c, 0, nb * 8, h->stream));
    HM_HIP(hipMemsetAsync(g.w1, 0, nb * 8, h->stream));
    HM_HIP(hipMemsetAsync(g.w2, 0, nb * 8, h->stream));
    if (keys) {
        HM_HIP(hipMemsetAsync(a.kmax, 0, (size_t)L * 8, h->stream));          // the lowest key
        HM_HIP(hipMemsetAsync(a.kmin, 0xff, (size_t)L * 8, h->stream));       // the highest
    }
    if (ge) HM_HIP(hipMemsetAsync(a.ge, 0, nb * sizeof(unsigned), h->stream));
    if (le) HM_HIP(hipMemsetAsync(a.le, 0, nb * sizeof(unsigned), h->stream));
    // column 0 alone through k_rec_trace_maps: c_0, w1, w2 of every pixel, which k_rec_trace_null reads at its end
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.L = 1; g.run = h->rec.map_frames; g.q = d_q0;
    hipLaunchKernelGGL(k_rec_trace_maps, dim3(hm_cdiv((int)(nb >> 2), 256), std::min(hm_cdiv(F, g.run), 65535), 1), dim3(256), 0,
                       h->stream, g);
    a.b = b; a.chunks = g.chunks; a.F = F; a.L = L; a.run = h->rec.null_frames; a.W = h->W; a.q = d_q; a.u1 = d_u1; a.vb = d_vb;
    a.tri = h->body.tri; a.c0 = g.c; a.w1 = g.w1; a.w2 = g.w2;
    const long long wgs = (long long)hm_cdiv((int)(nb >> 2), 256) * hm_cdiv(L, REC_MAP_GROUP);
    HM_ARG(wgs < (1ll << 31), "hm_body_rec_trace_null: %lld workgroups (a box of %d x %d pixels, %d traces)", wgs, b.bw, b.bh, L);
    hipLaunchKernelGGL(k_rec_trace_null, dim3((unsigned)wgs), dim3(256), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    std::vector<uint64_t> key(keys ? 2 * (size_t)L : 0);
    if (keys) {
        HM_HIP(hipMemcpyAsync(key.data(), a.kmax, (size_t)L * 8, hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipMemcpyAsync(key.data() + L, a.kmin, (size_t)L * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HM_HIP(hipStreamSynchronize(h->stream));
    // a key back to its double (d_null_key); one that no workgroup touched (a map without a pixel) is NaN
    auto unkey = [](uint64_t k) {
        const uint64_t u = (k >> 63) ? k & ~((uint64_t)1 << 63) : ~k;
        double x;
        memcpy(&x, &u, 8);
        return k == 0 || k == ~(uint64_t)0 ? std::nan("") : x;
    };
    for (int s = 0; s < L; s++) {
        if (tmax) tmax[s] = unkey(key[(size_t)s]);
        if (tmin) tmin[s] = unkey(key[(size_t)L + s]);
    }
    if (ge) HM_TRY(rec_expand_planes(h, a.ge, 1, ge));
    if (le) HM_TRY(rec_expand_planes(h, a.le, 1, le));
    return HM_OK;
}

// ---- the Gram matrix of the record's frames (gram_kernels.h) ----------------------------------------------------------
extern "C" int hm_body_rec_gram(hm_ctx_t h, int k0, int n, int stride, int64_t *G, uint64_t *s1)
{
    HM_ARG(n >= 1 && n <= REC_GRAM_MAX, "hm_body_rec_gram: %d frames outside 1..%d", n, REC_GRAM_MAX);
    HM_ARG(stride >= 1, "hm_body_rec_gram: stride %d (need >= 1)", stride);
    HM_ARG(k0 >= 0, "hm_body_rec_gram: first frame %d is negative", k0);
    HM_ARG(h != nullptr, "hm_body_rec_gram: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_gram"));
    const int F = h->rec.frames;
    const long long last = (long long)k0 + (long long)(n - 1) * stride;
    HM_ARG(last < F, "hm_body_rec_gram: %d frames from %d in steps of %d end at frame %lld of a record of %d", n, k0, stride, last, F);
    if (!(G || s1)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const RecBox &b = h->rec.box;
    const size_t nb = (size_t)b.pitch * b.bh, nn = (size_t)n * n;
    RecGram g;
    unsigned long long *d_s1 = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        g.sx = cv.take<unsigned long long>((size_t)n);
        d_s1 = cv.take<unsigned long long>(s1 ? (size_t)n : 0);
        g.G = G ? cv.take<unsigned long long>(nn) : nullptr;
    }));
    HM_HIP(hipMemsetAsync(g.sx, 0, (size_t)n * 8, h->stream));
    if (G) HM_HIP(hipMemsetAsync(g.G, 0, nn * 8, h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.k0 = k0; g.n = n; g.stride = stride; g.run = h->rec.gram_bytes;
    const int nbk = hm_cdiv(n, GRAM_BLK), pairs = G ? nbk * (nbk + 1) / 2 : nbk;
    const size_t runs = (nb + (size_t)g.run - 1) / (size_t)g.run;
    hipLaunchKernelGGL(k_rec_gram, dim3(pairs, (unsigned)std::min<size_t>(runs, 65535)), dim3(256), 0, h->stream, g);
    hipLaunchKernelGGL(k_rec_gram_fix, dim3(hm_cdiv(n, 256), std::min(n, 1024)), dim3(256), 0, h->stream, n, (long long)nb,
                       (const long long *)g.sx, (long long *)g.G, s1 ? d_s1 : nullptr);
    HM_HIP(hipGetLastError());
    if (G) HM_HIP(hipMemcpyAsync(G, g.G, nn * 8, hipMemcpyDeviceToHost, h->stream));
    if (s1) HM_HIP(hipMemcpyAsync(s1, d_s1, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// ---- the record against the deformation of its own tissue (deform_kernels.h) -----------------------------------------
// What both calls open with: T is the handle's number of triangles, the helper joined, a record with frames.
static int rec_tri_open(hm_ctx *h, const char *who, int T)
{
    HM_ARG(T == h->T, "%s: %d triangles given, the mesh has %d", who, T, h->T);
    HM_JOIN_LAZY(h);
    return body_rec_ready(h, who);
}

// queue t(p), the body map cut to the box (-1 in the padding and off the map), into d_tri
static void rec_tri_plane(hm_ctx *h, int *d_tri)
{
    const RecBox &b = h->rec.box;
    const int nb = b.pitch * b.bh;
    hipLaunchKernelGGL(k_rec_box_labels, dim3(hm_cdiv(nb, 256)), dim3(256), 0, h->stream, h->W, b, (const int *)h->body.tri,
                       (const int *)h->body.tri, d_tri);
}

extern "C" int hm_body_rec_tri_maps(hm_ctx_t h, int T, const int32_t *q, int64_t *c, uint64_t *w1, uint64_t *w2)
{
    HM_ARG(h && q, "hm_body_rec_tri_maps: NULL handle or traces");
    HM_TRY(rec_tri_open(h, "hm_body_rec_tri_maps", T));
    const int F = h->rec.frames;
    // |F c| and |w1 u1| <= F^2 x 255 x 32767
    HM_ARG((unsigned __int128)F * F * 255u * (unsigned)REC_TM_QMAX < ((unsigned __int128)1 << 63),
           "hm_body_rec_tri_maps: F x F x 255 x 32767 = %d x %d x 255 x 32767 could pass 2^63", F, F);
    const size_t ft = (size_t)F * T;
    std::vector<int16_t> q16(ft);
    for (size_t i = 0; i < ft; i++) {
        HM_ARG(q[i] >= -REC_TM_QMAX && q[i] <= REC_TM_QMAX, "hm_body_rec_tri_maps: q %d (frame %zu, triangle %zu) outside -%d..%d",
               (int)q[i], i / (size_t)T, i % (size_t)T, REC_TM_QMAX, REC_TM_QMAX);
        q16[i] = (int16_t)q[i];
    }
    if (!(c || w1 || w2)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const RecBox &b = h->rec.box;
    const size_t nb = (size_t)b.pitch * b.bh;
    RecTriMaps g;
    int *d_tri = nullptr;
    int16_t *d_q = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_tri = cv.take<int>(nb);
        d_q = cv.take<int16_t>(c ? ft : 0);
        g.c = c ? cv.take<unsigned long long>(nb) : nullptr;
        g.w1 = w1 || w2 ? cv.take<unsigned long long>(nb) : nullptr;
        g.w2 = w1 || w2 ? cv.take<unsigned long long>(nb) : nullptr;
    }));
    rec_tri_plane(h, d_tri);
    if (c) {
        HM_HIP(hipMemcpyAsync(d_q, q16.data(), ft * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
        HM_HIP(hipMemsetAsync(g.c, 0, nb * 8, h->stream));
    }
    if (g.w1) {
        HM_HIP(hipMemsetAsync(g.w1, 0, nb * 8, h->stream));
        HM_HIP(hipMemsetAsync(g.w2, 0, nb * 8, h->stream));
    }
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.T = T; g.run = h->rec.tm_frames; g.tri = d_tri; g.q = d_q;
    const dim3 grid(hm_cdiv((int)(nb >> 2), 256), std::min(hm_cdiv(F, g.run), 65535));
    if (c) hipLaunchKernelGGL(k_rec_tri_maps<1>, grid, dim3(256), 0, h->stream, g);
    else hipLaunchKernelGGL(k_rec_tri_maps<0>, grid, dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipStreamSynchronize(h->stream));
    if (c) HM_TRY(rec_expand_planes(h, g.c, 1, c));
    if (w1) HM_TRY(rec_expand_planes(h, g.w1, 1, w1));
    if (w2) HM_TRY(rec_expand_planes(h, g.w2, 1, w2));
    return HM_OK;
}

extern "C" int hm_body_rec_tri_gain(hm_ctx_t h, int T, const uint16_t *m, uint64_t *clipped)
{
    HM_ARG(h && m, "hm_body_rec_tri_gain: NULL handle or gains");
    HM_TRY(rec_tri_open(h, "hm_body_rec_tri_gain", T));
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    const size_t nb = (size_t)b.pitch * b.bh, ft = (size_t)F * T;
    RecTriGain g;
    int *d_tri = nullptr;
    uint16_t *d_m = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_tri = cv.take<int>(nb);
        d_m = cv.take<uint16_t>(ft);
        g.clipped = cv.take<unsigned long long>(1);
    }));
    rec_tri_plane(h, d_tri);
    HM_HIP(hipMemcpyAsync(d_m, m, ft * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.clipped, 0, sizeof(unsigned long long), h->stream));
    g.b = b; g.chunks = (uint8_t *const *)h->rec.tab; g.F = F; g.T = T; g.tri = d_tri; g.m = d_m;
    const int chunks = hm_cdiv(F, b.fpc), groups = hm_cdiv(std::min(F, b.fpc), REC_TG_FRAMES);
    hipLaunchKernelGGL(k_rec_tri_gain, dim3(hm_cdiv((int)(nb >> 2), 256), std::min(groups, 65535), std::min(chunks, 65535)), dim3(256), 0,
                       h->stream, g);
    HM_HIP(hipGetLastError());
    unsigned long long n = 0;
    HM_HIP(hipMemcpyAsync(&n, g.clipped, sizeof n, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    if (clipped) *clipped = n;
    return HM_OK;
}

// ---- residual motion of the record: patch sums, sums at given shifts, the shift in place, the smooth field (stab_kernels.h)
// the core of every patch on the host: core[y * pitch + x] = 1 where every box pixel within S of (x, y) is in the map `tri`
// (W values per row; two passes of prefix sums: rows, then columns); n_core: per patch
static void stab_core(const RecBox &b, const int *tri, int W, int B, int S, std::vector<uint8_t> &core, std::vector<uint32_t> &n_core)
{
    const RecGrid gr = rec_grid(b, B);
    const int n1 = 2 * S + 1;
    core.assign((size_t)b.pitch * b.bh, 0);
    n_core.assign((size_t)gr.np, 0);
    std::vector<uint8_t> hor((size_t)b.bw * b.bh, 0);
    std::vector<int> pre((size_t)std::max(b.bw, b.bh) + 1);
    for (int y = 0; y < b.bh; y++) {
        pre[0] = 0;
        for (int x = 0; x < b.bw; x++) pre[x + 1] = pre[x] + (tri[(size_t)(b.r0 + y) * W + b.c0 + x] >= 0);
        for (int x = S; x + S < b.bw; x++) hor[(size_t)y * b.bw + x] = pre[x + S + 1] - pre[x - S] == n1;
    }
    for (int x = 0; x < b.bw; x++) {
        pre[0] = 0;
        for (int y = 0; y < b.bh; y++) pre[y + 1] = pre[y] + hor[(size_t)y * b.bw + x];
        for (int y = S; y + S < b.bh; y++)
            if (pre[y + S + 1] - pre[y - S] == n1) {
                core[(size_t)y * b.pitch + x] = 1;
                n_core[(size_t)(y / B) * gr.npx + x / B]++;
            }
    }
}

extern "C" int hm_body_rec_match(hm_ctx_t h, int k0, int n_frames, int B, int S, const uint8_t *tmpl, uint32_t *n_core,
                                 uint32_t *A, uint32_t *V1, uint32_t *V2)
{
    HM_TRY(stab_patch_ok("hm_body_rec_match", B));
    HM_ARG(S >= 0 && S <= STAB_SMAX, "hm_body_rec_match: search radius %d outside 0..%d", S, STAB_SMAX);
    HM_ARG(h && tmpl, "hm_body_rec_match: NULL handle or template");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_match"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_match", k0, n_frames));
    const RecBox &b = h->rec.box;
    const RecGrid gr = rec_grid(b, B);
    const int nsh = (2 * S + 1) * (2 * S + 1);
    std::vector<uint8_t> core;
    std::vector<uint32_t> cnt;
    stab_core(b, h->body.h_tri.data(), h->W, B, S, core, cnt);
    if (n_core) memcpy(n_core, cnt.data(), (size_t)gr.np * sizeof(uint32_t));
    if (n_frames == 0 || !(A || V1 || V2)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const size_t n = (size_t)h->W * h->H, no = (size_t)n_frames * gr.np * nsh;
    StabMatch g;
    uint8_t *d_tmpl = nullptr, *d_core = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_tmpl = cv.take<uint8_t>(n);
        d_core = cv.take<uint8_t>(core.size());
        g.A = A ? cv.take<unsigned>(no) : nullptr;
        g.V1 = V1 ? cv.take<unsigned>(no) : nullptr;
        g.V2 = V2 ? cv.take<unsigned>(no) : nullptr;
    }));
    HM_HIP(hipMemcpyAsync(d_tmpl, tmpl, n, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_core, core.data(), core.size(), hipMemcpyHostToDevice, h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames; g.tpf = h->rec.tp_frames;
    g.B = B; g.S = S; g.npx = gr.npx; g.np = gr.np; g.tmpl = d_tmpl; g.core = d_core;
    const int runs = hm_cdiv(n_frames, g.tpf);
    hipLaunchKernelGGL(k_stab_match, dim3(gr.np, std::min(runs, 65535)), dim3(256), stab_lds_bytes(B, S), h->stream, g);
    HM_HIP(hipGetLastError());
    if (A) HM_HIP(hipMemcpyAsync(A, g.A, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (V1) HM_HIP(hipMemcpyAsync(V1, g.V1, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (V2) HM_HIP(hipMemcpyAsync(V2, g.V2, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// every shift of `count` (dx, dy) pairs within +-STAB_DMAX
static int stab_shifts_ok(const int8_t *shifts, size_t count, int np, const char *who)
{
    for (size_t i = 0; i < 2 * count; i++)
        HM_ARG(shifts[i] >= -STAB_DMAX && shifts[i] <= STAB_DMAX, "%s: shift %d (%s of patch %zu, frame %zu of those given) outside -%d..%d",
               who, (int)shifts[i], i & 1 ? "dy" : "dx", (i / 2) % (size_t)np, (i / 2) / (size_t)np, STAB_DMAX, STAB_DMAX);
    return HM_OK;
}

extern "C" int hm_body_rec_frame_sums(hm_ctx_t h, int k0, int n_frames, int B, const int8_t *shifts, uint32_t *out)
{
    if (shifts) HM_TRY(stab_patch_ok("hm_body_rec_frame_sums", B));
    HM_ARG((long long)n_frames * 255 < (1ll << 32), "hm_body_rec_frame_sums: %d frames x 255 could pass 2^32", n_frames);
    HM_ARG(h && out, "hm_body_rec_frame_sums: NULL handle or output");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_frame_sums"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_frame_sums", k0, n_frames));
    const RecBox &b = h->rec.box;
    StabSum g;
    g.B = shifts ? B : 1;
    const RecGrid gr = rec_grid(b, g.B);
    g.npx = gr.npx; g.np = gr.np;
    const size_t n = (size_t)h->W * h->H, ns = shifts ? (size_t)n_frames * g.np : 0;
    if (shifts) HM_TRY(stab_shifts_ok(shifts, ns, g.np, "hm_body_rec_frame_sums"));
    int8_t *d_sh = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        g.out = cv.take<unsigned>(n);
        d_sh = cv.take<int8_t>(2 * ns);
    }));
    if (ns) HM_HIP(hipMemcpyAsync(d_sh, shifts, 2 * ns, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, n * sizeof(unsigned), h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames;
    g.tri_of = h->body.tri; g.shifts = ns ? d_sh : nullptr;
    hipLaunchKernelGGL(k_stab_frame_sums, dim3(hm_cdiv(b.bw * b.bh, 256)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_shift(hm_ctx_t h, int B, const int8_t *shifts)
{
    HM_TRY(stab_patch_ok("hm_body_rec_shift", B));
    HM_ARG(h && shifts, "hm_body_rec_shift: NULL handle or shifts");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_shift"));
    const RecBox &b = h->rec.box;
    const RecGrid gr = rec_grid(b, B);
    const int F = h->rec.frames;
    StabShift g;
    g.b = b; g.W = h->W; g.B = B; g.npx = gr.npx; g.np = gr.np; g.tri_of = h->body.tri;
    const size_t ns = (size_t)F * g.np;
    HM_TRY(stab_shifts_ok(shifts, ns, g.np, "hm_body_rec_shift"));
    int8_t *d_sh = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) { d_sh = cv.take<int8_t>(2 * ns); }));
    return rec_with_scratch(h, std::min(b.fpc, F), [&](int per) -> int {
        HM_HIP(hipMemcpyAsync(d_sh, shifts, 2 * ns, hipMemcpyHostToDevice, h->stream));
        return rec_rewrite(h, per, [&](dim3 grid, const uint8_t *src, uint8_t *dst, int k, int m) {
            g.frames = m; g.shifts = d_sh + 2 * (size_t)k * g.np; g.src = src; g.dst = dst;
            hipLaunchKernelGGL(k_stab_shift, grid, dim3(256), 0, h->stream, g);
        });
    });
}

// every q of `count` (dx, dy) pairs within +-STAB_QMAX; packed with its validity for the device
static int stab_field_pack(const int16_t *q, const uint8_t *valid, size_t count, int np, const char *who, std::vector<unsigned> &qv)
{
    qv.resize(count);
    for (size_t i = 0; i < count; i++) {
        for (int c = 0; c < 2; c++)
            HM_ARG(q[2 * i + c] >= -STAB_QMAX && q[2 * i + c] <= STAB_QMAX,
                   "%s: q %d (%s of patch %zu, frame %zu of those given) outside -%d..%d", who, (int)q[2 * i + c], c ? "dy" : "dx",
                   i % (size_t)np, i / (size_t)np, STAB_QMAX, STAB_QMAX);
        qv[i] = stab_pack(q[2 * i], q[2 * i + 1], valid[i]);
    }
    return HM_OK;
}

extern "C" int hm_body_rec_field_sums(hm_ctx_t h, int k0, int n_frames, int B, const int16_t *q, const uint8_t *valid, uint32_t *out)
{
    HM_TRY(stab_patch_ok("hm_body_rec_field_sums", B));
    HM_ARG((long long)n_frames * 255 < (1ll << 32), "hm_body_rec_field_sums: %d frames x 255 could pass 2^32", n_frames);
    HM_ARG(h && q && valid && out, "hm_body_rec_field_sums: NULL handle, q, valid or output");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_field_sums"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_field_sums", k0, n_frames));
    const RecBox &b = h->rec.box;
    const RecGrid gr = rec_grid(b, B);
    StabFieldSum g;
    g.B = B; g.npx = gr.npx; g.npy = gr.npy; g.np = gr.np;
    const size_t n = (size_t)h->W * h->H, ns = (size_t)n_frames * g.np;
    std::vector<unsigned> qv;
    HM_TRY(stab_field_pack(q, valid, ns, g.np, "hm_body_rec_field_sums", qv));
    unsigned *d_qv = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        g.out = cv.take<unsigned>(n);
        d_qv = cv.take<unsigned>(ns);
    }));
    if (ns) HM_HIP(hipMemcpyAsync(d_qv, qv.data(), ns * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, n * sizeof(unsigned), h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames;
    g.tri_of = h->body.tri; g.qv = d_qv;
    hipLaunchKernelGGL(k_stab_field_sums, dim3(hm_cdiv(b.bw * b.bh, 256)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_warp(hm_ctx_t h, int B, const int16_t *q, const uint8_t *valid)
{
    HM_TRY(stab_patch_ok("hm_body_rec_warp", B));
    HM_ARG(h && q && valid, "hm_body_rec_warp: NULL handle, q or valid");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_warp"));
    const RecBox &b = h->rec.box;
    const RecGrid gr = rec_grid(b, B);
    const int F = h->rec.frames;
    StabWarp g;
    g.b = b; g.W = h->W; g.B = B; g.npx = gr.npx; g.npy = gr.npy; g.np = gr.np; g.tri_of = h->body.tri;
    const size_t ns = (size_t)F * g.np;
    std::vector<unsigned> qv;
    HM_TRY(stab_field_pack(q, valid, ns, g.np, "hm_body_rec_warp", qv));
    unsigned *d_qv = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) { d_qv = cv.take<unsigned>(ns); }));
    return rec_with_scratch(h, std::min(b.fpc, F), [&](int per) -> int {
        HM_HIP(hipMemcpyAsync(d_qv, qv.data(), ns * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
        return rec_rewrite(h, per, [&](dim3 grid, const uint8_t *src, uint8_t *dst, int k, int m) {
            g.frames = m; g.qv = d_qv + (size_t)k * g.np; g.src = src; g.dst = dst;
            hipLaunchKernelGGL(k_stab_warp, grid, dim3(256), 0, h->stream, g);
        });
    });
}

// ---- the running baseline per pixel of the record: baseline, excess and dF/F planes (detrend_kernels.h) -------------
static int det_args_ok(const char *who, int what, int half, int q, int floor, int gain)
{
    HM_ARG(what >= 0 && what <= 3, "%s: kind of plane %d outside 0..3 (0 as recorded, 1 baseline, 2 excess, 3 dF/F byte)", who, what);
    HM_ARG(half >= 0 && half <= DET_HALF_MAX, "%s: half %d outside 0..%d", who, half, DET_HALF_MAX);
    HM_ARG(q >= 0 && q <= 100, "%s: q %d outside 0..100", who, q);
    HM_ARG(floor >= 1 && floor <= 255, "%s: floor %d outside 1..255", who, floor);
    HM_ARG(gain >= 1 && gain <= 65535, "%s: gain %d outside 1..65535", who, gain);
    return HM_OK;
}

// the kind of plane and the baseline's parameters, as the two calls take them
struct DetPlanes { int what, half, q, floor, gain; };

// queue planes d.what (1..3) of the frames k .. k + m - 1 into dst (m frames in the record's layout)
// -- of the segments seg0 .. seg0 + nseg - 1 of the box frame alone if nseg > 0 (the rest of dst is left as it is)
static int det_queue(hm_ctx *h, const DetPlanes &d, int k, int m, uint8_t *dst, int seg0 = 0, int nseg = 0)
{
    RecRunning g;
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = h->rec.frames; g.k0 = k; g.n = m;
    g.run = h->rec.bl_frames; g.what = d.what; g.half = d.half; g.q = d.q; g.floor = d.floor; g.gain = d.gain; g.out = dst;
    g.seg0 = seg0;
    const int segs = nseg > 0 ? nseg : hm_cdiv(g.b.pitch * g.b.bh, 64), runs = hm_cdiv(m, g.run);
    hipLaunchKernelGGL(k_rec_running, dim3(segs, std::min(runs, 65535)), dim3(64), DET_LDS_BYTES, h->stream, g);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_body_rec_planes(hm_ctx_t h, int k0, int n_frames, int what, int half, int q, int floor, int gain, uint8_t *out)
{
    HM_TRY(det_args_ok("hm_body_rec_planes", what, half, q, floor, gain));
    HM_ARG(h != nullptr, "hm_body_rec_planes: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_planes"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_planes", k0, n_frames));
    HM_ARG(out || n_frames == 0, "hm_body_rec_planes: NULL output");
    const size_t px = (size_t)h->W * h->H;
    if (what == 0) {
        HM_HIP(hipStreamSynchronize(h->stream));
        for (int k = 0; k < n_frames; k++) HM_TRY(rec_expand(h, rec_frame(h, k0 + k), out + (size_t)k * px));
        return HM_OK;
    }
    const DetPlanes d = {what, half, q, floor, gain};
    return rec_with_scratch(h, n_frames, [&](int per) -> int {
        HM_TRY(rec_runs(h, per, k0, n_frames, true, [&](int k, int m, uint8_t *dst) { return det_queue(h, d, k, m, dst); },
                        [&](int j, const uint8_t *src) { return rec_expand(h, src, out + (size_t)j * px); }));
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    });
}

extern "C" int hm_body_rec_stats_add(hm_ctx_t h, int what, int half, int q, int floor, int gain)
{
    HM_TRY(det_args_ok("hm_body_rec_stats_add", what, half, q, floor, gain));
    HM_ARG(h != nullptr, "hm_body_rec_stats_add: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_stats_add"));
    HM_TRY(rec_stats_open(h, "hm_body_rec_stats_add"));
    const int F = h->rec.frames;
    if (what == 0) {
        for (int k = 0; k < F; k++) HM_TRY(rec_stats_add_plane(h, rec_frame(h, k)));
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const DetPlanes d = {what, half, q, floor, gain};
    return rec_with_scratch(h, F, [&](int per) -> int {
        // (a run's planes are queued behind the adds that read the scratch)
        HM_TRY(rec_runs(h, per, 0, F, false, [&](int k, int m, uint8_t *dst) { return det_queue(h, d, k, m, dst); },
                        [&](int, const uint8_t *src) { return rec_stats_add_plane(h, src); }));
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    });
}

// ---- events per pixel of the record: AR(1) deconvolution of every pixel's planes of a kind (events_kernels.h) ---------
struct EvParams { DetPlanes d; double g, lam, s_min; };

static int ev_args_ok(const char *who, double g, double lam, double s_min)
{
    HM_ARG(std::isfinite(g) && g > 0.0 && g < 1.0, "%s: g %g outside 0 < g < 1", who, g);
    HM_ARG(std::isfinite(lam) && lam >= 0.0, "%s: lam %g negative or not finite", who, lam);
    HM_ARG(std::isfinite(s_min) && s_min >= 0.0, "%s: s_min %g negative or not finite", who, s_min);
    return HM_OK;
}

// The pool stacks of every box pixel over all F frames, in passes over as many segments as rec.ev_bytes hold (one at
// least), then done(E, cnt, sum): E the event bytes of the frames k0 .. k0 + n - 1 in the record's layout (NULL if n is 0),
// cnt and sum per byte of a box frame (NULL unless want_sums), all on the device and complete.  A pass pushes the planes of
// kind d.what batch by batch -- the scratch of hm_body_rec_planes, filled for the pass's segments alone -- or the record
// itself for kind 0, then reads its pools out.  The stack, E and the scratch are freed on every return.
template <typename Done>
static int ev_call(hm_ctx *h, const char *who, const EvParams &p, int k0, int n, bool want_sums, Done done)
{
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    HM_ARG(F <= EV_FMAX, "%s: a record of %d frames (the pool stack holds frame numbers in 16 bits: %d frames at most)", who, F, EV_FMAX);
    const int segs = hm_cdiv(b.pitch * b.bh, 64);
    const size_t seg_bytes = (size_t)EV_PX_BYTES * 64 * F;
    const int per_pass = (int)std::max<size_t>(1, std::min<size_t>((size_t)segs, h->rec.ev_bytes / seg_bytes));
    std::vector<double> pw(2 * ((size_t)F + 1));
    double *pw2 = pw.data() + F + 1;
    pw[0] = 1.0;
    for (int l = 1; l <= F; l++) pw[l] = pw[l - 1] * p.g;
    for (int l = 0; l <= F; l++) pw2[l] = pw[l] * pw[l];
    double *d_pw = nullptr, *d_sum = nullptr;
    unsigned *d_cnt = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_pw = cv.take<double>(pw.size());
        if (want_sums) {
            d_cnt = cv.take<unsigned>((size_t)segs * 64);
            d_sum = cv.take<double>((size_t)segs * 64);
        }
    }));
    RecEvents e;
    e.b = b; e.chunks = (const uint8_t *const *)h->rec.tab; e.src = nullptr; e.ks = 0; e.F = F;
    e.g = p.g; e.mu = p.lam * (1.0 - p.g); e.lam = p.lam; e.pw = d_pw; e.pw2 = d_pw + F + 1;
    auto passes = [&](int per) -> int {
        for (int s0 = 0; s0 < segs; s0 += per_pass) {
            const int ns = std::min(per_pass, segs - s0);
            const size_t FP = (size_t)F * ns * 64;
            e.seg0 = s0; e.nseg = ns;
            e.v = (double *)h->rec.ev; e.w = e.v + FP; e.len = (uint16_t *)(e.w + FP); e.start = e.len + FP;
            if (p.d.what == 0) hipLaunchKernelGGL(k_rec_ev_push, dim3(ns), dim3(64), 0, h->stream, e, 0, F);
            else
                for (int k = 0; k < F; k += per) {          // (a batch's planes are queued behind the push that read the scratch)
                    const int m = std::min(per, F - k);
                    HM_TRY(det_queue(h, p.d, k, m, h->rec.scr, s0, ns));
                    e.src = h->rec.scr; e.ks = k;
                    hipLaunchKernelGGL(k_rec_ev_push, dim3(ns), dim3(64), 0, h->stream, e, k, m);
                }
            hipLaunchKernelGGL(k_rec_ev_read, dim3(ns), dim3(64), 0, h->stream, e, k0, n, h->rec.ev_out, p.s_min, d_cnt, d_sum);
            HM_HIP(hipGetLastError());
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    };
    const int rc = [&]() -> int {
        HM_HIP(h->own.grow(&h->rec.ev, (size_t)per_pass * seg_bytes));
        if (n > 0) {
            HM_HIP(h->own.grow(&h->rec.ev_out, (size_t)n * b.fs));
            HM_HIP(hipMemsetAsync(h->rec.ev_out, 0, (size_t)n * b.fs, h->stream));
        }
        HM_HIP(hipMemcpyAsync(d_pw, pw.data(), pw.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HM_TRY(p.d.what == 0 ? passes(0) : rec_with_scratch(h, F, passes));
        return done((const uint8_t *)h->rec.ev_out, (const unsigned *)d_cnt, (const double *)d_sum);
    }();
    if (rc) (void)hipStreamSynchronize(h->stream);
    const hipError_t fe = h->own.free(&h->rec.ev), fo = h->own.free(&h->rec.ev_out);
    if (rc) return rc;
    HM_HIP(fe);
    HM_HIP(fo);
    return HM_OK;
}

extern "C" int hm_body_rec_event_planes(hm_ctx_t h, int k0, int n_frames, int what, int half, int q, int floor, int gain, double g,
                                        double lam, uint8_t *out)
{
    HM_TRY(det_args_ok("hm_body_rec_event_planes", what, half, q, floor, gain));
    HM_TRY(ev_args_ok("hm_body_rec_event_planes", g, lam, 0.0));
    HM_ARG(h != nullptr, "hm_body_rec_event_planes: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_event_planes"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_event_planes", k0, n_frames));
    HM_ARG(out || n_frames == 0, "hm_body_rec_event_planes: NULL output");
    const size_t px = (size_t)h->W * h->H;
    const EvParams p = {{what, half, q, floor, gain}, g, lam, 0.0};
    return ev_call(h, "hm_body_rec_event_planes", p, k0, n_frames, false, [&](const uint8_t *E, const unsigned *, const double *) -> int {
        for (int k = 0; k < n_frames; k++) HM_TRY(rec_expand(h, E + (size_t)k * h->rec.box.fs, out + (size_t)k * px));
        return HM_OK;
    });
}

extern "C" int hm_body_rec_event_stats_add(hm_ctx_t h, int what, int half, int q, int floor, int gain, double g, double lam)
{
    HM_TRY(det_args_ok("hm_body_rec_event_stats_add", what, half, q, floor, gain));
    HM_TRY(ev_args_ok("hm_body_rec_event_stats_add", g, lam, 0.0));
    HM_ARG(h != nullptr, "hm_body_rec_event_stats_add: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_event_stats_add"));
    HM_TRY(rec_stats_open(h, "hm_body_rec_event_stats_add"));
    const int F = h->rec.frames;
    const EvParams p = {{what, half, q, floor, gain}, g, lam, 0.0};
    return ev_call(h, "hm_body_rec_event_stats_add", p, 0, F, false, [&](const uint8_t *E, const unsigned *, const double *) -> int {
        for (int k = 0; k < F; k++) HM_TRY(rec_stats_add_plane(h, E + (size_t)k * h->rec.box.fs));
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    });
}

extern "C" int hm_body_rec_event_sums(hm_ctx_t h, int what, int half, int q, int floor, int gain, double g, double lam, double s_min,
                                      uint32_t *count, double *sum)
{
    HM_TRY(det_args_ok("hm_body_rec_event_sums", what, half, q, floor, gain));
    HM_TRY(ev_args_ok("hm_body_rec_event_sums", g, lam, s_min));
    HM_ARG(h != nullptr, "hm_body_rec_event_sums: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_event_sums"));
    const EvParams p = {{what, half, q, floor, gain}, g, lam, s_min};
    return ev_call(h, "hm_body_rec_event_sums", p, 0, 0, true, [&](const uint8_t *, const unsigned *d_cnt, const double *d_sum) -> int {
        const RecBox &b = h->rec.box;
        const size_t nb = (size_t)b.pitch * b.bh, px = (size_t)h->W * h->H;
        std::vector<unsigned> cnt(nb);
        std::vector<double> sm(nb);
        HM_HIP(hipMemcpy(cnt.data(), d_cnt, nb * sizeof(unsigned), hipMemcpyDeviceToHost));
        HM_HIP(hipMemcpy(sm.data(), d_sum, nb * sizeof(double), hipMemcpyDeviceToHost));
        if (count) std::fill(count, count + px, 0u);
        if (sum) std::fill(sum, sum + px, 0.0);
        for (int yb = 0; yb < b.bh; yb++)
            for (int x = 0; x < b.bw; x++) {
                const size_t o = (size_t)(b.r0 + yb) * h->W + b.c0 + x, i = (size_t)yb * b.pitch + x;
                if (count) count[o] = cnt[i];
                if (sum) sum[o] = sm[i];
            }
        return HM_OK;
    });
}

// ---- the residual of the record: what the cells' model leaves of every frame (residual_kernels.h) --------------------
static int res_args_ok(const char *who, int n_layers, const int32_t *labels, int L, const int32_t *traces, int offset)
{
    HM_ARG(n_layers >= 1 && n_layers <= 4, "%s: %d layers outside 1..4", who, n_layers);
    HM_ARG(L >= 1 && L <= REC_RES_LMAX, "%s: %d labels outside 1..%d", who, L, REC_RES_LMAX);
    HM_ARG(offset >= 0 && offset <= 255, "%s: offset %d outside 0..255", who, offset);
    HM_ARG(labels && traces, "%s: NULL labels or traces", who);
    return HM_OK;
}

// The cells of the box as k_rec_residual reads them, from the caller's planes: per layer and box pixel the label and its
// weight in one dword (lay), the pixels that count (live: in the map `tri` and not under a blank) and the layers a segment
// of 256 pixels needs (seg_nl).  Off the map and under a blank nothing is packed: a segment of such pixels alone costs
// no layer.  The labels are within -1 .. L - 1 (hm_labels_ok).
static void res_pack_host(const RecBox &b, const int *tri, int W, int H, int n_layers, const int32_t *labels, const uint16_t *weights,
                          const uint8_t *blank, std::vector<unsigned> &lay, std::vector<uint8_t> &live, std::vector<uint8_t> &seg_nl)
{
    const size_t n = (size_t)W * H, npx = (size_t)b.pitch * b.bh;
    lay.assign((size_t)n_layers * npx, 0u);
    live.assign(npx, 0);
    seg_nl.assign(hm_cdiv((int)(npx >> 2), 64), 0);
    for (int yb = 0; yb < b.bh; yb++)
        for (int x = 0; x < b.bw; x++) {
            const size_t p = (size_t)(b.r0 + yb) * W + b.c0 + x, i = (size_t)yb * b.pitch + x;
            if (tri[p] < 0 || (blank && blank[p])) continue;
            live[i] = 1;
            for (int j = 0; j < n_layers; j++) {
                const int s = labels[(size_t)j * n + p];
                if (s < 0) continue;
                lay[(size_t)j * npx + i] = ((unsigned)s << 16) | (weights ? (unsigned)weights[(size_t)j * n + p] : 65535u);
                uint8_t &top = seg_nl[i >> 8];
                top = std::max<uint8_t>(top, (uint8_t)(j + 1));
            }
        }
}

// The cells of the box, packed for k_rec_residual and sent to the device with the traces; a label outside -1 .. L - 1
// anywhere in the planes is refused here.
static int res_pack(hm_ctx *h, const char *who, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                    const int32_t *traces, const uint8_t *blank, int offset, bool want_clipped, RecResidual &g)
{
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    HM_ARG((long long)F * L < (1ll << 30), "%s: %d frames x %d labels", who, F, L);
    HM_TRY(hm_labels_ok(who, n_layers, labels, (size_t)h->W * h->H, L));
    std::vector<unsigned> lay;
    std::vector<uint8_t> live, seg_nl;
    res_pack_host(b, h->body.h_tri.data(), h->W, h->H, n_layers, labels, weights, blank, lay, live, seg_nl);
    unsigned *d_lay = nullptr, *d_live = nullptr;
    uint8_t *d_seg = nullptr;
    int *d_tr = nullptr;
    unsigned long long *d_clip = nullptr;
    HM_TRY(body_rec_carve(h, [&](RecCarve &cv) {
        d_lay = cv.take<unsigned>(lay.size());
        d_live = cv.take<unsigned>(live.size() >> 2);
        d_seg = cv.take<uint8_t>(seg_nl.size());
        d_tr = cv.take<int>((size_t)F * L);
        d_clip = cv.take<unsigned long long>(1);
    }));
    // (pageable sources: each copy has left the host array when the call returns)
    HM_HIP(hipMemcpyAsync(d_lay, lay.data(), lay.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_live, live.data(), live.size(), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_seg, seg_nl.data(), seg_nl.size(), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_tr, traces, (size_t)F * L * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(d_clip, 0, sizeof(unsigned long long), h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.run = h->rec.res_frames; g.nl = n_layers; g.L = L; g.offset = offset;
    g.lay = d_lay; g.live = d_live; g.seg_nl = d_seg; g.traces = d_tr; g.clipped = want_clipped ? d_clip : nullptr;
    return HM_OK;
}

// queue the residual planes of the frames k .. k + m - 1 into dst (m frames in the record's layout)
static int res_queue(hm_ctx *h, RecResidual g, int k, int m, uint8_t *dst)
{
    g.k0 = k; g.n = m; g.out = dst;
    const int segs = hm_cdiv((g.b.pitch * g.b.bh) >> 2, 64), runs = hm_cdiv(m, g.run);
    hipLaunchKernelGGL(k_rec_residual, dim3(segs, std::min(runs, 65535)), dim3(64), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

static int res_clipped(hm_ctx *h, const RecResidual &g, uint64_t *clipped)
{
    if (!clipped) return HM_OK;
    unsigned long long c = 0;
    HM_HIP(hipMemcpyAsync(&c, g.clipped, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    *clipped = c;
    return HM_OK;
}

extern "C" int hm_body_rec_residual_planes(hm_ctx_t h, int k0, int n_frames, int n_layers, const int32_t *labels,
                                           const uint16_t *weights, int L, const int32_t *traces, const uint8_t *blank,
                                           int offset, uint8_t *out, uint64_t *clipped)
{
    HM_TRY(res_args_ok("hm_body_rec_residual_planes", n_layers, labels, L, traces, offset));
    HM_ARG(h != nullptr, "hm_body_rec_residual_planes: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_residual_planes"));
    HM_TRY(rec_range_ok(h, "hm_body_rec_residual_planes", k0, n_frames));
    HM_ARG(out || n_frames == 0, "hm_body_rec_residual_planes: NULL output");
    RecResidual g;
    HM_TRY(res_pack(h, "hm_body_rec_residual_planes", n_layers, labels, weights, L, traces, blank, offset, clipped != nullptr, g));
    const size_t px = (size_t)h->W * h->H;
    return rec_with_scratch(h, n_frames, [&](int per) -> int {
        HM_TRY(rec_runs(h, per, k0, n_frames, true, [&](int k, int m, uint8_t *dst) { return res_queue(h, g, k, m, dst); },
                        [&](int j, const uint8_t *src) { return rec_expand(h, src, out + (size_t)j * px); }));
        return res_clipped(h, g, clipped);
    });
}

extern "C" int hm_body_rec_residual_stats_add(hm_ctx_t h, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                                              const int32_t *traces, const uint8_t *blank, int offset, uint64_t *clipped)
{
    HM_TRY(res_args_ok("hm_body_rec_residual_stats_add", n_layers, labels, L, traces, offset));
    HM_ARG(h != nullptr, "hm_body_rec_residual_stats_add: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, "hm_body_rec_residual_stats_add"));
    HM_TRY(rec_stats_open(h, "hm_body_rec_residual_stats_add"));
    RecResidual g;
    HM_TRY(res_pack(h, "hm_body_rec_residual_stats_add", n_layers, labels, weights, L, traces, blank, offset, clipped != nullptr, g));
    const int F = h->rec.frames;
    return rec_with_scratch(h, F, [&](int per) -> int {
        // (a run's planes are queued behind the adds that read the scratch)
        HM_TRY(rec_runs(h, per, 0, F, false, [&](int k, int m, uint8_t *dst) { return res_queue(h, g, k, m, dst); },
                        [&](int, const uint8_t *src) { return rec_stats_add_plane(h, src); }));
        HM_HIP(hipStreamSynchronize(h->stream));
        return res_clipped(h, g, clipped);
    });
}

// ---- activity waves: latency maps per event, their sums over the events, the local fits' sums (waves_kernels.h) --------
static int wv_step_ok(const char *who, int step)
{
    HM_ARG(step >= 1 && step <= REC_WV_STEP_MAX, "%s: node step %d outside 1..%d", who, step, REC_WV_STEP_MAX);
    return HM_OK;
}

extern "C" int hm_body_rec_wave_nodes(hm_ctx_t h, int step, int *nx, int *ny, int *c0, int *r0)
{
    HM_TRY(wv_step_ok("hm_body_rec_wave_nodes", step));
    HM_ARG(h != nullptr, "hm_body_rec_wave_nodes: NULL handle");
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_begun(h, "hm_body_rec_wave_nodes"));
    const RecBox &b = h->rec.box;
    if (nx) *nx = hm_cdiv(b.bw, step);
    if (ny) *ny = hm_cdiv(b.bh, step);
    if (c0) *c0 = b.c0;
    if (r0) *r0 = b.r0;
    return HM_OK;
}

// a plane of the box on the device -> a full W x H plane of the caller's, `fill` outside the box
template <typename T>
static int wv_expand(const hm_ctx *h, const T *d_src, T fill, T *out)
{
    const RecBox &b = h->rec.box;
    const size_t es = sizeof(T);
    std::fill(out, out + (size_t)h->W * h->H, fill);
    HM_HIP(hipMemcpy2D(out + (size_t)b.r0 * h->W + b.c0, (size_t)h->W * es, d_src, (size_t)b.pitch * es, (size_t)b.bw * es, (size_t)b.bh,
                       hipMemcpyDeviceToHost));
    return HM_OK;
}

extern "C" int hm_body_rec_waves(hm_ctx_t h, int E, const int32_t *triggers, int what, int half, int q, int floor, int gain, int bin,
                                 int pre, int lead, int post, int min_rise, int step, int Rf, uint16_t *n_bin, int32_t *lat,
                                 int32_t *rise, uint8_t *why, uint32_t *cnt, int64_t *sum_lat, int64_t *sum_lat2, int64_t *fit)
{
    const char *who = "hm_body_rec_waves";
    HM_TRY(det_args_ok(who, what, half, q, floor, gain));
    HM_ARG(E >= 1 && E <= REC_WV_EMAX, "%s: %d events outside 1..%d", who, E, REC_WV_EMAX);
    HM_ARG(triggers != nullptr, "%s: NULL triggers", who);
    HM_ARG(bin >= 0 && bin <= REC_WV_BMAX, "%s: bin radius %d outside 0..%d", who, bin, REC_WV_BMAX);
    HM_ARG(pre >= 1 && pre <= REC_WV_PRE_MAX, "%s: pre %d outside 1..%d", who, pre, REC_WV_PRE_MAX);
    HM_ARG(lead >= 0 && lead <= REC_WV_LEAD_MAX, "%s: lead %d outside 0..%d", who, lead, REC_WV_LEAD_MAX);
    HM_ARG(post >= 1 && post <= REC_WV_POST_MAX, "%s: post %d outside 1..%d", who, post, REC_WV_POST_MAX);
    HM_ARG(min_rise >= 1 && min_rise <= 255, "%s: min_rise %d outside 1..255", who, min_rise);
    HM_TRY(wv_step_ok(who, step));
    HM_ARG(Rf >= 1 && Rf <= REC_WV_RF_MAX, "%s: fit radius %d outside 1..%d", who, Rf, REC_WV_RF_MAX);
    HM_ARG(h != nullptr, "%s: NULL handle", who);
    HM_JOIN_LAZY(h);
    HM_TRY(body_rec_ready(h, who));
    const int F = h->rec.frames;
    for (int e = 0; e < E; e++) {
        const long long t = triggers[e];
        HM_ARG(t - lead - pre >= 0 && t + post <= F - 1, "%s: event %d: trigger %lld needs the frames %lld .. %lld (pre %d, lead %d, "
               "post %d) of a record of F = %d frames", who, e, t, t - lead - pre, t + post, pre, lead, post, F);
    }
    const bool want_sums = cnt || sum_lat || sum_lat2, want_lat = lat || rise || why || want_sums || fit;
    if (!(n_bin || want_lat)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const RecBox &b = h->rec.box;
    const size_t nb = (size_t)b.pitch * b.bh, px = (size_t)h->W * h->H;
    const int nx = hm_cdiv(b.bw, step), ny = hm_cdiv(b.bh, step), nodes = nx * ny, frames = pre + lead + post + 1;
    // the events of a launch: rec.wv_frames at most, and no more than keep their planes and the fit's sums below 1 GiB (one at least)
    const size_t per_event = 9 * nb + (fit ? (size_t)nodes * 9 * sizeof(long long) : 0);
    const int per = !want_lat ? 0 : (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(E, h->rec.wv_frames), ((size_t)1 << 30) / per_event));
    RecWaves g;
    uint8_t *d_mask = nullptr, *d_planes = nullptr;
    uint16_t *d_nbin = nullptr;
    int *d_trig = nullptr;
    unsigned *d_cnt = nullptr;
    long long *d_s1 = nullptr, *d_s2 = nullptr, *d_fit = nullptr;
    auto lay = [&](RecCarve &cv) {
        d_mask = cv.take<uint8_t>(nb);
        d_nbin = cv.take<uint16_t>(nb);
        d_trig = cv.take<int>((size_t)per);
        g.lat = cv.take<int>((size_t)per * nb);
        g.rise = cv.take<int>((size_t)per * nb);
        g.why = cv.take<uint8_t>((size_t)per * nb);
        d_cnt = cv.take<unsigned>(want_sums ? nb : 0);
        d_s1 = cv.take<long long>(want_sums ? nb : 0);
        d_s2 = cv.take<long long>(want_sums ? nb : 0);
        d_fit = cv.take<long long>(fit ? (size_t)per * nodes * 9 : 0);
        d_planes = cv.take<uint8_t>(what != 0 && want_lat ? (size_t)frames * b.fs : 0);
    };
    const DetPlanes d = {what, half, q, floor, gain};
    const int rc = [&]() -> int {
        RecCarve cv = {nullptr, 0};
        lay(cv);
        HM_HIP(h->own.grow(&h->rec.wv, cv.off));
        cv = {h->rec.wv, 0};
        lay(cv);
        hipLaunchKernelGGL(k_rec_wv_mask, dim3(hm_cdiv((int)nb, 256)), dim3(256), 0, h->stream, h->W, b, (const int *)h->body.tri, d_mask);
        hipLaunchKernelGGL(k_rec_wv_nbin, dim3(hm_cdiv((int)nb, 256)), dim3(256), 0, h->stream, b, bin, (const uint8_t *)d_mask, d_nbin);
        HM_HIP(hipGetLastError());
        if (want_sums) {
            HM_HIP(hipMemsetAsync(d_cnt, 0, nb * sizeof(unsigned), h->stream));
            HM_HIP(hipMemsetAsync(d_s1, 0, nb * 8, h->stream));
            HM_HIP(hipMemsetAsync(d_s2, 0, nb * 8, h->stream));
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        if (n_bin) HM_TRY(wv_expand<uint16_t>(h, d_nbin, 0, n_bin));
        g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.src = nullptr; g.ks = 0;
        g.bin = bin; g.pre = pre; g.lead = lead; g.post = post; g.min_rise = min_rise; g.trig = d_trig; g.mask = d_mask; g.nbin = d_nbin;
        const int tiles = hm_cdiv(b.bw, WV_TW) * hm_cdiv(b.bh, WV_TH);
        for (int e0 = 0; want_lat && e0 < E;) {
            // the launch's events: as many as `per`; of kinds 1..3, as long as their windows together span no more frames than one
            // window's planes take (events of one trigger, then)
            int m = 1, lo = triggers[e0] - lead - pre, hi = triggers[e0] + post;
            for (; e0 + m < E && m < per; m++) {
                const int l1 = std::min(lo, triggers[e0 + m] - lead - pre), h1 = std::max(hi, triggers[e0 + m] + post);
                if (what != 0 && h1 - l1 + 1 > frames) break;
                lo = l1; hi = h1;
            }
            HM_HIP(hipMemcpyAsync(d_trig, triggers + e0, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
            if (what != 0) {
                HM_TRY(det_queue(h, d, lo, hi - lo + 1, d_planes));
                g.src = d_planes; g.ks = lo;
            }
            hipLaunchKernelGGL(k_rec_wv_lat, dim3(tiles, m), dim3(256), 0, h->stream, g);
            if (want_sums)
                hipLaunchKernelGGL(k_rec_wv_sums, dim3(hm_cdiv((int)nb, 256)), dim3(256), 0, h->stream, b, m, (const int *)g.lat, d_cnt,
                                   d_s1, d_s2);
            if (fit)
                hipLaunchKernelGGL(k_rec_wv_fit, dim3(nodes, m), dim3(64), 0, h->stream, b, step, Rf, nx, (const int *)g.lat, d_fit);
            HM_HIP(hipGetLastError());
            HM_HIP(hipStreamSynchronize(h->stream));
            for (int e = 0; e < m; e++) {
                if (lat) HM_TRY(wv_expand<int32_t>(h, g.lat + (size_t)e * nb, REC_WV_NONE, lat + (size_t)(e0 + e) * px));
                if (rise) HM_TRY(wv_expand<int32_t>(h, g.rise + (size_t)e * nb, 0, rise + (size_t)(e0 + e) * px));
                if (why) HM_TRY(wv_expand<uint8_t>(h, g.why + (size_t)e * nb, 255, why + (size_t)(e0 + e) * px));
            }
            if (fit) HM_HIP(hipMemcpy(fit + (size_t)e0 * nodes * 9, d_fit, (size_t)m * nodes * 9 * 8, hipMemcpyDeviceToHost));
            e0 += m;
        }
        if (cnt) HM_TRY(rec_expand_planes(h, d_cnt, 1, cnt));
        if (sum_lat) HM_TRY(rec_expand_planes(h, d_s1, 1, sum_lat));
        if (sum_lat2) HM_TRY(rec_expand_planes(h, d_s2, 1, sum_lat2));
        return HM_OK;
    }();
    if (rc) (void)hipStreamSynchronize(h->stream);
    const hipError_t fe = h->own.free(&h->rec.wv);
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}
