// 16-bit input (hm_deep_*, include/hydra_mi.h): host orchestration and C-ABI; the kernels are in
// deep_kernels.h, which this translation unit alone compiles.
// One handle owns the device copy of a run's 16-bit pixels, the table, the 64-bit histogram, the clip words and two
// page-locked staging blocks used in turn.  hm_deep_hist_add and hm_deep_map work on a stream of the handle's and return
// when they are done; hm_deep_map_run_dev queues on the caller's stream and returns.
// Full-depth traces (hm_deep_body_*; kernels in deeptrace_kernels.h, which this translation unit alone
// compiles too): the same handle owns the columns, a second device copy of a run, the runs' states, sums and planes, an
// upload stream and the events between it and `stream`; of the filter handle it borrows the body map (BodyMapView).
#include "hm_common.h"
#include "deep_kernels.h"
#include "deeptrace_kernels.h"
#include <algorithm>
#include <cstring>

#define DEEP_VALUES 65536

struct hm_deep {
    int device = 0, W = 0, H = 0, max_run = 1;
    size_t n = 0;                                // pixels of a frame
    HmOwner own{1};
    bool ready = false, have_lut = false;
    int lo = 0, hi = 0;
    std::vector<uint8_t> lut;                    // as given to hm_deep_set_lut; uploaded by the first call that needs it
    bool lut_sent = false;
    uint16_t *d_in = nullptr;                    // max_run frames
    uint8_t *d_lut = nullptr;
    unsigned *d_clip = nullptr;                  // 2 words per frame of a run
    unsigned long long *d_hist = nullptr;
    uint64_t samples = 0;
    struct Stage {                               // page-locked; two, used in turn, so that a run never writes what the copy
        uint16_t *px = nullptr;                  // of the run before may still read
        hipEvent_t copied = nullptr;
        bool used = false;
    } stage[2];
    int turn = 0;
    uint64_t last_h2d = 0, total_h2d = 0;
    // hm_deep_hist_add's and hm_deep_map's own
    hipStream_t stream = nullptr;
    uint8_t *d_out = nullptr;
    // hm_deep_body_*: the columns as set (col_ptr stays on the host: the pieces are cut from it) ...
    int C = 0;
    std::vector<int64_t> col_ptr;
    int *d_pix = nullptr;
    uint16_t *d_wt = nullptr;
    DeepPiece *d_pieces = nullptr;               // ... cut for pieces_E entries a wave (0: to be cut)
    int npieces = 0, pieces_E = 0;
    bool any_split = false;
    // ... and a run's second device copy (runs alternate between d_in and d_in2, so that the upload of one is free to go
    // beside the kernels of the other), states (page-locked and on the device), sums and planes
    uint16_t *d_in2 = nullptr, *d_planes = nullptr;
    double *d_X[2] = {nullptr, nullptr}, *h_X[2] = {nullptr, nullptr};
    unsigned long long *d_sums = nullptr;
    hipStream_t up_stream = nullptr;             // the uploads; the kernels and the downloads are on `stream`
    hipEvent_t uploaded[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
};

extern "C" int hm_deep_create(int device, int W, int H, int max_run, hm_deep_t *out)
{
    HM_ARG(out, "hm_deep_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "hm_deep_create: frame size %dx%d outside 1..32767", W, H);
    HM_ARG(max_run >= 1 && max_run <= 64, "hm_deep_create: max_run %d outside 1..64", max_run);
    hm_deep *d = new hm_deep();
    d->device = device; d->W = W; d->H = H; d->max_run = max_run;
    d->n = (size_t)W * (size_t)H;
    *out = d;
    return HM_OK;
}

extern "C" int hm_deep_destroy(hm_deep_t d)
{
    if (!d) return HM_OK;
    if (!d->own.mem.empty() || !d->own.streams.empty() || !d->own.events.empty()) {
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();           // (maps queued on the callers' streams read the handle's buffers)
        d->own.release();
    }
    delete d;
    return HM_OK;
}

static int deep_buffers(hm_deep *d)
{
    HM_HIP(hipSetDevice(d->device));
    if (!d->ready) {
        const size_t run = (size_t)d->max_run;
        HM_HIP(d->own.alloc(&d->d_in, run * d->n * sizeof(uint16_t)));
        HM_HIP(d->own.alloc(&d->d_lut, (size_t)DEEP_VALUES));
        HM_HIP(d->own.alloc(&d->d_clip, 2 * run * sizeof(unsigned)));
        HM_HIP(d->own.alloc(&d->d_hist, (size_t)DEEP_VALUES * sizeof(unsigned long long)));
        for (hm_deep::Stage &s : d->stage) {
            HM_HIP(d->own.host_alloc(&s.px, run * d->n * sizeof(uint16_t), hipHostMallocDefault));
            HM_HIP(d->own.event(&s.copied));
        }
        HM_HIP(d->own.stream(&d->stream, false));
        HM_HIP(hipMemset(d->d_hist, 0, (size_t)DEEP_VALUES * sizeof(unsigned long long)));
        HM_HIP(hipDeviceSynchronize());
        d->ready = true;
    }
    if (d->have_lut && !d->lut_sent) {
        HM_HIP(hipDeviceSynchronize());         // (maps queued with the table before may still read it)
        HM_HIP(hipMemcpy(d->d_lut, d->lut.data(), (size_t)DEEP_VALUES, hipMemcpyHostToDevice));
        d->lut_sent = true;
    }
    return HM_OK;
}

// the next staging block, free to be written
static int deep_stage(hm_deep *d, hm_deep::Stage **st)
{
    *st = &d->stage[d->turn];
    d->turn ^= 1;
    if ((*st)->used) HM_HIP(hipEventSynchronize((*st)->copied));
    return HM_OK;
}

extern "C" int hm_deep_hist_reset(hm_deep_t d)
{
    HM_ARG(d, "hm_deep_hist_reset: NULL handle");
    d->samples = 0;
    if (!d->ready) return HM_OK;                 // (nothing was ever added)
    HM_HIP(hipSetDevice(d->device));
    HM_HIP(hipMemsetAsync(d->d_hist, 0, (size_t)DEEP_VALUES * sizeof(unsigned long long), d->stream));
    HM_HIP(hipStreamSynchronize(d->stream));
    return HM_OK;
}

extern "C" int hm_deep_hist_add(hm_deep_t d, int64_t nframes, const uint16_t *host_frames, int swap)
{
    HM_ARG(d && host_frames, "hm_deep_hist_add: NULL argument");
    HM_ARG(nframes >= 1, "hm_deep_hist_add: %lld frames, at least 1 is needed", (long long)nframes);
    HM_TRY(deep_buffers(d));
    for (int64_t f0 = 0; f0 < nframes; f0 += d->max_run) {
        const size_t k = (size_t)std::min<int64_t>(d->max_run, nframes - f0);
        const size_t total = k * d->n;
        hm_deep::Stage *st;
        HM_TRY(deep_stage(d, &st));
        memcpy(st->px, host_frames + (size_t)f0 * d->n, total * sizeof(uint16_t));
        // (the launch before reads d_in: this copy is behind it on the same stream)
        HM_HIP(hipMemcpyAsync(d->d_in, st->px, total * sizeof(uint16_t), hipMemcpyHostToDevice, d->stream));
        HM_HIP(hipEventRecord(st->copied, d->stream));
        st->used = true;
        // chunks of at least 32768 pixels (a workgroup's fill and flush are 16384 bins each), at most 256 of them
        const size_t chunks = std::min<size_t>(256, std::max<size_t>(1, total / 32768));
        const size_t per = ((total + chunks - 1) / chunks + DEEP_VEC - 1) / DEEP_VEC * DEEP_VEC;
        const unsigned gx = (unsigned)((total + per - 1) / per);
        hipLaunchKernelGGL(k_deep_hist, dim3(gx, DEEP_VALUES / DEEP_HIST_BINS), dim3(DEEP_HIST_THREADS), 0, d->stream,
                           (const uint16_t *)d->d_in, total, per, swap ? 1 : 0, d->d_hist);
        HM_HIP(hipGetLastError());
        d->samples += total;
    }
    HM_HIP(hipStreamSynchronize(d->stream));
    return HM_OK;
}

extern "C" int hm_deep_hist_get(hm_deep_t d, uint64_t *hist, uint64_t *samples)
{
    HM_ARG(d && hist, "hm_deep_hist_get: NULL argument");
    if (samples) *samples = d->samples;
    if (!d->ready) {                             // (nothing was ever added)
        memset(hist, 0, (size_t)DEEP_VALUES * sizeof(uint64_t));
        return HM_OK;
    }
    HM_HIP(hipSetDevice(d->device));
    HM_HIP(hipMemcpyAsync(hist, d->d_hist, (size_t)DEEP_VALUES * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipStreamSynchronize(d->stream));
    return HM_OK;
}

extern "C" int hm_deep_set_lut(hm_deep_t d, const uint8_t *lut, int lo, int hi)
{
    HM_ARG(d && lut, "hm_deep_set_lut: NULL argument");
    HM_ARG(lo >= 0 && hi <= DEEP_VALUES - 1, "hm_deep_set_lut: window %d..%d outside 0..65535", lo, hi);
    HM_ARG(lo < hi, "hm_deep_set_lut: lo %d >= hi %d: a window needs lo < hi", lo, hi);
    d->lut.assign(lut, lut + DEEP_VALUES);
    d->lo = lo; d->hi = hi;
    d->have_lut = true;
    d->lut_sent = false;
    return HM_OK;
}

extern "C" int hm_deep_map_run_dev(hm_deep_t d, int nframes, const uint16_t *host_frames, int swap, void *d_frame, void *d_mask,
                                   void *d_shown, uint64_t stride, int threshold, uint32_t *d_status, void *stream)
{
    HM_ARG(d && host_frames && d_frame, "hm_deep_map_run_dev: NULL argument");
    HM_ARG(nframes >= 1 && nframes <= d->max_run, "hm_deep_map_run_dev: %d frames outside 1..max_run = %d", nframes, d->max_run);
    HM_ARG(threshold >= 0 && threshold <= 255, "hm_deep_map_run_dev: threshold %d outside 0..255", threshold);
    HM_ARG(nframes == 1 || stride >= (uint64_t)d->n, "hm_deep_map_run_dev: a frame stride of %llu for frames of %zu pixels",
           (unsigned long long)stride, d->n);
    if (!d->have_lut) {
        hm_set_error("hm_deep_map_run_dev: no table set (hm_deep_set_lut comes first)");
        return HM_ERR_STATE;
    }
    HM_TRY(deep_buffers(d));
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)nframes * d->n;
    hm_deep::Stage *st;
    HM_TRY(deep_stage(d, &st));
    memcpy(st->px, host_frames, total * sizeof(uint16_t));
    HM_HIP(hipMemcpyAsync(d->d_in, st->px, total * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    HM_HIP(hipEventRecord(st->copied, s));
    st->used = true;
    d->last_h2d = total * sizeof(uint16_t);
    d->total_h2d += d->last_h2d;
    HM_HIP(hipMemsetAsync(d->d_clip, 0, 2 * (size_t)nframes * sizeof(unsigned), s));
    DeepOut o{};
    o.frame = (uint8_t *)d_frame; o.mask = (uint8_t *)d_mask; o.shown = (uint8_t *)d_shown;
    o.stride = (size_t)stride; o.n = d->n;
    o.lo = (unsigned)d->lo; o.hi = (unsigned)d->hi;
    o.threshold = threshold; o.swap = swap ? 1 : 0;
    o.base8 = (((uintptr_t)d_frame | (uintptr_t)d_mask | (uintptr_t)d_shown) & 7) == 0;
    const size_t nvec = d->n / DEEP_VEC + 2;                       // (a frame's vectors: at most this many)
    // four vectors a thread where the frame has them, at most 256 blocks a frame: few workgroups, so few clip atomics
    const unsigned gx = (unsigned)std::min<size_t>(256, (nvec + 4 * DEEP_MAP_THREADS - 1) / (4 * DEEP_MAP_THREADS));
    hipLaunchKernelGGL(k_deep_map, dim3(gx, (unsigned)nframes), dim3(DEEP_MAP_THREADS), 0, s, (const uint16_t *)d->d_in,
                       (const uint8_t *)d->d_lut, o, d->d_clip);
    HM_HIP(hipGetLastError());
    if (d_status)
        HM_HIP(hipMemcpyAsync(d_status, d->d_clip, 2 * (size_t)nframes * sizeof(uint32_t), hipMemcpyDefault, s));
    return HM_OK;
}

extern "C" int hm_deep_map(hm_deep_t d, const uint16_t *host_frame, int swap, uint8_t *out, uint32_t *clipped)
{
    HM_ARG(d && host_frame && out, "hm_deep_map: NULL argument");
    if (!d->have_lut) {
        hm_set_error("hm_deep_map: no table set (hm_deep_set_lut comes first)");
        return HM_ERR_STATE;
    }
    HM_TRY(deep_buffers(d));
    HM_HIP(d->own.alloc(&d->d_out, d->n));
    HM_TRY(hm_deep_map_run_dev(d, 1, host_frame, swap, d->d_out, nullptr, nullptr, (uint64_t)d->n, 0, nullptr, d->stream));
    uint32_t clip[2] = {0, 0};
    HM_HIP(hipMemcpyAsync(clip, d->d_clip, sizeof(clip), hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipMemcpyAsync(out, d->d_out, d->n, hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipStreamSynchronize(d->stream));
    if (clipped) { clipped[0] = clip[0]; clipped[1] = clip[1]; }
    return HM_OK;
}

extern "C" int hm_deep_uploaded(hm_deep_t d, uint64_t *last_run, uint64_t *total)
{
    HM_ARG(d, "hm_deep_uploaded: NULL handle");
    if (last_run) *last_run = d->last_h2d;
    if (total) *total = d->total_h2d;
    return HM_OK;
}

// ---- full-depth traces (deeptrace_kernels.h) ---------------------------------------------------------------------------
static int deep_same_frame(const hm_deep *d, const BodyMapView &v, const char *who)
{
    HM_ARG(d->device == v.device && d->W == v.W && d->H == v.H,
           "%s: the deep handle is %dx%d on device %d, the filter handle %dx%d on device %d: they must agree", who, d->W, d->H,
           d->device, v.W, v.H, v.device);
    return HM_OK;
}

extern "C" int hm_deep_body_set_columns(hm_deep_t d, hm_ctx_t h, int C, const int64_t *col_ptr, const int32_t *pix,
                                        const uint16_t *wt)
{
    HM_ARG(d && h, "hm_deep_body_set_columns: NULL handle");
    if (!pix) {                                  // clears
        d->C = 0; d->col_ptr.clear(); d->npieces = 0; d->pieces_E = 0;
        return HM_OK;
    }
    HM_ARG(C >= 1 && C <= 4096, "hm_deep_body_set_columns: %d columns outside 1..4096", C);
    HM_ARG(col_ptr && wt, "hm_deep_body_set_columns: NULL col_ptr or wt");
    HM_ARG(col_ptr[0] == 0, "hm_deep_body_set_columns: col_ptr[0] = %lld, not 0", (long long)col_ptr[0]);
    for (int s = 0; s < C; s++)
        HM_ARG(col_ptr[s + 1] >= col_ptr[s], "hm_deep_body_set_columns: col_ptr is not ascending at column %d: %lld after %lld", s,
               (long long)col_ptr[s + 1], (long long)col_ptr[s]);
    const int64_t M = col_ptr[C];
    HM_ARG(M <= (int64_t)DEEP_COL_ENTRIES_MAX, "hm_deep_body_set_columns: %lld entries, at most %d", (long long)M, DEEP_COL_ENTRIES_MAX);
    for (int64_t e = 0; e < M; e++)
        HM_ARG(pix[e] >= 0 && (size_t)pix[e] < d->n, "hm_deep_body_set_columns: entry %lld is pixel %d, outside 0..%zu (a %dx%d frame)",
               (long long)e, pix[e], d->n - 1, d->W, d->H);
    BodyMapView v;
    HM_TRY(body_map_view(h, &v));
    HM_TRY(deep_same_frame(d, v, "hm_deep_body_set_columns"));
    HM_TRY(deep_buffers(d));
    HM_HIP(hipStreamSynchronize(d->stream));
    d->C = 0;                                    // (until the columns are in place)
    const size_t m = (size_t)std::max<int64_t>(M, 1);
    HM_HIP(d->own.grow(&d->d_pix, m * sizeof(int)));
    HM_HIP(d->own.grow(&d->d_wt, m * sizeof(uint16_t)));
    if (M) {
        HM_HIP(hipMemcpy(d->d_pix, pix, (size_t)M * sizeof(int), hipMemcpyHostToDevice));
        HM_HIP(hipMemcpy(d->d_wt, wt, (size_t)M * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    d->col_ptr.assign(col_ptr, col_ptr + C + 1);
    d->pieces_E = 0;
    d->C = C;
    return HM_OK;
}

// the columns cut into pieces of at most E entries, on the device
static int deep_pieces(hm_deep *d, int E)
{
    if (d->pieces_E == E) return HM_OK;
    std::vector<DeepPiece> pc;
    d->any_split = false;
    for (int s = 0; s < d->C; s++) {
        const int64_t a = d->col_ptr[s], len = d->col_ptr[s + 1] - a;
        if (len <= E) { pc.push_back(DeepPiece{(long long)a, (int)len, s}); continue; }
        d->any_split = true;
        for (int64_t o = 0; o < len; o += E)
            pc.push_back(DeepPiece{(long long)(a + o), (int)std::min<int64_t>(E, len - o), (int)((unsigned)s | DEEP_PIECE_SPLIT)});
    }
    HM_HIP(hipStreamSynchronize(d->stream));     // (a launch before read the pieces in place)
    HM_HIP(d->own.grow(&d->d_pieces, pc.size() * sizeof(DeepPiece)));
    HM_HIP(hipMemcpy(d->d_pieces, pc.data(), pc.size() * sizeof(DeepPiece), hipMemcpyHostToDevice));
    d->npieces = (int)pc.size();
    d->pieces_E = E;
    return HM_OK;
}

extern "C" int hm_deep_body_run(hm_deep_t d, hm_ctx_t h, int64_t nframes, const uint16_t *host_frames, int swap, const double *X,
                                uint64_t *sums, uint16_t *planes)
{
    HM_ARG(d && h, "hm_deep_body_run: NULL handle");
    HM_ARG(host_frames && X, "hm_deep_body_run: NULL frames or states");
    HM_ARG(nframes >= 1, "hm_deep_body_run: %lld frames, at least 1 is needed", (long long)nframes);
    HM_ARG(sums || planes, "hm_deep_body_run: neither sums nor planes asked for");
    if (sums && d->C == 0) {
        hm_set_error("hm_deep_body_run: sums asked for, and hm_deep_body_set_columns has set no columns");
        return HM_ERR_STATE;
    }
    BodyMapView v;
    HM_TRY(body_map_view(h, &v));
    HM_TRY(deep_same_frame(d, v, "hm_deep_body_run"));
    HM_TRY(deep_buffers(d));
    const size_t run = (size_t)d->max_run, n = d->n, xs = (size_t)4 * v.N, C = (size_t)d->C;
    HM_HIP(d->own.alloc(&d->d_in2, run * n * sizeof(uint16_t)));
    HM_HIP(d->own.stream(&d->up_stream, false));
    for (int b = 0; b < 2; b++) {
        HM_HIP(d->own.grow(&d->d_X[b], run * xs * sizeof(double)));
        HM_HIP(d->own.host_grow(&d->h_X[b], run * xs * sizeof(double), hipHostMallocDefault));
        HM_HIP(d->own.event(&d->uploaded[b]));
        HM_HIP(d->own.event(&d->consumed[b]));
    }
    if (sums) {
        HM_HIP(d->own.grow(&d->d_sums, run * C * sizeof(unsigned long long)));
        HM_TRY(deep_pieces(d, v.col_entries));
    }
    if (planes) HM_HIP(d->own.alloc(&d->d_planes, run * n * sizeof(uint16_t)));
    uint16_t *const in[2] = {d->d_in, d->d_in2};
    const int64_t runs = (nframes + d->max_run - 1) / d->max_run;
    // the upload of run i: staged, then copied on the upload stream once the kernels of run i - 2 have read the copy it replaces
    auto upload = [&](int64_t i) -> int {
        const int b = (int)(i & 1);
        const int64_t f0 = i * d->max_run;
        const size_t k = (size_t)std::min<int64_t>(d->max_run, nframes - f0);
        hm_deep::Stage *st;
        HM_TRY(deep_stage(d, &st));
        memcpy(st->px, host_frames + (size_t)f0 * n, k * n * sizeof(uint16_t));
        if (i >= 2) HM_HIP(hipStreamWaitEvent(d->up_stream, d->consumed[b], 0));
        HM_HIP(hipMemcpyAsync(in[b], st->px, k * n * sizeof(uint16_t), hipMemcpyHostToDevice, d->up_stream));
        // (the states go through a page-locked block as the frames do: a copy from the caller's pageable memory could hold
        // this thread until the stream reaches it)
        if (i >= 2) HM_HIP(hipEventSynchronize(d->uploaded[b]));
        memcpy(d->h_X[b], X + (size_t)f0 * xs, k * xs * sizeof(double));
        HM_HIP(hipMemcpyAsync(d->d_X[b], d->h_X[b], k * xs * sizeof(double), hipMemcpyHostToDevice, d->up_stream));
        HM_HIP(hipEventRecord(st->copied, d->up_stream));
        st->used = true;
        HM_HIP(hipEventRecord(d->uploaded[b], d->up_stream));
        return HM_OK;
    };
    int rc = upload(0);
    for (int64_t i = 0; i < runs && rc == HM_OK; i++) {
        rc = [&]() -> int {
            const int b = (int)(i & 1);
            const int64_t f0 = i * d->max_run;
            const size_t k = (size_t)std::min<int64_t>(d->max_run, nframes - f0);
            HM_HIP(hipStreamWaitEvent(d->stream, d->uploaded[b], 0));
            DeepWarp a;
            a.n = (int)n; a.W = d->W; a.H = d->H; a.swap = swap ? 1 : 0;
            a.tri_of = v.tri; a.bary = v.bary; a.tidx = v.tidx;
            a.X = d->d_X[b]; a.xstride = xs; a.frames = in[b];
            if (sums) {
                // (the words the pieces of a split column add to; a whole column's word is stored, an empty column's too)
                if (d->any_split) HM_HIP(hipMemsetAsync(d->d_sums, 0, k * C * sizeof(unsigned long long), d->stream));
                hipLaunchKernelGGL(k_deep_cols, dim3((unsigned)hm_cdiv(d->npieces, DEEP_COL_WAVES), (unsigned)k), dim3(64 * DEEP_COL_WAVES),
                                   0, d->stream, a, d->npieces, d->C, (const DeepPiece *)d->d_pieces, (const int *)d->d_pix,
                                   (const uint16_t *)d->d_wt, d->d_sums);
            }
            if (planes)
                hipLaunchKernelGGL(k_body_warp16, dim3((unsigned)hm_cdiv(hm_cdiv((int)n, 4), 256), (unsigned)k), dim3(256), 0, d->stream, a,
                                   d->d_planes);
            HM_HIP(hipGetLastError());
            HM_HIP(hipEventRecord(d->consumed[b], d->stream));
            if (i + 1 < runs) HM_TRY(upload(i + 1));           // (before the downloads into pageable memory, which may hold this thread)
            if (sums)
                HM_HIP(hipMemcpyAsync(sums + (size_t)f0 * C, d->d_sums, k * C * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
            if (planes)
                HM_HIP(hipMemcpyAsync(planes + (size_t)f0 * n, d->d_planes, k * n * sizeof(uint16_t), hipMemcpyDeviceToHost, d->stream));
            return HM_OK;
        }();
    }
    // (also after a failure: nothing of this call is in flight when it returns)
    const hipError_t e1 = hipStreamSynchronize(d->up_stream), e2 = hipStreamSynchronize(d->stream);
    if (rc) return rc;
    HM_HIP(e1);
    HM_HIP(e2);
    return HM_OK;
}
