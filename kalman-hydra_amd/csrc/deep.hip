// 16-bit input (hm_deep_*, include/hydra_mi.h): host orchestration and C-ABI; the kernels are in
// deep_kernels.h, which this translation unit alone compiles.
// One handle owns the device copy of a run's 16-bit pixels, the table, the 64-bit histogram, the clip words and two
// page-locked staging blocks used in turn.  hm_deep_hist_add and hm_deep_map work on a stream of the handle's and return
// when they are done; hm_deep_map_run_dev queues on the caller's stream and returns.
#include "hm_common.h"
#include "deep_kernels.h"
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
