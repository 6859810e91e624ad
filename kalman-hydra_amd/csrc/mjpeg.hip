// Motion-JPEG on the device: the baseline JPEG encoder of the video writer (hm_mjpeg_*) and the decoder of AVI / MJPEG input
// (hm_mjpeg_dec_*).  Host orchestration and C-ABI (include/hydra_mi.h); the kernels are in mjpeg_kernels.h and
// mjpeg_dec_kernels.h, which this translation unit alone compiles; the decoder's parser and host entropy path are in
// mjpeg_dec.cpp (no HIP).  Both work on handles of their own (hm_mjpeg, hm_mjpeg_dec) and name no filter handle.
#include "hm_common.h"
#include "hm_types.h"
#include "mjpeg_kernels.h"
#include "mjpeg_tables.h"
#include "mjpeg_dec_kernels.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

// ---- Motion-JPEG: the baseline JPEG encoder of the video writer (mjpeg_kernels.h) ----------------
struct hm_mjpeg {
    int device = 0, quality = 0, restart_rows = 1;
    MjGeo g{};
    MjTables tab{};
    std::vector<uint8_t> header;
    uint64_t max_stream = 0;
    HmOwner own{1};
    // built by the first encode
    MjTables *d_tab = nullptr;
    int16_t *d_coef = nullptr;
    uint16_t *d_acbits = nullptr;
    unsigned *d_bitbuf = nullptr, *d_ibits = nullptr, *d_isize = nullptr, *d_ioff = nullptr;
    bool ready = false;
    // hm_mjpeg_encode's own
    hipStream_t stream = nullptr;
    uint8_t *d_frame = nullptr, *d_out = nullptr;
    unsigned *d_size = nullptr;
};

static void mj_header(hm_mjpeg *e)
{
    std::vector<uint8_t> &h = e->header;
    auto seg = [&](uint8_t marker, const std::vector<uint8_t> &body) {
        h.push_back(0xFF); h.push_back(marker);
        const size_t n = body.size() + 2;
        h.push_back((uint8_t)(n >> 8)); h.push_back((uint8_t)n);
        h.insert(h.end(), body.begin(), body.end());
    };
    const int C = e->g.C, sets = C == 3 ? 2 : 1;
    h.push_back(0xFF); h.push_back(0xD8);                                                       // SOI
    seg(0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                              // APP0: JFIF 1.01, 1:1
    for (int s = 0; s < sets; s++) {                                                            // DQT, 8 bits, zigzag order
        std::vector<uint8_t> b{(uint8_t)s};
        for (int k = 0; k < 64; k++) b.push_back((uint8_t)e->tab.quant[s][k]);
        seg(0xDB, b);
    }
    {                                                                                           // SOF0
        std::vector<uint8_t> b{8, (uint8_t)(e->g.H >> 8), (uint8_t)e->g.H, (uint8_t)(e->g.W >> 8), (uint8_t)e->g.W, (uint8_t)C};
        for (int c = 0; c < C; c++) { b.push_back((uint8_t)(c + 1)); b.push_back(0x11); b.push_back(c ? 1 : 0); }
        seg(0xC0, b);
    }
    for (int s = 0; s < sets; s++) {                                                            // DHT: DC then AC of each set
        std::vector<uint8_t> b{(uint8_t)s};
        b.insert(b.end(), MJ_DC_BITS[s], MJ_DC_BITS[s] + 16);
        b.insert(b.end(), MJ_DC_VALS, MJ_DC_VALS + 12);
        seg(0xC4, b);
        std::vector<uint8_t> a{(uint8_t)(0x10 | s)};
        a.insert(a.end(), MJ_AC_BITS[s], MJ_AC_BITS[s] + 16);
        a.insert(a.end(), MJ_AC_VALS[s], MJ_AC_VALS[s] + 162);
        seg(0xC4, a);
    }
    seg(0xDD, {(uint8_t)(e->g.ri >> 8), (uint8_t)e->g.ri});                                     // DRI
    {                                                                                           // SOS
        std::vector<uint8_t> b{(uint8_t)C};
        for (int c = 0; c < C; c++) { b.push_back((uint8_t)(c + 1)); b.push_back(c ? 0x11 : 0x00); }
        b.push_back(0); b.push_back(63); b.push_back(0);
        seg(0xDA, b);
    }
}

extern "C" int hm_mjpeg_create(int device, int W, int H, int channels, int quality, int restart_rows, hm_mjpeg_t *out)
{
    HM_ARG(out, "hm_mjpeg_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "hm_mjpeg_create: frame size %dx%d outside 1..32767", W, H);
    HM_ARG(channels == 1 || channels == 3, "hm_mjpeg_create: %d channels, not 1 or 3", channels);
    HM_ARG(quality >= 1 && quality <= 100, "hm_mjpeg_create: quality %d outside 1..100", quality);
    HM_ARG(restart_rows >= 1, "hm_mjpeg_create: restart_rows %d below 1", restart_rows);
    const int bw = (W + 7) / 8, bh = (H + 7) / 8;
    const long long ri = (long long)bw * std::min(restart_rows, bh);
    HM_ARG(ri <= 65535, "hm_mjpeg_create: %lld blocks in a restart interval (%d across, %d rows), more than 65535", ri, bw,
           std::min(restart_rows, bh));
    hm_mjpeg *e = new hm_mjpeg();
    e->device = device; e->quality = quality; e->restart_rows = restart_rows;
    MjGeo &g = e->g;
    g.W = W; g.H = H; g.C = channels; g.bw = bw; g.bh = bh;
    g.ri = (int)ri;
    g.n_mcu = bw * bh;
    g.n_int = (g.n_mcu + g.ri - 1) / g.ri;
    e->max_stream = (uint64_t)g.n_mcu * channels * (8 * MJ_BLOCK_WORDS) + 2ull * g.n_int;
    if (e->max_stream >= (1ull << 31)) {
        hm_set_error("hm_mjpeg_create: a frame of %dx%d x %d can code to %llu bytes, 2^31 or more", W, H, channels,
                     (unsigned long long)e->max_stream);
        delete e;
        return HM_ERR_ARG;
    }
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int s = 0; s < 2; s++) {
        for (int i = 0; i < 64; i++)
            e->tab.quant[s][mj_zigzag_pos(i)] = (uint16_t)std::min(255, std::max(1, (MJ_QUANT[s][i] * scale + 50) / 100));
        mj_huffman(MJ_DC_BITS[s], MJ_DC_VALS, e->tab.dc_code[s], e->tab.dc_len[s]);
        mj_huffman(MJ_AC_BITS[s], MJ_AC_VALS[s], e->tab.ac_code[s], e->tab.ac_len[s]);
    }
    mj_header(e);
    *out = e;
    return HM_OK;
}

extern "C" int hm_mjpeg_destroy(hm_mjpeg_t e)
{
    if (!e) return HM_OK;
    if (!e->own.mem.empty() || !e->own.streams.empty()) {      // (also what a first encode that failed part-way left)
        (void)hipSetDevice(e->device);
        (void)hipDeviceSynchronize();           // (encodes queued on the callers' streams read the handle's buffers)
        e->own.release();
    }
    delete e;
    return HM_OK;
}

extern "C" int hm_mjpeg_header(hm_mjpeg_t e, uint8_t *buf, uint64_t cap, uint64_t *n)
{
    HM_ARG(e && n, "hm_mjpeg_header: NULL argument");
    *n = e->header.size();
    if (!buf) return HM_OK;                     // (the size alone)
    HM_ARG(cap >= e->header.size(), "hm_mjpeg_header: the header has %zu bytes, the buffer %llu", e->header.size(),
           (unsigned long long)cap);
    memcpy(buf, e->header.data(), e->header.size());
    return HM_OK;
}

extern "C" uint64_t hm_mjpeg_max_bytes(hm_mjpeg_t e) { return e ? e->header.size() + e->max_stream : 0; }

static int mj_buffers(hm_mjpeg *e)
{
    if (e->ready) return HM_OK;
    const MjGeo &g = e->g;
    const size_t nblk = (size_t)g.n_mcu * g.C;
    HM_HIP(e->own.alloc(&e->d_tab, sizeof(MjTables)));
    HM_HIP(e->own.alloc(&e->d_coef, nblk * 64 * sizeof(int16_t)));
    HM_HIP(e->own.alloc(&e->d_acbits, nblk * sizeof(uint16_t)));
    HM_HIP(e->own.alloc(&e->d_bitbuf, nblk * MJ_BLOCK_WORDS * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_ibits, (size_t)g.n_int * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_isize, (size_t)g.n_int * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_ioff, ((size_t)g.n_int + 1) * sizeof(unsigned)));
    HM_HIP(hipMemcpy(e->d_tab, &e->tab, sizeof(MjTables), hipMemcpyHostToDevice));
    HM_HIP(hipMemset(e->d_bitbuf, 0, nblk * MJ_BLOCK_WORDS * sizeof(unsigned)));     // k_mjpeg_pack keeps it zero
    HM_HIP(hipDeviceSynchronize());
    e->ready = true;
    return HM_OK;
}

extern "C" int hm_mjpeg_encode_dev(hm_mjpeg_t e, const void *d_frame, void *out, uint64_t cap, uint32_t *size_word, void *stream)
{
    HM_ARG(e && d_frame && out && size_word, "hm_mjpeg_encode_dev: NULL argument");
    HM_HIP(hipSetDevice(e->device));
    HM_TRY(mj_buffers(e));
    const MjGeo &g = e->g;
    hipStream_t s = (hipStream_t)stream;
    const unsigned cap32 = (unsigned)std::min<uint64_t>(cap, 0xFFFFFFFFull);
    hipLaunchKernelGGL(k_mjpeg_blocks, dim3((unsigned)hm_cdiv(g.n_mcu, mj_blocks_mcus(g.C))), dim3(MJ_THREADS), 0, s, g,
                       (const MjTables *)e->d_tab, (const uint8_t *)d_frame, e->d_coef, e->d_acbits);
    const int emit_threads = std::min(MJ_EMIT_MAX, (g.ri * g.C + 63) / 64 * 64);       // whole waves
    hipLaunchKernelGGL(k_mjpeg_emit, dim3((unsigned)g.n_int), dim3((unsigned)emit_threads), 0, s, g, (const MjTables *)e->d_tab,
                       (const int16_t *)e->d_coef, (const uint16_t *)e->d_acbits, e->d_bitbuf, e->d_ibits);
    hipLaunchKernelGGL(k_mjpeg_count, dim3((unsigned)g.n_int), dim3(MJ_THREADS), 0, s, g, (const unsigned *)e->d_bitbuf,
                       (const unsigned *)e->d_ibits, e->d_isize);
    hipLaunchKernelGGL(k_mjpeg_offsets, dim3(1), dim3(MJ_THREADS), 0, s, g, (const unsigned *)e->d_isize, e->d_ioff);
    hipLaunchKernelGGL(k_mjpeg_pack, dim3((unsigned)g.n_int), dim3(MJ_THREADS), 0, s, g, e->d_bitbuf, (const unsigned *)e->d_ibits,
                       (const unsigned *)e->d_isize, (const unsigned *)e->d_ioff, (uint8_t *)out, cap32, (unsigned *)size_word);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_mjpeg_encode(hm_mjpeg_t e, const uint8_t *frame, uint8_t *out, uint64_t cap, uint64_t *n)
{
    HM_ARG(e && frame && out && n, "hm_mjpeg_encode: NULL argument");
    *n = 0;
    const size_t hdr = e->header.size();
    HM_ARG(cap > hdr, "hm_mjpeg_encode: a buffer of %llu bytes does not hold the header's %zu", (unsigned long long)cap, hdr);
    HM_HIP(hipSetDevice(e->device));
    const size_t fb = (size_t)e->g.W * e->g.H * e->g.C;
    const uint64_t room = std::min<uint64_t>(cap - hdr, e->max_stream);
    HM_HIP(e->own.stream(&e->stream, false));
    HM_HIP(e->own.alloc(&e->d_frame, fb));
    HM_HIP(e->own.grow(&e->d_out, (size_t)room));
    HM_HIP(e->own.alloc(&e->d_size, sizeof(unsigned)));
    HM_HIP(hipMemcpyAsync(e->d_frame, frame, fb, hipMemcpyHostToDevice, e->stream));
    HM_TRY(hm_mjpeg_encode_dev(e, e->d_frame, e->d_out, room, e->d_size, e->stream));
    unsigned size = 0;
    HM_HIP(hipMemcpyAsync(&size, e->d_size, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    HM_HIP(hipStreamSynchronize(e->stream));
    *n = hdr + size;
    HM_ARG(size <= room, "hm_mjpeg_encode: the frame codes to %zu + %u bytes, the buffer has %llu", hdr, size,
           (unsigned long long)cap);
    memcpy(out, e->header.data(), hdr);
    HM_HIP(hipMemcpy(out + hdr, e->d_out, size, hipMemcpyDeviceToHost));
    return HM_OK;
}


// ---- Motion-JPEG, decoding (mjpeg_dec_kernels.h, mjpeg_dec.cpp) -----------------------------------

static_assert(sizeof(MjdFrame) == HM_MJPEG_DESC_BYTES, "hydra_mi.h states the size of a frame's descriptor");

struct hm_mjpeg_dec {
    int device = 0, W = 0, H = 0, max_run = 1;
    int entropy = HM_MJPEG_ENTROPY_AUTO, pool = 4;                          // hm_mjpeg_dec_tune
    int auto_intervals = 512;                    // hm_mjpeg_dec_tune "auto_intervals": measured, DESIGN section 23 (256: the host pool still wins)
    size_t blk_cap = 0;                          // luma blocks of a frame's slot in the coefficient buffer
    HmOwner own{1};
    std::vector<MjdParsed> parsed;               // per frame of a run, reused
    MjdPool *workers = nullptr;                  // the host entropy path's threads: started by the first run that needs them
    uint64_t last_h2d = 0, total_h2d = 0;        // bytes the last run, and all runs, queued host-to-device
    // built by the first decode; the byte and interval buffers grow when a run is larger than any before
    bool ready = false;
    MjdFrame *d_frames = nullptr;
    MjdInterval *d_iv = nullptr;
    uint8_t *d_bytes = nullptr;
    int16_t *d_coef = nullptr;
    unsigned *d_bad = nullptr;
    size_t iv_cap = 0, bytes_cap = 0;
    struct Stage {                               // page-locked; two, used in turn, so that a run never writes what the copies
        MjdFrame *frames = nullptr;              // of the run before may still read
        MjdInterval *iv = nullptr;
        uint8_t *bytes = nullptr;
        int16_t *coef = nullptr;                 // host entropy path only
        hipEvent_t copied = nullptr;
        bool used = false;
    } stage[2];
    int turn = 0;
    // hm_mjpeg_decode's own
    hipStream_t stream = nullptr;
    uint8_t *d_out = nullptr;
    uint32_t *d_status = nullptr;
};

extern "C" int hm_mjpeg_dec_create(int device, int W, int H, int max_run, hm_mjpeg_dec_t *out)
{
    HM_ARG(out, "hm_mjpeg_dec_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "hm_mjpeg_dec_create: frame size %dx%d outside 1..32767", W, H);
    HM_ARG(max_run >= 1 && max_run <= 64, "hm_mjpeg_dec_create: max_run %d outside 1..64", max_run);
    hm_mjpeg_dec *d = new hm_mjpeg_dec();
    d->device = device; d->W = W; d->H = H; d->max_run = max_run;
    d->blk_cap = (size_t)(2 * ((W + 15) / 16)) * (size_t)(2 * ((H + 15) / 16));        // covers every accepted sampling
    d->parsed.resize((size_t)max_run);
    *out = d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_destroy(hm_mjpeg_dec_t d)
{
    if (!d) return HM_OK;
    if (!d->own.mem.empty() || !d->own.streams.empty() || !d->own.events.empty()) {
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();           // (decodes queued on the callers' streams read the handle's buffers)
        d->own.release();
    }
    delete d->workers;
    delete d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_uploaded(hm_mjpeg_dec_t d, uint64_t *last_run, uint64_t *total)
{
    HM_ARG(d, "hm_mjpeg_dec_uploaded: NULL handle");
    if (last_run) *last_run = d->last_h2d;
    if (total) *total = d->total_h2d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_tune(hm_mjpeg_dec_t d, const char *name, int value)
{
    HM_ARG(d && name, "hm_mjpeg_dec_tune: NULL argument");
    const std::string n(name);
    if (n == "entropy") {
        HM_ARG(value >= HM_MJPEG_ENTROPY_AUTO && value <= HM_MJPEG_ENTROPY_DEVICE, "hm_mjpeg_dec_tune: entropy %d is none of 0 auto, 1 host, 2 device", value);
        d->entropy = value;
    } else if (n == "pool") {
        HM_ARG(value >= 1 && value <= 16, "hm_mjpeg_dec_tune: pool %d outside 1..16", value);
        d->pool = value;
    } else if (n == "auto_intervals") {
        HM_ARG(value >= 0, "hm_mjpeg_dec_tune: auto_intervals %d below 0", value);
        d->auto_intervals = value;
    } else {
        HM_ARG(false, "hm_mjpeg_dec_tune: no tune named '%s' (entropy, pool, auto_intervals)", name);
    }
    return HM_OK;
}

static int mjd_parse_for(hm_mjpeg_dec *d, const char *who, const uint8_t *file, uint64_t n, MjdParsed *p)
{
    HM_TRY(mjd_parse(file, n, p));
    HM_ARG(p->W == d->W && p->H == d->H, "%s: a frame of %dx%d for a decoder of %dx%d", who, p->W, p->H, d->W, d->H);
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_entropy_host(hm_mjpeg_dec_t d, const uint8_t *file, uint64_t n, int16_t *coef, uint64_t cap,
                                         uint32_t *bad)
{
    HM_ARG(d && file && coef && bad, "hm_mjpeg_dec_entropy_host: NULL argument");
    MjdParsed &p = d->parsed[0];
    HM_TRY(mjd_parse_for(d, "hm_mjpeg_dec_entropy_host", file, n, &p));
    const uint64_t need = (uint64_t)p.frame.scan.n_mcu * p.hs * p.vs * 64;
    HM_ARG(cap >= need, "hm_mjpeg_dec_entropy_host: %llu coefficients, room for %llu", (unsigned long long)need, (unsigned long long)cap);
    HM_ARG(((uintptr_t)coef & 7) == 0, "hm_mjpeg_dec_entropy_host: coef is not 8-byte aligned");
    *bad = mjd_entropy_host(p, file, coef);
    return HM_OK;
}

static int mjd_buffers(hm_mjpeg_dec *d)
{
    if (d->ready) return HM_OK;
    const size_t run = (size_t)d->max_run;
    HM_HIP(d->own.alloc(&d->d_frames, run * sizeof(MjdFrame)));
    HM_HIP(d->own.alloc(&d->d_coef, run * d->blk_cap * 64 * sizeof(int16_t)));
    HM_HIP(d->own.alloc(&d->d_bad, run * sizeof(unsigned)));
    for (hm_mjpeg_dec::Stage &s : d->stage) {
        HM_HIP(d->own.host_alloc(&s.frames, run * sizeof(MjdFrame), hipHostMallocDefault));
        HM_HIP(d->own.event(&s.copied));
    }
    HM_HIP(hipMemset(d->d_bad, 0, run * sizeof(unsigned)));       // k_mjdec_idct keeps it zero
    HM_HIP(hipDeviceSynchronize());
    d->ready = true;
    return HM_OK;
}

extern "C" int hm_mjpeg_decode_run_dev(hm_mjpeg_dec_t d, int nframes, const uint8_t *const *files, const uint64_t *sizes,
                                       void *d_frame, void *d_mask, void *d_shown, uint64_t frame_stride, uint64_t pitch,
                                       int threshold, uint32_t *status_words, void *stream)
{
    HM_ARG(d && files && sizes && d_frame, "hm_mjpeg_decode_run_dev: NULL argument");
    HM_ARG(nframes >= 1 && nframes <= d->max_run, "hm_mjpeg_decode_run_dev: %d frames outside 1..max_run = %d", nframes, d->max_run);
    HM_ARG(pitch >= (uint64_t)d->W, "hm_mjpeg_decode_run_dev: a row pitch of %llu for rows of %d", (unsigned long long)pitch, d->W);
    HM_ARG(nframes == 1 || frame_stride >= pitch * (uint64_t)(d->H - 1) + (uint64_t)d->W,
           "hm_mjpeg_decode_run_dev: a frame stride of %llu for frames of %d rows at pitch %llu", (unsigned long long)frame_stride, d->H,
           (unsigned long long)pitch);
    // the frames: parsed and refused before anything is queued
    size_t n_iv = 0, n_bytes = 0, n_host = 0;
    unsigned max_int = 0, max_blk = 0;
    for (int i = 0; i < nframes; i++) {
        HM_ARG(files[i], "hm_mjpeg_decode_run_dev: frame %d is NULL", i);
        MjdParsed &p = d->parsed[(size_t)i];
        HM_TRY(mjd_parse_for(d, "hm_mjpeg_decode_run_dev", files[i], sizes[i], &p));
        MjdFrame &f = p.frame;
        const bool dev = d->entropy == HM_MJPEG_ENTROPY_DEVICE ||
                         (d->entropy == HM_MJPEG_ENTROPY_AUTO && (d->auto_intervals > 0 ? f.n_int >= (unsigned)d->auto_intervals : p.ri != 0));
        f.dev_entropy = dev ? 1 : 0;
        f.bad_host = 0;
        f.int_off = (uint32_t)n_iv;
        f.data_off = (uint32_t)n_bytes;
        const unsigned nblk = f.scan.n_mcu * (unsigned)(p.hs * p.vs);
        HM_ARG(nblk <= d->blk_cap, "hm_mjpeg_decode_run_dev: %u blocks in frame %d, room for %zu", nblk, i, d->blk_cap);
        max_blk = std::max(max_blk, nblk);
        if (dev) {
            n_iv += f.n_int;
            n_bytes += ((size_t)sizes[i] + 15) & ~(size_t)15;
            max_int = std::max(max_int, f.n_int);
        } else {
            n_host++;
        }
    }
    HM_ARG(n_bytes < (1ull << 32), "hm_mjpeg_decode_run_dev: %zu bytes in a run, 2^32 or more", n_bytes);
    HM_HIP(hipSetDevice(d->device));
    HM_TRY(mjd_buffers(d));
    hipStream_t s = (hipStream_t)stream;
    hm_mjpeg_dec::Stage &st = d->stage[d->turn];
    d->turn ^= 1;
    if (st.used) HM_HIP(hipEventSynchronize(st.copied));          // (the copies of the run before last: long done)
    if (n_iv) {
        HM_HIP(d->own.host_grow(&st.iv, n_iv * sizeof(MjdInterval), hipHostMallocDefault));
        HM_HIP(d->own.host_grow(&st.bytes, n_bytes, hipHostMallocDefault));
        if (n_iv > d->iv_cap || n_bytes > d->bytes_cap) {
            HM_HIP(hipDeviceSynchronize());                       // (queued decodes may read the buffers that move)
            d->iv_cap = std::max(d->iv_cap, n_iv + n_iv / 2);
            d->bytes_cap = std::max(d->bytes_cap, n_bytes + n_bytes / 2);
            HM_HIP(d->own.grow(&d->d_iv, d->iv_cap * sizeof(MjdInterval)));
            HM_HIP(d->own.grow(&d->d_bytes, d->bytes_cap));
        }
    }
    if (n_host) {
        HM_HIP(d->own.host_grow(&st.coef, (size_t)d->max_run * d->blk_cap * 64 * sizeof(int16_t), hipHostMallocDefault));
        const MjdParsed *ps[64];
        const uint8_t *fs[64];
        int16_t *cs[64];
        uint32_t bad[64];
        int which[64], k = 0;
        for (int i = 0; i < nframes; i++)
            if (!d->parsed[(size_t)i].frame.dev_entropy) {
                ps[k] = &d->parsed[(size_t)i]; fs[k] = files[i]; cs[k] = st.coef + (size_t)i * d->blk_cap * 64; which[k++] = i;
            }
        if (d->workers && d->workers->threads() != d->pool) { delete d->workers; d->workers = nullptr; }      // (re-tuned)
        if (!d->workers) d->workers = new MjdPool(d->pool);
        d->workers->run(k, ps, fs, cs, bad);
        for (int j = 0; j < k; j++) d->parsed[(size_t)which[j]].frame.bad_host = bad[j];
    }
    for (int i = 0; i < nframes; i++) {
        const MjdParsed &p = d->parsed[(size_t)i];
        st.frames[i] = p.frame;
        if (p.frame.dev_entropy) {
            memcpy(st.iv + p.frame.int_off, p.intervals.data(), p.intervals.size() * sizeof(MjdInterval));
            memcpy(st.bytes + p.frame.data_off, files[i], (size_t)sizes[i]);
        }
    }
    uint64_t h2d = (uint64_t)nframes * sizeof(MjdFrame);         // every host-to-device copy below adds its size
    HM_HIP(hipMemcpyAsync(d->d_frames, st.frames, (size_t)nframes * sizeof(MjdFrame), hipMemcpyHostToDevice, s));
    if (n_iv) {
        HM_HIP(hipMemcpyAsync(d->d_iv, st.iv, n_iv * sizeof(MjdInterval), hipMemcpyHostToDevice, s));
        HM_HIP(hipMemcpyAsync(d->d_bytes, st.bytes, n_bytes, hipMemcpyHostToDevice, s));
        h2d += n_iv * sizeof(MjdInterval) + n_bytes;
    }
    for (int i = 0; i < nframes; i++) {
        const MjdFrame &f = d->parsed[(size_t)i].frame;
        if (f.dev_entropy) continue;
        const size_t at = (size_t)i * d->blk_cap * 64, count = (size_t)f.scan.n_mcu * (size_t)(f.scan.hs * f.scan.vs) * 64;
        HM_HIP(hipMemcpyAsync(d->d_coef + at, st.coef + at, count * sizeof(int16_t), hipMemcpyHostToDevice, s));
        h2d += count * sizeof(int16_t);
    }
    d->last_h2d = h2d;
    d->total_h2d += h2d;
    HM_HIP(hipEventRecord(st.copied, s));
    st.used = true;
    if (n_iv)
        hipLaunchKernelGGL(k_mjdec_entropy, dim3((unsigned)hm_cdiv((int)max_int, MJD_ENT_THREADS), (unsigned)nframes), dim3(MJD_ENT_THREADS),
                           0, s, (const MjdFrame *)d->d_frames, (const MjdInterval *)d->d_iv, (const uint8_t *)d->d_bytes, d->d_coef,
                           d->blk_cap, d->d_bad);
    MjdOut o{};
    o.frame = (uint8_t *)d_frame; o.mask = (uint8_t *)d_mask; o.shown = (uint8_t *)d_shown;
    o.frame_stride = (size_t)frame_stride; o.pitch = (size_t)pitch;
    o.W = d->W; o.H = d->H; o.threshold = threshold;
    o.words = (((uintptr_t)d_frame | (uintptr_t)d_mask | (uintptr_t)d_shown | (uintptr_t)frame_stride | (uintptr_t)pitch) & 3) == 0;
    hipLaunchKernelGGL(k_mjdec_idct, dim3((unsigned)hm_cdiv((int)max_blk, MJD_IDCT_BLOCKS), (unsigned)nframes), dim3(MJD_IDCT_THREADS), 0, s,
                       (const MjdFrame *)d->d_frames, (const int16_t *)d->d_coef, d->blk_cap, o, d->d_bad, status_words);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_mjpeg_decode(hm_mjpeg_dec_t d, const uint8_t *file, uint64_t n, uint8_t *out, int strict, uint32_t *bad)
{
    HM_ARG(d && file && out, "hm_mjpeg_decode: NULL argument");
    if (bad) *bad = 0;
    HM_HIP(hipSetDevice(d->device));
    const size_t fb = (size_t)d->W * d->H;
    HM_HIP(d->own.stream(&d->stream, false));
    HM_HIP(d->own.alloc(&d->d_out, fb));
    HM_HIP(d->own.alloc(&d->d_status, sizeof(uint32_t)));
    const uint8_t *files[1] = {file};
    const uint64_t sizes[1] = {n};
    HM_TRY(hm_mjpeg_decode_run_dev(d, 1, files, sizes, d->d_out, nullptr, nullptr, fb, (uint64_t)d->W, 0, d->d_status, d->stream));
    uint32_t status = 0;
    HM_HIP(hipMemcpyAsync(&status, d->d_status, sizeof(status), hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipMemcpyAsync(out, d->d_out, fb, hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipStreamSynchronize(d->stream));
    if (bad) *bad = status;
    HM_ARG(!strict || status == 0, "hm_mjpeg_decode: %u bad restart intervals (malformed entropy-coded data)", status);
    return HM_OK;
}
