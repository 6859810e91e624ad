// The library's video container: uncompressed 24-bit AVI (RIFF 'AVI ', one 'DIB ' video stream), continued past the
// RIFF size limit in OpenDML 'AVIX' RIFFs ("OpenDML AVI File Format Extensions", Matrox, 1996: an 'indx' super index
// in the stream header list, one 'ix00' standard index per RIFF, the total frame count in 'odml'/'dmlh').  The first
// RIFF also carries the legacy 'idx1' index.  Replaces the cv::VideoWriter of the reference's flow tool
// (src/optical_flow_ext.cpp:351-358) and gives run_kalmanfilter.py's fn_out its video (reference run_kalmanfilter.py:43-44).
// Host code only: the one place the format is known; the Python package and the native flow tool both call it.
// hm_avi_open_codec(HM_AVI_MJPG) writes the same container around compressed chunks ('MJPG' handler and biCompression,
// '00dc' chunks of any length padded to even, their sizes in both indexes, the buffer-size fields patched at close).
#include "hm_common.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

const int SUPER_ENTRIES = 256;          // RIFFs the super index can name: 256 GiB at the default limit

struct Avi {
    FILE *f = nullptr;
    int W = 0, H = 0, fps = 20;
    uint32_t stride = 0, frame_bytes = 0;
    uint64_t limit = 0;
    long long total = 0;                // frames written
    // positions (bytes from the start of the file) of the fields patched at the end
    long long avih_frames = 0, strh_length = 0, indx_pos = 0, dmlh_frames = 0;
    // the RIFF being written
    long long riff_pos = 0, movi_pos = 0;
    bool first = true;
    std::vector<long long> chunks;      // header positions of this RIFF's frame chunks
    bool mjpg = false;                  // compressed chunks: their sizes, the largest of the file, the fields it patches
    std::vector<uint32_t> sizes;
    uint32_t largest = 0;
    long long avih_rate = 0, avih_buffer = 0, strh_buffer = 0;
    struct Super { long long off; uint32_t size, duration; };
    std::vector<Super> supers;
    std::vector<uint8_t> row;
    bool failed = false;
};

void put(Avi &a, const void *p, size_t n)
{
    if (fwrite(p, 1, n, a.f) != n) a.failed = true;
}
void u32(Avi &a, uint32_t v) { uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)}; put(a, b, 4); }
void u16(Avi &a, uint16_t v) { uint8_t b[2] = {(uint8_t)v, (uint8_t)(v >> 8)}; put(a, b, 2); }
void u8(Avi &a, uint8_t v) { put(a, &v, 1); }
void u64(Avi &a, uint64_t v) { u32(a, (uint32_t)v); u32(a, (uint32_t)(v >> 32)); }
void cc(Avi &a, const char *s) { put(a, s, 4); }
long long tell(Avi &a) { return (long long)ftello(a.f); }
void seek(Avi &a, long long pos)
{
    if (fseeko(a.f, (off_t)pos, SEEK_SET) != 0) a.failed = true;
}
void patch32(Avi &a, long long pos, uint32_t v)
{
    const long long here = tell(a);
    seek(a, pos);
    u32(a, v);
    seek(a, here);
}

// 'RIFF' size type 'LIST' size 'movi' -> the RIFF's position
void open_riff(Avi &a, const char *type, bool headers)
{
    a.riff_pos = tell(a);
    cc(a, "RIFF"); u32(a, 0); cc(a, type);
    if (headers) {
        const uint32_t idx_bytes = 24 + 16 * SUPER_ENTRIES;
        const uint32_t strl = 4 + (8 + 56) + (8 + 40) + (8 + idx_bytes);
        const uint32_t odml = 4 + 8 + 248;
        cc(a, "LIST"); u32(a, 4 + (8 + 56) + (8 + strl) + (8 + odml)); cc(a, "hdrl");
        cc(a, "avih"); u32(a, 56);
        u32(a, (uint32_t)(1000000 / a.fps));            // dwMicroSecPerFrame
        a.avih_rate = tell(a);
        u32(a, a.frame_bytes * (uint32_t)a.fps);        // dwMaxBytesPerSec
        u32(a, 0);                                      // dwPaddingGranularity
        u32(a, 0x10);                                   // dwFlags: AVIF_HASINDEX
        a.avih_frames = tell(a); u32(a, 0);             // dwTotalFrames (of this RIFF)
        u32(a, 0); u32(a, 1);                           // dwInitialFrames, dwStreams
        a.avih_buffer = tell(a);
        u32(a, a.frame_bytes + 8);                      // dwSuggestedBufferSize
        u32(a, (uint32_t)a.W); u32(a, (uint32_t)a.H);
        for (int i = 0; i < 4; i++) u32(a, 0);
        cc(a, "LIST"); u32(a, strl); cc(a, "strl");
        cc(a, "strh"); u32(a, 56);
        cc(a, "vids"); cc(a, a.mjpg ? "MJPG" : "DIB ");
        u32(a, 0); u16(a, 0); u16(a, 0); u32(a, 0);     // dwFlags, wPriority, wLanguage, dwInitialFrames
        u32(a, 1); u32(a, (uint32_t)a.fps); u32(a, 0);  // dwScale, dwRate, dwStart
        a.strh_length = tell(a); u32(a, 0);             // dwLength (all frames)
        a.strh_buffer = tell(a);
        u32(a, a.frame_bytes + 8); u32(a, 0xFFFFFFFFu); u32(a, a.mjpg ? 0 : a.frame_bytes);   // buffer size, quality, sample size
        u16(a, 0); u16(a, 0); u16(a, (uint16_t)a.W); u16(a, (uint16_t)a.H);     // rcFrame
        cc(a, "strf"); u32(a, 40);                      // BITMAPINFOHEADER, positive height: rows bottom-up
        u32(a, 40); u32(a, (uint32_t)a.W); u32(a, (uint32_t)a.H); u16(a, 1); u16(a, 24);
        if (a.mjpg) cc(a, "MJPG"); else u32(a, 0);      // biCompression
        u32(a, a.frame_bytes); u32(a, 0); u32(a, 0); u32(a, 0); u32(a, 0);
        a.indx_pos = tell(a);
        cc(a, "indx"); u32(a, idx_bytes);
        u16(a, 4); u8(a, 0); u8(a, 0);                  // wLongsPerEntry, bIndexSubType, bIndexType = AVI_INDEX_OF_INDEXES
        u32(a, 0); cc(a, a.mjpg ? "00dc" : "00db"); u32(a, 0); u32(a, 0); u32(a, 0);
        std::vector<uint8_t> zero(16 * SUPER_ENTRIES, 0);
        put(a, zero.data(), zero.size());
        cc(a, "LIST"); u32(a, odml); cc(a, "odml");
        cc(a, "dmlh"); u32(a, 248);
        a.dmlh_frames = tell(a); u32(a, 0);
        std::vector<uint8_t> z2(244, 0);
        put(a, z2.data(), z2.size());
    }
    a.movi_pos = tell(a);
    cc(a, "LIST"); u32(a, 0); cc(a, "movi");
    a.chunks.clear();
    a.sizes.clear();
}

// the standard index of the RIFF (inside its 'movi'), its sizes, and for the first RIFF 'idx1'
void close_riff(Avi &a)
{
    const uint32_t k = (uint32_t)a.chunks.size();
    const long long ix = tell(a);
    const uint64_t base = (uint64_t)a.movi_pos;
    cc(a, "ix00"); u32(a, 24 + 8 * k);
    u16(a, 2); u8(a, 0); u8(a, 1);                      // wLongsPerEntry, bIndexSubType, bIndexType = AVI_INDEX_OF_CHUNKS
    const char *id = a.mjpg ? "00dc" : "00db";
    u32(a, k); cc(a, id); u64(a, base); u32(a, 0);
    for (uint32_t i = 0; i < k; i++) {
        u32(a, (uint32_t)(a.chunks[i] + 8 - (long long)base));
        u32(a, a.mjpg ? a.sizes[i] : a.frame_bytes);
    }
    a.supers.push_back({ix, 32 + 8 * k, k});
    const long long end_movi = tell(a);
    patch32(a, a.movi_pos + 4, (uint32_t)(end_movi - a.movi_pos - 8));
    if (a.first) {
        patch32(a, a.avih_frames, k);
        cc(a, "idx1"); u32(a, 16 * k);
        for (uint32_t i = 0; i < k; i++) {
            cc(a, id); u32(a, 0x10);                    // AVIIF_KEYFRAME
            u32(a, (uint32_t)(a.chunks[i] - (a.movi_pos + 8))); u32(a, a.mjpg ? a.sizes[i] : a.frame_bytes);
        }
    }
    const long long end = tell(a);
    patch32(a, a.riff_pos + 4, (uint32_t)(end - a.riff_pos - 8));
    a.first = false;
}

int fail(Avi *a, const char *what)
{
    hm_set_error("AVI %s failed (%s)", what, a->f && ferror(a->f) ? "write error" : "file error");
    return HM_ERR_ARG;
}

}  // namespace

static int avi_open(const char *who, const char *path, int W, int H, int fps, uint64_t riff_limit, bool mjpg, hm_avi_t *out)
{
    HM_ARG(out, "%s: out is NULL", who);
    *out = nullptr;
    HM_ARG(path, "%s: path is NULL", who);
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "%s: frame size %dx%d outside 1..32767", who, W, H);
    HM_ARG(fps >= 1 && fps <= 1000, "%s: %d frames/s outside 1..1000", who, fps);
    if (riff_limit == 0) riff_limit = 1ull << 30;
    const uint32_t stride = ((uint32_t)W * 3 + 3) & ~3u;
    HM_ARG((uint64_t)stride * H < (1ull << 31), "%s: a frame of %dx%d is too large", who, W, H);
    HM_ARG(riff_limit < (1ull << 32), "%s: a RIFF holds at most 4 GiB", who);
    // (compressed chunks: the headers and the indexes of a chunk; a chunk larger than the limit gets a RIFF of its own)
    HM_ARG(!mjpg || riff_limit >= 16384, "%s: a RIFF limit of %llu bytes does not hold the headers", who,
           (unsigned long long)riff_limit);
    HM_ARG(mjpg || riff_limit >= 2ull * (stride * H + 8) + 16384, "%s: a RIFF limit of %llu bytes does not hold two frames", who,
           (unsigned long long)riff_limit);
    Avi *a = new Avi();
    a->mjpg = mjpg;
    a->W = W; a->H = H; a->fps = fps;
    a->stride = stride;
    a->frame_bytes = stride * (uint32_t)H;
    a->limit = riff_limit;
    a->row.assign(a->stride, 0);
    a->f = fopen(path, "wb");
    if (!a->f) {
        hm_set_error("%s: cannot open %s for writing", who, path);
        delete a;
        return HM_ERR_ARG;
    }
    open_riff(*a, "AVI ", true);
    if (a->failed) {
        const int rc = fail(a, "header write");
        fclose(a->f);
        delete a;
        return rc;
    }
    *out = (hm_avi_t)a;
    return HM_OK;
}

extern "C" int hm_avi_open(const char *path, int W, int H, int fps, uint64_t riff_limit, hm_avi_t *out)
{
    return avi_open("hm_avi_open", path, W, H, fps, riff_limit, false, out);
}

extern "C" int hm_avi_open_codec(const char *path, int W, int H, int fps, uint64_t riff_limit, int codec, hm_avi_t *out)
{
    if (out) *out = nullptr;
    HM_ARG(codec == HM_AVI_RAW || codec == HM_AVI_MJPG, "hm_avi_open_codec: codec %d is neither HM_AVI_RAW (0) nor HM_AVI_MJPG (1)",
           codec);
    return avi_open("hm_avi_open_codec", path, W, H, fps, riff_limit, codec == HM_AVI_MJPG, out);
}

extern "C" int hm_avi_write_chunk(hm_avi_t h, const uint8_t *data, uint64_t n)
{
    Avi *a = (Avi *)h;
    HM_ARG(a && data, "hm_avi_write_chunk: NULL argument");
    HM_ARG(a->mjpg, "hm_avi_write_chunk: the file was opened for uncompressed frames (hm_avi_write)");
    HM_ARG(n >= 1 && n < (1ull << 31), "hm_avi_write_chunk: a chunk of %llu bytes, outside 1..2^31-1", (unsigned long long)n);
    HM_ARG(!a->failed, "hm_avi_write_chunk: an earlier write of this file failed");
    const long long k = (long long)a->chunks.size();
    const long long padded = (long long)(n + (n & 1));
    // as hm_avi_write, with the bytes this chunk really takes
    const long long need = tell(*a) + 8 + padded + 32 + 8 * (k + 1) + (a->first ? 8 + 16 * (k + 1) : 0) - a->riff_pos;
    if (k > 0 && (uint64_t)need > a->limit) {
        HM_ARG((int)a->supers.size() + 1 < SUPER_ENTRIES, "hm_avi_write_chunk: more than %d RIFFs", SUPER_ENTRIES);
        close_riff(*a);
        open_riff(*a, "AVIX", false);
    }
    a->chunks.push_back(tell(*a));
    a->sizes.push_back((uint32_t)n);
    if ((uint32_t)n > a->largest) a->largest = (uint32_t)n;
    cc(*a, "00dc"); u32(*a, (uint32_t)n);
    put(*a, data, (size_t)n);
    if (n & 1) u8(*a, 0);
    a->total++;
    if (a->failed) return fail(a, "chunk write");
    return HM_OK;
}

extern "C" int hm_avi_write(hm_avi_t h, const uint8_t *bgr)
{
    Avi *a = (Avi *)h;
    HM_ARG(a && bgr, "hm_avi_write: NULL argument");
    HM_ARG(!a->mjpg, "hm_avi_write: the file was opened for compressed chunks (hm_avi_write_chunk)");
    HM_ARG(!a->failed, "hm_avi_write: an earlier write of this file failed");
    const long long k = (long long)a->chunks.size();
    // this frame, the RIFF's standard index and (first RIFF) idx1 must fit in the limit, else the next RIFF
    const long long need = tell(*a) + 8 + a->frame_bytes + 32 + 8 * (k + 1) + (a->first ? 8 + 16 * (k + 1) : 0) - a->riff_pos;
    if (k > 0 && (uint64_t)need > a->limit) {
        HM_ARG((int)a->supers.size() + 1 < SUPER_ENTRIES, "hm_avi_write: more than %d RIFFs", SUPER_ENTRIES);
        close_riff(*a);
        open_riff(*a, "AVIX", false);
    }
    a->chunks.push_back(tell(*a));
    cc(*a, "00db"); u32(*a, a->frame_bytes);
    const size_t w3 = (size_t)a->W * 3;
    for (int r = a->H - 1; r >= 0; r--) {        // DIB rows bottom-up, padded to 4 bytes
        memcpy(a->row.data(), bgr + (size_t)r * w3, w3);
        put(*a, a->row.data(), a->stride);
    }
    a->total++;
    if (a->failed) return fail(a, "frame write");
    return HM_OK;
}

extern "C" int hm_avi_close(hm_avi_t h)
{
    Avi *a = (Avi *)h;
    if (!a) return HM_OK;
    close_riff(*a);
    patch32(*a, a->strh_length, (uint32_t)a->total);
    patch32(*a, a->dmlh_frames, (uint32_t)a->total);
    if (a->mjpg) {
        patch32(*a, a->avih_rate, (uint32_t)std::min<uint64_t>((uint64_t)a->largest * (uint32_t)a->fps, 0xFFFFFFFFull));
        patch32(*a, a->avih_buffer, a->largest + 8);
        patch32(*a, a->strh_buffer, a->largest + 8);
    }
    patch32(*a, a->indx_pos + 12, (uint32_t)a->supers.size());
    const long long here = tell(*a);
    seek(*a, a->indx_pos + 32);
    for (const auto &s : a->supers) { u64(*a, (uint64_t)s.off); u32(*a, s.size); u32(*a, s.duration); }
    seek(*a, here);
    const bool bad = a->failed || fclose(a->f) != 0;
    a->f = nullptr;
    int rc = HM_OK;
    if (bad) { hm_set_error("hm_avi_close: writing the AVI file failed"); rc = HM_ERR_ARG; }
    delete a;
    return rc;
}
