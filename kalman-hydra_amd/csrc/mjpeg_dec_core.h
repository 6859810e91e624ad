// Motion-JPEG decoding: what the host parser, the host entropy path and the device kernel share (include/hydra_mi.h,
// "Motion-JPEG, decoding").  Plain C++ with no dependency, so that tools/mjpeg_dec_check.cpp can
// compile it as host code under the sanitizers; under hipcc the routines are __host__ __device__ and
// k_mjdec_entropy (mjpeg_dec_kernels.h) runs the very same source.
//
// Bounds.  Every byte is read through mjd_byte, which compares the position with the interval's end first; every
// coefficient is written through a block pointer the MCU counter gives (mjd_interval), never through anything the stream
// says: a run moves k, and k is compared with 63 before it indexes.  Table indices are masked to the tables' sizes.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define MJD_HD __host__ __device__
#else
#define MJD_HD
#endif

#define MJD_MAX_TABS 6                       // Huffman tables of a scan: DC and AC of up to three components

struct MjdHuff {
    uint16_t look[256];                      // the next 8 bits -> (length << 8) | symbol of a code of 1..8 bits; 0: none that short
    int32_t maxcode[17];                     // [l]: the largest code of l bits, -1 when there is none
    int32_t valoff[17];                      // [l]: a code c of l bits is vals[valoff[l] + c]
    uint8_t vals[256];
};

struct MjdScan {
    uint32_t n_mcu, ri;                      // MCUs of the frame; MCUs of an interval (n_mcu without DRI)
    int32_t mw, mh;                          // MCUs across and down
    int32_t hs, vs;                          // luma blocks of an MCU across and down (1 x 1 with one component)
    int32_t ncomp;
    uint8_t dc_slot[3], ac_slot[3], pad[2];  // per component: which of the frame's tables
};

struct MjdFrame {                            // one frame of a run, as the kernels see it
    uint32_t data_off;                       // where the file lies in the run's uploaded bytes
    uint32_t int_off, n_int;                 // its intervals in the run's table
    int32_t dev_entropy;                     // k_mjdec_entropy decodes it (else the host has sent the coefficients)
    uint32_t bad_host;                       // bad intervals the host path counted
    MjdScan scan;
    uint16_t quant[64];                      // the luma table, zigzag order
    MjdHuff tab[MJD_MAX_TABS];
};

struct MjdInterval { uint32_t start, end, first_mcu; };      // bytes [start, end) of the file

// natural index of every zigzag position
#define MJD_ZIGZAG                                                                                                      \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

struct MjdBits {
    const uint8_t *p, *end;
    uint32_t acc;                            // the low n bits are the ones not yet used
    int n;
};

// the next data byte of the interval, -1 when there is none: the range is used up, or an FF that no 00 follows (fill
// before the marker that ends the interval)
MJD_HD inline int mjd_byte(MjdBits &s)
{
    if (s.p >= s.end) return -1;
    const int b = *s.p;
    if (b != 0xFF) { s.p++; return b; }
    if (s.end - s.p >= 2 && s.p[1] == 0) { s.p += 2; return 0xFF; }
    s.p = s.end;
    return -1;
}

MJD_HD inline void mjd_fill(MjdBits &s)
{
    while (s.n <= 24) {
        const int b = mjd_byte(s);
        if (b < 0) return;
        s.acc = (s.acc << 8) | (uint32_t)b;
        s.n += 8;
    }
}

// one Huffman symbol; -1: a code of no table, or the bytes ran out
MJD_HD inline int mjd_symbol(MjdBits &s, const MjdHuff &h)
{
    mjd_fill(s);
    const uint32_t c16 = (s.n >= 16 ? s.acc >> (s.n - 16) : s.acc << (16 - s.n)) & 0xFFFFu;      // zeros past the end
    const unsigned lk = h.look[c16 >> 8];
    int len, sym;
    if (lk) {
        len = (int)(lk >> 8);
        sym = (int)(lk & 255u);
    } else {
        int32_t c = 0;
        for (len = 9; len <= 16; len++) {
            c = (int32_t)(c16 >> (16 - len));
            if (c <= h.maxcode[len]) break;
        }
        if (len > 16) return -1;
        sym = h.vals[(uint32_t)(h.valoff[len] + c) & 255u];
    }
    if (len > s.n) return -1;
    s.n -= len;
    return sym;
}

// k further bits (k <= 11) as the value they code (T.81 F.2.2.1, EXTEND); false: the bytes ran out
MJD_HD inline bool mjd_value(MjdBits &s, int k, int &v)
{
    v = 0;
    if (k == 0) return true;
    mjd_fill(s);
    if (s.n < k) return false;
    const int raw = (int)((s.acc >> (s.n - k)) & ((1u << k) - 1u));
    s.n -= k;
    v = raw < (1 << (k - 1)) ? raw - (1 << k) + 1 : raw;
    return true;
}

// one block: out[64] (all zero on entry) takes the coefficients in zigzag order, out NULL steps over the block.
// false: the block is bad.
MJD_HD inline bool mjd_block(MjdBits &s, const MjdHuff &dc, const MjdHuff &ac, uint32_t &pred, int16_t *out)
{
    int v;
    const int t = mjd_symbol(s, dc);
    if (t < 0 || t > 11) return false;
    if (!mjd_value(s, t, v)) return false;
    pred += (uint32_t)v;                                         // 32-bit wrap; the coefficient is its low 16 bits
    if (out) out[0] = (int16_t)(uint16_t)pred;
    int k = 1;
    while (k < 64) {
        const int rs = mjd_symbol(s, ac);
        if (rs < 0) return false;
        const int r = rs >> 4, size = rs & 15;
        if (size == 0) {
            if (r != 15) break;                                  // EOB
            k += 16;                                             // ZRL: a coefficient must follow
            if (k > 63) return false;
            continue;
        }
        if (size > 10) return false;
        k += r;
        if (k > 63) return false;
        if (!mjd_value(s, size, v)) return false;
        if (out) out[k] = (int16_t)v;
        k++;
    }
    return true;
}

typedef uint64_t __attribute__((may_alias)) mjd_u64_alias;      // wide stores into int16 blocks that mjd_block writes next

MJD_HD inline void mjd_zero(int16_t *o)                        // (blocks are 8-byte aligned)
{
    mjd_u64_alias *q = (mjd_u64_alias *)o;
    for (int i = 0; i < 16; i++) q[i] = 0;
}

// One interval: MCUs first_mcu .. min(first_mcu + ri, n_mcu) - 1, the luma blocks of MCU m to coef[(m lb + j) 64], lb = hs vs.
// From the first bad block on everything is zero.  Returns 1 when the interval is bad.
MJD_HD inline int mjd_interval(const MjdScan &g, const MjdHuff *tab, const uint8_t *file, MjdInterval iv, int16_t *coef)
{
    const uint32_t lb = (uint32_t)(g.hs * g.vs);
    const uint32_t left = g.n_mcu - (iv.first_mcu < g.n_mcu ? iv.first_mcu : g.n_mcu);
    const uint32_t count = g.ri < left ? g.ri : left;
    MjdBits s{file + iv.start, file + iv.end, 0u, 0};
    const MjdHuff &ydc = tab[g.dc_slot[0]], &yac = tab[g.ac_slot[0]];
    const MjdHuff &bdc = tab[g.dc_slot[1]], &bac = tab[g.ac_slot[1]];
    const MjdHuff &rdc = tab[g.dc_slot[2]], &rac = tab[g.ac_slot[2]];
    uint32_t py = 0, pb = 0, pr = 0;
    bool bad = false;
    for (uint32_t i = 0; i < count; i++) {
        const size_t m = (size_t)iv.first_mcu + i;
        for (uint32_t j = 0; j < lb; j++) {
            int16_t *o = coef + (m * lb + j) * 64;
            mjd_zero(o);
            if (!bad && !mjd_block(s, ydc, yac, py, o)) {
                bad = true;
                mjd_zero(o);
            }
        }
        if (g.ncomp == 3) {
            if (!bad && !mjd_block(s, bdc, bac, pb, nullptr)) bad = true;
            if (!bad && !mjd_block(s, rdc, rac, pr, nullptr)) bad = true;
        }
    }
    return bad ? 1 : 0;
}

// ---- the host side (mjpeg_dec.cpp) ----------------------------------------------------------------------------------
#include <vector>

struct MjdParsed {
    int W = 0, H = 0, components = 0, hs = 1, vs = 1, ri = 0;       // ri: the DRI value, 0 without
    MjdFrame frame;                                               // scan, quant, tables; int_off 0
    std::vector<MjdInterval> intervals;
};

// Headers and the marker scan of one file.  HM_OK, or HM_ERR_ARG with the marker or field in hm_last_error.
int mjd_parse(const uint8_t *file, uint64_t n, MjdParsed *out);
// All intervals of a parsed file on this thread: coef takes n_mcu hs vs blocks of 64.  Returns the number of bad intervals.
uint32_t mjd_entropy_host(const MjdParsed &p, const uint8_t *file, int16_t *coef);
// Several files at once on a fixed set of host threads (1..16, the thread that calls run among them), a file at a time
// each; bad[i]: bad intervals of file i.  The threads are started once and sleep between runs.
class MjdPool {
public:
    explicit MjdPool(int threads);
    ~MjdPool();
    MjdPool(const MjdPool &) = delete;
    MjdPool &operator=(const MjdPool &) = delete;
    int threads() const { return n; }
    void run(int count, const MjdParsed *const *parsed, const uint8_t *const *files, int16_t *const *coef, uint32_t *bad);
private:
    struct Impl;
    Impl *m;
    int n;
};
