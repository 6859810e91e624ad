// Baseline JPEG encoder of the video writer (include/hydra_mi.h, "Motion-JPEG").  Compiled by
// mjpeg.hip alone.  Five launches per frame, all on the caller's stream:
//   k_mjpeg_blocks   a workgroup stages the samples of 256 (grey) or 85 (colour) MCUs in LDS, every pixel loaded and
//                    converted once; then one thread per 8x8 block of one component: DCT, quantisation, zigzag -> 64
//                    int16 and the bit length of the block's AC code
//   k_mjpeg_emit     one workgroup per restart interval, a thread per block (in turns of 1024 when there are more): scan
//                    of the blocks' bit lengths (the DC difference is known here), then every block ORs its code into the
//                    interval's area of the bit buffer
//   k_mjpeg_count    one workgroup per interval: the FF bytes of its area -> the interval's size in the stream
//   k_mjpeg_offsets  one workgroup: scan of the sizes -> every interval's offset and the stream's size
//   k_mjpeg_pack     one workgroup per interval: copies its bytes to the stream with FF 00 stuffing and the marker that
//                    ends it, clears the words it has read (the bit buffer is all zero between frames), and writes the
//                    size word.  A stream larger than `cap` is not written at all.
// An interval's area holds 208 bytes a block (64 coefficients of at most 26 bits), so no code can leave it; the stream is
// sized before a byte of it is written.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define MJ_THREADS 256
#define MJ_EMIT_MAX 1024                     // k_mjpeg_emit: a thread per block of the interval, up to this many at a time
#define MJ_BLOCK_WORDS 52                    // 64 * 26 bits = 208 bytes

struct MjTables {                            // device copy of an encoder's tables
    uint16_t quant[2][64];                   // zigzag order; [0] Y / grey, [1] Cb Cr
    uint16_t dc_code[2][12];
    uint8_t dc_len[2][12];
    uint16_t ac_code[2][256];                // by (run << 4) | size
    uint8_t ac_len[2][256];
};

struct MjGeo {
    int W, H, C;                             // frame, components
    int bw, bh;                              // blocks across and down
    int ri;                                  // MCUs in a restart interval
    int n_mcu, n_int;                        // MCUs of the frame, restart intervals
};

// rint(4096 cos(k pi / 16)), k = 0 .. 31
__device__ __host__ constexpr int mj_cos16(int k)
{
    constexpr int q[9] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0};
    k &= 31;
    if (k > 16) k = 32 - k;
    return k <= 8 ? q[k] : -q[16 - k];
}
// the DCT table: rint(2^13 c(u)/2 cos((2x+1) u pi / 16))
__device__ __host__ constexpr int mj_dct(int u, int x) { return u == 0 ? 2896 : mj_cos16((2 * x + 1) * u); }

// natural index -> zigzag position
__device__ __host__ constexpr int mj_zigzag_pos(int natural)
{
    constexpr uint8_t zz[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43,
                                9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return zz[natural];
}

#define MJ_ROW_SHIFT 11                      // 13 - 2: two fractional bits between the passes
#define MJ_COL_SHIFT 12                      // 13 + 2 - 3: the coefficient keeps three fractional bits for the quantiser

__device__ inline int mj_bitlen(int v) { return 32 - __clz(v); }     // v >= 0; 0 -> 0

// the exclusive scan of one value per thread over the workgroup (whole waves, at most 16 of them): a shuffle scan
// inside each wave, the waves' sums scanned by the first wave through `lds` (16 words); *total: the sum
__device__ inline unsigned mj_scan(unsigned v, unsigned *lds, unsigned *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        unsigned w = lane < nw ? lds[lane] : 0u;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const unsigned y = __shfl_up(w, d, 64);
            if (lane >= d) w += y;
        }
        if (lane < nw) lds[lane] = w;
    }
    __syncthreads();
    const unsigned before = wave ? lds[wave - 1] : 0u;
    *total = lds[nw - 1];
    __syncthreads();
    return before + x - v;
}

// coefficient k of a block held as eight 16-byte loads (k a constant once the loop around it is unrolled)
__device__ inline int mj_coef(const uint4 (&raw)[8], int k)
{
    const uint4 q = raw[k >> 3];
    const unsigned w = (k & 6) == 0 ? q.x : (k & 6) == 2 ? q.y : (k & 6) == 4 ? q.z : q.w;
    return (int)(int16_t)((k & 1) ? (w >> 16) : (w & 0xFFFFu));
}

#define MJ_STAGE_STRIDE 68                   // bytes a block's 64 samples take in LDS: 17 words, so that the threads' word
                                             // reads fall into different banks

// signed byte i of a word
__device__ inline int mj_s8(int w, int i) { return (int)((unsigned)w << (24 - 8 * i)) >> 24; }

// MCUs a workgroup of k_mjpeg_blocks takes: a thread per block of a component
__device__ __host__ constexpr int mj_blocks_mcus(int C) { return MJ_THREADS / C; }

__global__ __launch_bounds__(MJ_THREADS) void k_mjpeg_blocks(MjGeo g, const MjTables *__restrict__ tab,
                                                             const uint8_t *__restrict__ frame, int16_t *__restrict__ coef,
                                                             uint16_t *__restrict__ acbits)
{
    // the samples of the workgroup's blocks, less 128: block (MCU, component) at (MCU * C + component) * MJ_STAGE_STRIDE.
    // Every pixel is loaded and converted once, by threads that walk the rows of a block side by side.
    __shared__ __attribute__((aligned(16))) int8_t stage[MJ_THREADS * MJ_STAGE_STRIDE];
    const int m0 = blockIdx.x * mj_blocks_mcus(g.C);
    const int nm = min(mj_blocks_mcus(g.C), g.n_mcu - m0);
    for (int p = threadIdx.x; p < nm * 64; p += MJ_THREADS) {
        const int ml = p >> 6, y = (p >> 3) & 7, x = p & 7;
        const int mcu = m0 + ml;
        const int bx = mcu % g.bw, by = mcu / g.bw;
        const int py = min(by * 8 + y, g.H - 1), px = min(bx * 8 + x, g.W - 1);
        const uint8_t *q = frame + ((size_t)py * g.W + px) * g.C;
        int8_t *s = stage + ml * g.C * MJ_STAGE_STRIDE + (y * 8 + x);
        if (g.C == 1) {
            s[0] = (int8_t)((int)q[0] - 128);
        } else {
            const int B = q[0], G = q[1], R = q[2];
            s[0] = (int8_t)(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128);
            s[MJ_STAGE_STRIDE] = (int8_t)(((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128);
            s[2 * MJ_STAGE_STRIDE] = (int8_t)(((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x >= nm * g.C) return;
    const int j = m0 * g.C + (int)threadIdx.x;
    const int set = (j % g.C) ? 1 : 0;
    const int *mine = (const int *)(stage + threadIdx.x * MJ_STAGE_STRIDE);
    int tmp[64];
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const int w0 = mine[2 * y], w1 = mine[2 * y + 1];
        const int s[8] = {mj_s8(w0, 0), mj_s8(w0, 1), mj_s8(w0, 2), mj_s8(w0, 3),
                          mj_s8(w1, 0), mj_s8(w1, 1), mj_s8(w1, 2), mj_s8(w1, 3)};
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int a = 1 << (MJ_ROW_SHIFT - 1);
#pragma unroll
            for (int x = 0; x < 8; x++) a += mj_dct(u, x) * s[x];
            tmp[y * 8 + u] = a >> MJ_ROW_SHIFT;
        }
    }
    int q[64];                               // quantised, zigzag order
#pragma unroll
    for (int u = 0; u < 8; u++) {
#pragma unroll
        for (int v = 0; v < 8; v++) {
            int a = 1 << (MJ_COL_SHIFT - 1);
#pragma unroll
            for (int y = 0; y < 8; y++) a += mj_dct(v, y) * tmp[y * 8 + u];
            const int c = a >> MJ_COL_SHIFT;             // 8 x the coefficient
            const int k = mj_zigzag_pos(v * 8 + u);
            const int qv = tab->quant[set][k];
            const int m = (2 * abs(c) + 8 * qv) / (16 * qv);
            q[k] = c < 0 ? -m : m;
        }
    }
    int16_t *o = coef + (size_t)j * 64;
    unsigned bits = 0;
    int run = 0;
    o[0] = (int16_t)q[0];
#pragma unroll
    for (int k = 1; k < 64; k++) {
        o[k] = (int16_t)q[k];
        if (q[k] == 0) {
            run++;
        } else {
            bits += (unsigned)tab->ac_len[set][0xF0] * (unsigned)(run >> 4);     // ZRL for every 16 zeros
            const int size = mj_bitlen(abs(q[k]));
            bits += tab->ac_len[set][((run & 15) << 4) | size] + size;
            run = 0;
        }
    }
    if (run > 0) bits += tab->ac_len[set][0];
    acbits[j] = (uint16_t)bits;
}

// the bit writer of one block: bits go out most significant first, as whole 32-bit words ORed into the area
struct MjBits {
    unsigned *words;                         // the interval's area
    unsigned w;                              // the word being filled
    unsigned long long acc;
    int n;                                   // bits of acc not yet written (those before the block's start are zero)
    __device__ void put(unsigned code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const unsigned v = (unsigned)(acc >> (n - 32));
            atomicOr(words + w, __builtin_bswap32(v));
            w++;
            n -= 32;
        }
    }
    __device__ void flush()
    {
        if (n > 0) atomicOr(words + w, __builtin_bswap32((unsigned)(acc << (32 - n))));
    }
};

__global__ __launch_bounds__(MJ_EMIT_MAX) void k_mjpeg_emit(MjGeo g, const MjTables *__restrict__ tab,
                                                           const int16_t *__restrict__ coef,
                                                           const uint16_t *__restrict__ acbits, unsigned *__restrict__ bitbuf,
                                                           unsigned *__restrict__ ibits)
{
    __shared__ unsigned lds[16];
    const int i = blockIdx.x;
    const int mcu0 = i * g.ri;
    const int nblk = min(g.ri, g.n_mcu - mcu0) * g.C;
    const size_t j0 = (size_t)mcu0 * g.C;
    unsigned *area = bitbuf + j0 * MJ_BLOCK_WORDS;
    unsigned carry = 0;
    for (int base = 0; base < nblk; base += (int)blockDim.x) {
        const int l = base + (int)threadIdx.x;
        const bool on = l < nblk;
        const size_t j = j0 + (on ? l : 0);
        const int set = (int)(j % g.C) ? 1 : 0;
        const int16_t *c = coef + j * 64;
        uint4 raw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) raw[i] = on ? ((const uint4 *)c)[i] : make_uint4(0, 0, 0, 0);
        int diff = 0, cat = 0;
        unsigned len = 0;
        if (on) {
            diff = mj_coef(raw, 0) - (l >= g.C ? c[-64 * g.C] : 0);
            cat = mj_bitlen(abs(diff));
            len = tab->dc_len[set][cat] + cat + acbits[j];
        }
        unsigned total;
        const unsigned off = carry + mj_scan(len, lds, &total);
        carry += total;
        if (!on) continue;
        MjBits b;
        b.words = area;
        b.w = off >> 5;
        b.acc = 0;
        b.n = (int)(off & 31);
        b.put(((unsigned)tab->dc_code[set][cat] << cat) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1)),
              tab->dc_len[set][cat] + cat);
        int run = 0;
#pragma unroll
        for (int k = 1; k < 64; k++) {
            const int v = mj_coef(raw, k);
            if (v == 0) {
                run++;
                continue;
            }
            for (; run > 15; run -= 16) b.put(tab->ac_code[set][0xF0], tab->ac_len[set][0xF0]);
            const int size = mj_bitlen(abs(v));
            const int sym = (run << 4) | size;
            b.put(((unsigned)tab->ac_code[set][sym] << size) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1)),
                  tab->ac_len[set][sym] + size);
            run = 0;
        }
        if (run > 0) b.put(tab->ac_code[set][0], tab->ac_len[set][0]);
        if (l == nblk - 1) {                 // the interval ends on a byte: 1-bits
            const int pad = (int)((0u - (off + len)) & 7u);
            if (pad) b.put((1u << pad) - 1, pad);
            ibits[i] = off + len + pad;
        }
        b.flush();
    }
}

__device__ inline unsigned mj_ff_bytes(unsigned v)
{
    return ((v & 0xFFu) == 0xFFu) + ((v & 0xFF00u) == 0xFF00u) + ((v & 0xFF0000u) == 0xFF0000u) + ((v >> 24) == 0xFFu);
}

__global__ __launch_bounds__(MJ_THREADS) void k_mjpeg_count(MjGeo g, const unsigned *__restrict__ bitbuf,
                                                            const unsigned *__restrict__ ibits, unsigned *__restrict__ isize)
{
    __shared__ unsigned ff;
    const int i = blockIdx.x;
    if (threadIdx.x == 0) ff = 0;
    __syncthreads();
    const unsigned *area = bitbuf + (size_t)i * g.ri * g.C * MJ_BLOCK_WORDS;
    const unsigned nbytes = ibits[i] >> 3, nwords = (nbytes + 3) >> 2;
    unsigned n = 0;
    for (unsigned w = threadIdx.x; w < nwords; w += MJ_THREADS) n += mj_ff_bytes(area[w]);   // (past nbytes: zero)
    if (n) atomicAdd(&ff, n);
    __syncthreads();
    if (threadIdx.x == 0) isize[i] = nbytes + ff + 2;
}

__global__ __launch_bounds__(MJ_THREADS) void k_mjpeg_offsets(MjGeo g, const unsigned *__restrict__ isize,
                                                              unsigned *__restrict__ ioff)
{
    __shared__ unsigned lds[16];
    unsigned carry = 0;
    for (int base = 0; base < g.n_int; base += MJ_THREADS) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < g.n_int ? isize[i] : 0u;
        unsigned total;
        const unsigned off = carry + mj_scan(v, lds, &total);
        carry += total;
        if (i < g.n_int) ioff[i] = off;
    }
    if (threadIdx.x == 0) ioff[g.n_int] = carry;                     // the stream's size
}

__global__ __launch_bounds__(MJ_THREADS) void k_mjpeg_pack(MjGeo g, unsigned *__restrict__ bitbuf,
                                                           const unsigned *__restrict__ ibits, const unsigned *__restrict__ isize,
                                                           const unsigned *__restrict__ ioff, uint8_t *__restrict__ out,
                                                           unsigned cap, unsigned *__restrict__ size_word)
{
    __shared__ unsigned lds[16];
    const int i = blockIdx.x;
    const unsigned size = ioff[g.n_int];
    const bool fits = size <= cap;
    if (i == 0 && threadIdx.x == 0) *size_word = size;
    unsigned *area = bitbuf + (size_t)i * g.ri * g.C * MJ_BLOCK_WORDS;
    const unsigned nbytes = ibits[i] >> 3, nwords = (nbytes + 3) >> 2;
    uint8_t *o = out + ioff[i];
    unsigned carry = 0;
    for (unsigned base = 0; base < nwords; base += MJ_THREADS) {
        const unsigned w = base + threadIdx.x;
        unsigned v = 0, valid = 0;
        if (w < nwords) {
            v = area[w];
            area[w] = 0;
            valid = min(4u, nbytes - 4 * w);
        }
        unsigned total;
        unsigned pos = carry + mj_scan(valid + mj_ff_bytes(v), lds, &total);
        carry += total;
        if (fits) {
            for (unsigned k = 0; k < valid; k++) {
                const uint8_t b = (uint8_t)(v >> (8 * k));
                o[pos++] = b;
                if (b == 0xFF) o[pos++] = 0;
            }
        }
    }
    if (fits && threadIdx.x == 0) {          // RSTm between intervals, EOI after the last
        o[isize[i] - 2] = 0xFF;
        o[isize[i] - 1] = i == g.n_int - 1 ? 0xD9 : (uint8_t)(0xD0 + (i & 7));
    }
}
