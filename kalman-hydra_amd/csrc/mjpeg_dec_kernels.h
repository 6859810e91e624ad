// Motion-JPEG decoding on the device (include/hydra_mi.h, "Motion-JPEG, decoding").
//
//   k_mjdec_entropy  grid (ceil(intervals / 64), frames of the run) x 64 threads: a thread decodes one restart interval
//                    of its frame with mjd_interval (mjpeg_dec_core.h, the host path's own source) into the frame's
//                    coefficient blocks.  The frame's Huffman tables are copied to LDS first.  Frames whose
//                    coefficients the host sent are stepped over.  A bad interval adds one to the frame's counter.
//   k_mjdec_idct     grid (ceil(luma blocks / 32), frames) x 256 threads: 8 threads per block.  Dequantise into LDS in
//                    natural order, a thread per column (pass 1), a thread per row (pass 2), range limit, and the row's
//                    8 bytes to the grey frame and, when asked, to the mask and the shown frame, cropped to W x H.  The
//                    first thread of a frame publishes the frame's status word and puts its counter back to zero.
//
// Integers only, all sums in uint32_t (two's-complement wrap): libjpeg's "islow" inverse DCT, CONST_BITS 13, PASS1_BITS 2.
// Vector stores only: uint32_t pairs where base, strides and pitch are multiples of 4 (the host checks), else bytes.
#pragma once
#include "mjpeg_dec_core.h"

#define MJD_ENT_THREADS 64
#define MJD_IDCT_THREADS 256
#define MJD_IDCT_BLOCKS 32                   // blocks of 8 x 8 a workgroup of k_mjdec_idct transforms

struct MjdOut {
    uint8_t *frame, *mask, *shown;           // mask and shown may be NULL
    size_t frame_stride, pitch;              // bytes from a frame of the run to the next, from a row to the next
    int W, H;
    int threshold;                           // mask = frame > threshold
    int words;                               // every address of a row's 8 bytes is a multiple of 4
};

static __constant__ uint8_t MJD_NATURAL[64] = MJD_ZIGZAG;

__global__ __launch_bounds__(MJD_ENT_THREADS) void k_mjdec_entropy(const MjdFrame *__restrict__ frames,
                                                                     const MjdInterval *__restrict__ intervals,
                                                                     const uint8_t *__restrict__ bytes, int16_t *__restrict__ coef,
                                                                     size_t blk_cap, unsigned *__restrict__ bad)
{
    __shared__ MjdHuff tab[MJD_MAX_TABS];
    const MjdFrame &f = frames[blockIdx.y];
    if (!f.dev_entropy || blockIdx.x * MJD_ENT_THREADS >= f.n_int) return;         // (the whole workgroup)
    {
        const uint32_t *src = (const uint32_t *)f.tab;
        uint32_t *dst = (uint32_t *)tab;
        for (unsigned i = threadIdx.x; i < sizeof(tab) / 4; i += MJD_ENT_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const unsigned i = blockIdx.x * MJD_ENT_THREADS + threadIdx.x;
    if (i >= f.n_int) return;
    const MjdScan g = f.scan;
    const MjdInterval iv = intervals[f.int_off + i];
    if (mjd_interval(g, tab, bytes + f.data_off, iv, coef + (size_t)blockIdx.y * blk_cap * 64)) atomicAdd(&bad[blockIdx.y], 1u);
}

// FIX(x) = rint(x 2^13) of jidctint.c
#define MJD_F_0_298631336 2446u
#define MJD_F_0_390180644 3196u
#define MJD_F_0_541196100 4433u
#define MJD_F_0_765366865 6270u
#define MJD_F_0_899976223 7373u
#define MJD_F_1_175875602 9633u
#define MJD_F_1_501321110 12299u
#define MJD_F_1_847759065 15137u
#define MJD_F_1_961570560 16069u
#define MJD_F_2_053119869 16819u
#define MJD_F_2_562915447 20995u
#define MJD_F_3_072711026 25172u

// one 8-point pass: d in, (x + 2^(SHIFT-1)) >> SHIFT out (arithmetic shift of the wrapped 32-bit sum)
template <int SHIFT> __device__ inline void mjd_idct8(const uint32_t d[8], int32_t r[8])
{
    uint32_t z1 = (d[2] + d[6]) * MJD_F_0_541196100;
    const uint32_t t2 = z1 - d[6] * MJD_F_1_847759065, t3 = z1 + d[2] * MJD_F_0_765366865;
    const uint32_t t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = d[7], a1 = d[5], a2 = d[3], a3 = d[1];
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * MJD_F_1_175875602;
    a0 *= MJD_F_0_298631336; a1 *= MJD_F_2_053119869; a2 *= MJD_F_3_072711026; a3 *= MJD_F_1_501321110;
    z1 *= 0u - MJD_F_0_899976223; z2 *= 0u - MJD_F_2_562915447; z3 *= 0u - MJD_F_1_961570560; z4 *= 0u - MJD_F_0_390180644;
    z3 += z5; z4 += z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const uint32_t half = 1u << (SHIFT - 1);
    r[0] = (int32_t)(t10 + a3 + half) >> SHIFT; r[7] = (int32_t)(t10 - a3 + half) >> SHIFT;
    r[1] = (int32_t)(t11 + a2 + half) >> SHIFT; r[6] = (int32_t)(t11 - a2 + half) >> SHIFT;
    r[2] = (int32_t)(t12 + a1 + half) >> SHIFT; r[5] = (int32_t)(t12 - a1 + half) >> SHIFT;
    r[3] = (int32_t)(t13 + a0 + half) >> SHIFT; r[4] = (int32_t)(t13 - a0 + half) >> SHIFT;
}

// libjpeg's range limit: x & 1023 through the table centred on 128
__device__ inline unsigned mjd_limit(int32_t x)
{
    const unsigned v = (unsigned)x & 1023u;
    return v < 128u ? v + 128u : v < 512u ? 255u : v < 896u ? 0u : v - 896u;
}

__device__ inline void mjd_store8(uint8_t *p, const unsigned v[8], int n, bool words)
{
    if (words && n == 8) {
        ((uint32_t *)p)[0] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        ((uint32_t *)p)[1] = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
    } else {
#pragma unroll
        for (int x = 0; x < 8; x++)
            if (x < n) p[x] = (uint8_t)v[x];
    }
}

__global__ __launch_bounds__(MJD_IDCT_THREADS) void k_mjdec_idct(const MjdFrame *__restrict__ frames, const int16_t *__restrict__ coef,
                                                                   size_t blk_cap, MjdOut out, unsigned *__restrict__ bad,
                                                                   uint32_t *__restrict__ status)
{
    __shared__ uint32_t ws[MJD_IDCT_BLOCKS][72];                                      // (72: pass 1's column reads of 4 blocks miss each other's banks; pass 2's rows still collide)
    const MjdFrame &f = frames[blockIdx.y];
    const int hs = f.scan.hs, vs = f.scan.vs, mw = f.scan.mw;
    const unsigned lb = (unsigned)(hs * vs), nblk = f.scan.n_mcu * lb;
    const unsigned b0 = blockIdx.x * MJD_IDCT_BLOCKS;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (status) status[blockIdx.y] = bad[blockIdx.y] + f.bad_host;
        bad[blockIdx.y] = 0;
    }
    if (b0 >= nblk) return;                                                          // (the whole workgroup)
    const int16_t *src = coef + ((size_t)blockIdx.y * blk_cap + b0) * 64;
    const unsigned here = min((unsigned)MJD_IDCT_BLOCKS, nblk - b0) * 64;
    for (unsigned e = threadIdx.x; e < here; e += MJD_IDCT_THREADS) {
        const unsigned k = e & 63u;
        ws[e >> 6][MJD_NATURAL[k]] = (uint32_t)((int32_t)src[e] * (int32_t)f.quant[k]);
    }
    __syncthreads();
    const unsigned blk = threadIdx.x >> 3, lane = threadIdx.x & 7u;
    const bool live = b0 + blk < nblk;
    uint32_t d[8];
    int32_t r[8];
    if (live) {                                                                      // pass 1: column `lane`
#pragma unroll
        for (int v = 0; v < 8; v++) d[v] = ws[blk][v * 8 + lane];
        mjd_idct8<11>(d, r);
#pragma unroll
        for (int v = 0; v < 8; v++) ws[blk][v * 8 + lane] = (uint32_t)r[v];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int u = 0; u < 8; u++) d[u] = ws[blk][lane * 8 + u];                        // pass 2: row `lane`
    mjd_idct8<18>(d, r);
    const unsigned b = b0 + blk, m = b / lb, j = b % lb;
    const int bx = (int)(m % (unsigned)mw) * hs + (int)(j % (unsigned)hs), by = (int)(m / (unsigned)mw) * vs + (int)(j / (unsigned)hs);
    const int x0 = bx * 8, y = by * 8 + (int)lane;
    if (y >= out.H || x0 >= out.W) return;                                           // padding of the last MCU row / column
    const int n = min(8, out.W - x0);
    unsigned g[8], mk[8], sh[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        g[u] = mjd_limit(r[u]);
        mk[u] = (int)g[u] > out.threshold ? 1u : 0u;
        sh[u] = mk[u] ? g[u] : 0u;
    }
    const size_t at = (size_t)blockIdx.y * out.frame_stride + (size_t)y * out.pitch + (size_t)x0;
    mjd_store8(out.frame + at, g, n, out.words != 0);
    if (out.mask) mjd_store8(out.mask + at, mk, n, out.words != 0);
    if (out.shown) mjd_store8(out.shown + at, sh, n, out.words != 0);
}
