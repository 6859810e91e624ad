// The Gram matrix of frames of the kept registered video (hm_body_rec_gram; hydra_mi/pca.py; DESIGN.md section 22;
// tests/pca_ref.py restates the host's half in loops and Python integers).
//
// For the frames f_i = k0 + i stride, i = 0 .. n - 1, v_f(p) the recorded byte of box pixel p:
//   G[i, j] = sum_p v_fi(p) v_fj(p)       int64, the full symmetric n x n matrix
//   s1[i]   = sum_p v_fi(p)               uint64
// The products are made by v_mfma_i32_16x16x64_i8, which multiplies SIGNED bytes: with x = v - 128 (one XOR with 0x80 per
// byte) and Kp = pitch * bh, the bytes of a frame,
//   sum_p v_i v_j = sum_p x_i x_j + 128 (s_i + s_j) - 16384 Kp,        s_i = sum_p x_i + 128 Kp.
// k_rec_gram forms sum x_i x_j and sum x_i (a column of ones through the same instruction), k_rec_gram_fix turns them into
// G and s1.  The padding and the box pixels off the map are recorded as 0, so the sums over the box are the sums over the map.
#pragma once
#include "roi_kernels.h"         // (d_rec_frame; REC_GRAM_MAX, REC_GRAM_BYTES_MAX: hm_types.h)

typedef int gram_v4i __attribute__((ext_vector_type(4)));

struct RecGram {
    RecBox b;
    const uint8_t *const *chunks;
    int k0, n, stride;                 // the frames k0 + i stride, i < n
    int run;                           // bytes per run: a multiple of 64, <= REC_GRAM_BYTES_MAX
    unsigned long long *G;             // n x n sums of x_i x_j (two's complement), zeroed by the caller; NULL: the sums of x only
    unsigned long long *sx;            // n sums of x_i (two's complement), zeroed by the caller
};

// The 16 bytes of a frame at byte q of it as signed x = v - 128; p is their address.  A byte at or past nb is x = 0: it adds
// nothing to any sum.  nb is a multiple of 4 and at most pitch * bh (the end of the run, or of the frame): the gap up to fs is
// not read as data, and nothing at or past fs is loaded (fs is pitch * bh rounded up to 16 and q a multiple of 16, so q < nb
// keeps the 16-byte load inside the frame).
__device__ __forceinline__ gram_v4i d_gram_frag(const uint8_t *p, size_t q, size_t nb)
{
    gram_v4i w = {0, 0, 0, 0};
    if (q < nb) {
        w = *(const __attribute__((address_space(1))) gram_v4i *)p;          // (the record is global memory: a global load, not a flat one)
        w ^= (int)0x80808080u;
        if (q + 4 >= nb) w.y = 0;
        if (q + 8 >= nb) w.z = 0;
        if (q + 12 >= nb) w.w = 0;
    }
    return w;
}

#define GRAM_BLK 128                   // rows and columns of G a workgroup owns
#define GRAM_PASS 256                  // bytes of every frame staged in LDS per pass: four steps of the instruction
#define GRAM_PITCH (GRAM_PASS + 16)    // bytes between two rows in LDS: 68 dwords, so the 16 rows of a tile start 4 banks apart

// A workgroup of four waves owns a 128 x 128 block (bi, bj >= bi) of G and one run of g.run bytes of the frames; wave w owns
// the 64 x 64 quarter (w >> 1, w & 1) of it as 4 x 4 tiles of 16 x 16.  blockIdx.x is the pair of blocks (upper triangle,
// row-major), blockIdx.y strides over the runs.  Per pass the workgroup stages GRAM_PASS bytes of its 128 row frames and its
// 128 column frames in LDS as x = v - 128 (d_gram_frag: one 16-byte global load per piece, 16 pieces a row, 8 + 8 pieces a
// thread; a diagonal block stages its frames once), so a byte of the record is asked for once per workgroup, not once per
// wave and tile.  Then, per step of 64 bytes, lane l of a wave reads for each of its four row tiles and four column tiles
// frame (l & 15) of the tile with the 16 bytes at 16 (l >> 4) of the step (ds_read_b128) and the wave does 16 MFMAs: both
// operands by one rule, so byte k of a row meets byte k of a column whatever order the instruction takes the 64 in.
// A frame index at or past n is clamped to n - 1; its results are not stored.  Bytes at or past the end of the run or of
// the frame are staged as x = 0.  The quarters on the diagonal of a diagonal block also multiply their rows into a column
// of ones: the sums of x.  C/D: column l & 15, row 4 (l >> 4) + register.
// The accumulators are 32-bit: |x_i x_j| <= 2^14 and a run has at most REC_GRAM_BYTES_MAX = 131008 bytes, 2^14 x 131008 <
// 2^31 (hm_types.h).  At the end of a run they are widened and added with 64-bit integer atomics, an off-diagonal block to
// both places: whole numbers mod 2^64, the same bytes in any order and for every run length.  No thread leaves before a
// barrier: the trips of both loops are the same for the whole workgroup.
__global__ __launch_bounds__(256) void k_rec_gram(RecGram g)
{
    __shared__ __attribute__((aligned(16))) uint8_t sa[GRAM_BLK * GRAM_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t sb[GRAM_BLK * GRAM_PITCH];
    __shared__ const uint8_t *frame[2 * GRAM_BLK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kg = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int nbk = (g.n + GRAM_BLK - 1) / GRAM_BLK;
    int bi = 0, rem = blockIdx.x;
    if (g.G) {
        while (rem >= nbk - bi) { rem -= nbk - bi; bi++; }       // (blockIdx.x < nbk (nbk + 1) / 2: it ends with bi < nbk)
    } else {
        bi = rem; rem = 0;                                         // the diagonal blocks alone
    }
    const int bj = bi + rem;
    const bool diag = bi == bj, sums = diag && wi == wj;
    const size_t nb = (size_t)g.b.pitch * g.b.bh;
    {
        const int i = min((tid < GRAM_BLK ? bi : bj) * GRAM_BLK + (tid & (GRAM_BLK - 1)), g.n - 1);
        frame[tid] = d_rec_frame(g.b, g.chunks, g.k0 + i * g.stride);
    }
    const uint8_t *la = sa + (wi * 64 + r) * GRAM_PITCH + 16 * kg;
    const uint8_t *lb = (diag ? sa : sb) + (wj * 64 + r) * GRAM_PITCH + 16 * kg;
    const gram_v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const size_t runs = (nb + (size_t)g.run - 1) / (size_t)g.run;
    for (size_t run = blockIdx.y; run < runs; run += gridDim.y) {
        const size_t o0 = run * (size_t)g.run, o1 = min(o0 + (size_t)g.run, nb);
        gram_v4i acc[4][4], as[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            as[t] = gram_v4i{0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; u++) acc[t][u] = gram_v4i{0, 0, 0, 0};
        }
        for (size_t o = o0; o < o1; o += GRAM_PASS) {
            __syncthreads();                                       // the previous pass has been read (and `frame` written)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int p = tid + 256 * i, row = p >> 4;
                const size_t q = o + 16 * (size_t)(p & 15);
                *(gram_v4i *)(sa + row * GRAM_PITCH + 16 * (p & 15)) = d_gram_frag(frame[row] + q, q, o1);
            }
            if (!diag) {                                           // (the whole workgroup)
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int p = tid + 256 * i, row = p >> 4;
                    const size_t q = o + 16 * (size_t)(p & 15);
                    *(gram_v4i *)(sb + row * GRAM_PITCH + 16 * (p & 15)) = d_gram_frag(frame[GRAM_BLK + row] + q, q, o1);
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < GRAM_PASS / 64; s++) {
                gram_v4i a[4], b[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    a[t] = *(const gram_v4i *)(la + t * 16 * GRAM_PITCH + 64 * s);
                    b[t] = *(const gram_v4i *)(lb + t * 16 * GRAM_PITCH + 64 * s);
                }
                if (sums) {                                        // (the whole wave)
#pragma unroll
                    for (int t = 0; t < 4; t++) as[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], ones, as[t], 0, 0, 0);
                }
                if (g.G) {
#pragma unroll
                    for (int t = 0; t < 4; t++)
#pragma unroll
                        for (int u = 0; u < 4; u++) acc[t][u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[u], acc[t][u], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = bi * GRAM_BLK + wi * 64 + 16 * t + 4 * kg + i;
                if (row >= g.n) continue;
                if (g.G) {
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int col = bj * GRAM_BLK + wj * 64 + 16 * u + r, v = acc[t][u][i];
                        if (col >= g.n || v == 0) continue;
                        atomicAdd(g.G + (size_t)row * g.n + col, (unsigned long long)(long long)v);
                        if (!diag) atomicAdd(g.G + (size_t)col * g.n + row, (unsigned long long)(long long)v);
                    }
                }
                if (sums && r == 0 && as[t][i] != 0) atomicAdd(g.sx + row, (unsigned long long)(long long)as[t][i]);
            }
    }
}

// sum x_i x_j, sum x_i -> G and s1 (the identity at the head of this file), kp = pitch * bh; a thread per column j,
// blockIdx.y strides over the rows.  G or s1 may be NULL.
__global__ __launch_bounds__(256) void k_rec_gram_fix(int n, long long kp, const long long *__restrict__ sx, long long *G,
                                                      unsigned long long *s1)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long long sj = sx[j] + 128 * kp;
    if (s1 && blockIdx.y == 0) s1[j] = (unsigned long long)sj;
    if (!G) return;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const long long si = sx[i] + 128 * kp;
        G[(size_t)i * n + j] += 128 * (si + sj) - 16384 * kp;
    }
}
