// The registered video kept on the device (hm_body_rec_*) and the integer reductions over it that footprints, ROIs and
// traces are built from (hydra_mi/roi.py; tests/roi_ref.py restates all of it in NumPy and Python integers).
//
// The record holds, per frame, the bounding box of the body map: bh rows of `pitch` bytes (bw rounded up to 4, the
// padding 0), one byte per pixel, frames `fs` bytes apart (a multiple of 16) in chunks of `fpc` frames each.  A pixel
// outside the map is registered as 0 (k_body_warp), so a sum over any set of box pixels is the sum over its map pixels:
// the reductions look at the map only where they count pixels, which the host does.
#pragma once
#include "hm_types.h"         // (struct RecBox, REC_TP_MAX, d_peel_add)

__device__ __forceinline__ const uint8_t *d_rec_frame(const RecBox &b, const uint8_t *const *chunks, int k)
{
    const int ch = k / b.fpc;
    return chunks[ch] + (size_t)(k - ch * b.fpc) * b.fs;
}

// sum over the wave, every lane gets it (64 bits as two halves)
__device__ __forceinline__ unsigned long long d_wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// The registered plane (W x H, what k_body_warp has just written) -> one frame of the record; a dword per thread.
__global__ __launch_bounds__(256) void k_rec_copy(int W, RecBox b, const uint8_t *__restrict__ reg, uint8_t *__restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int per_row = b.pitch >> 2;
    if (i >= per_row * b.bh) return;
    const int y = i / per_row, x = 4 * (i - y * per_row);
    const uint8_t *src = reg + (size_t)(b.r0 + y) * W + b.c0 + x;
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (x + j < b.bw) w |= (unsigned)src[j] << (8 * j);
    *(unsigned *)(dst + (size_t)y * b.pitch + x) = w;
}

// The label image cut to the box: the label on map pixels, -1 elsewhere and in the padding.
__global__ __launch_bounds__(256) void k_rec_box_labels(int W, RecBox b, const int *__restrict__ tri_of,
                                                        const int *__restrict__ labels, int *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= b.pitch * b.bh) return;
    const int y = i / b.pitch, x = i - y * b.pitch;
    int l = -1;
    if (x < b.bw) {                    // (the padding may lie beyond the frame)
        const int p = (b.r0 + y) * W + b.c0 + x;
        if (tri_of[p] >= 0) l = labels[p];
    }
    out[i] = l;
}

// Sums per label and frame, out[k * L + label] (zeroed by the caller): 4 box pixels per thread, blockIdx.y strides over
// the frames, one atomic per distinct label of a wave (d_peel_add).  No thread leaves before the sums.
__global__ __launch_bounds__(256) void k_rec_label_sums(RecBox b, const uint8_t *const *__restrict__ chunks, int F,
                                                        const int *__restrict__ lab, int L, unsigned long long *__restrict__ out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool in = q < (b.pitch >> 2) * b.bh;
    int key[4] = {-1, -1, -1, -1};
    if (in) {
        const int4 t = *(const int4 *)(lab + 4 * q);
        key[0] = t.x; key[1] = t.y; key[2] = t.z; key[3] = t.w;
    }
    for (int k = blockIdx.y; k < F; k += gridDim.y) {
        const unsigned w = in ? *(const unsigned *)(d_rec_frame(b, chunks, k) + 4 * (size_t)q) : 0u;
        const unsigned val[4] = {w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, w >> 24};
        d_peel_add(key, val, out + (size_t)k * L);
    }
}

#define REC_RMAX 32                    // the largest disc, ring or weight window: |dx|, |dy| <= 32
#define REC_WIN_RMAX 16                // the largest footprint window

struct RecSeeds {
    RecBox b;
    const uint8_t *const *chunks;
    int F, P, R;                       // frames, seeds, half width of the window walked
    const int2 *seeds;                 // (col, row) in the frame
    double rd2, ri2, ro2;              // r_disc^2, r_in^2, r_out^2 as the host rounded them
    const unsigned *nT, *nG;           // map pixels of every seed's disc and ring (counted by the host)
    unsigned long long *T, *G;         // F x P
    long long *U;                      // F x P: n_G T - n_T G
};

// One wave per frame and seed: T = sum over the disc (d2 <= r_disc^2), G = sum over the ring (r_in^2 <= d2 <= r_out^2),
// d2 the whole number dx^2 + dy^2 compared in binary64, and U = n_G T - n_T G.  A lane's sums stay below 2^32.
__global__ __launch_bounds__(256) void k_rec_seed_traces(RecSeeds g)
{
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= g.F * g.P) return;     // (the whole wave)
    const int k = wave / g.P, s = wave - k * g.P;
    const int2 sd = g.seeds[s];
    const uint8_t *f = d_rec_frame(g.b, g.chunks, k);
    const int S = 2 * g.R + 1;
    unsigned t = 0, r = 0;
    for (int i = lane; i < S * S; i += 64) {
        const int iy = i / S, dy = iy - g.R, dx = i - iy * S - g.R;
        const int x = sd.x + dx - g.b.c0, y = sd.y + dy - g.b.r0;
        if (x < 0 || x >= g.b.bw || y < 0 || y >= g.b.bh) continue;
        const double d2 = (double)(dx * dx + dy * dy);
        const bool inT = d2 <= g.rd2, inG = d2 >= g.ri2 && d2 <= g.ro2;
        if (!(inT || inG)) continue;
        const unsigned v = f[(size_t)y * g.b.pitch + x];
        if (inT) t += v;
        if (inG) r += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t += (unsigned)__shfl_xor((int)t, o);
        r += (unsigned)__shfl_xor((int)r, o);
    }
    if (lane == 0) {
        const size_t o = (size_t)k * g.P + s;
        g.T[o] = t;
        g.G[o] = r;
        g.U[o] = (long long)g.nG[s] * (long long)t - (long long)g.nT[s] * (long long)r;
    }
}

struct RecWin {
    RecBox b;
    const uint8_t *const *chunks;
    int F, P, R;
    const int2 *seeds;
    const long long *U;                // F x P (k_rec_seed_traces)
    unsigned long long *w1, *w2;       // P x (2R + 1)^2
    long long *c;                      // P x (2R + 1)^2
    long long *u1, *u2;                // P
};

// One thread per window pixel (blockIdx.y: the seed), the frames in ascending order: w1 = sum v, w2 = sum v^2,
// c = sum v U; the thread of window pixel 0 also writes u1 = sum U, u2 = sum U^2.  0 for a window pixel outside the box.
// The host has refused seeds whose F (255 n_T n_G)^2 could pass 2^63: every sum is exact.
__global__ __launch_bounds__(256) void k_rec_window_sums(RecWin g)
{
    const int S = 2 * g.R + 1, n = S * S;
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2 sd = g.seeds[s];
    const int iy = i / S, dy = iy - g.R, dx = i - iy * S - g.R;
    const int x = sd.x + dx - g.b.c0, y = sd.y + dy - g.b.r0;
    const bool in = x >= 0 && x < g.b.bw && y >= 0 && y < g.b.bh;
    const size_t off = in ? (size_t)y * g.b.pitch + x : 0;
    unsigned long long a1 = 0, a2 = 0;
    long long ac = 0, b1 = 0, b2 = 0;
    for (int k0 = 0, ch = 0; k0 < g.F; k0 += g.b.fpc, ch++) {
        const uint8_t *f = g.chunks[ch] + off;
        const int m = min(g.b.fpc, g.F - k0);
        for (int j = 0; j < m; j++, f += g.b.fs) {
            const long long U = g.U[(size_t)(k0 + j) * g.P + s];
            const long long v = in ? (long long)*f : 0ll;
            a1 += (unsigned long long)v;
            a2 += (unsigned long long)(v * v);
            ac += v * U;
            b1 += U;
            b2 += U * U;
        }
    }
    const size_t o = (size_t)s * n + i;
    g.w1[o] = a1;
    g.w2[o] = a2;
    g.c[o] = ac;
    if (i == 0) {
        g.u1[s] = b1;
        g.u2[s] = b2;
    }
}

// One wave per frame and seed: out[k * P + s] = sum over the window of weight x value (weights P x (2R + 1)^2).
__global__ __launch_bounds__(256) void k_rec_weighted_sums(RecBox b, const uint8_t *const *__restrict__ chunks, int F, int P,
                                                           int R, const int2 *__restrict__ seeds,
                                                           const uint16_t *__restrict__ weights,
                                                           unsigned long long *__restrict__ out)
{
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= F * P) return;         // (the whole wave)
    const int k = wave / P, s = wave - k * P;
    const int2 sd = seeds[s];
    const uint8_t *f = d_rec_frame(b, chunks, k);
    const int S = 2 * R + 1;
    const uint16_t *a = weights + (size_t)s * S * S;
    unsigned long long sum = 0;
    for (int i = lane; i < S * S; i += 64) {
        const int iy = i / S, dy = iy - R, dx = i - iy * S - R;
        const int x = sd.x + dx - b.c0, y = sd.y + dy - b.r0;
        if (x < 0 || x >= b.bw || y < 0 || y >= b.bh) continue;
        sum += (unsigned long long)((unsigned)a[i] * (unsigned)f[(size_t)y * b.pitch + x]);
    }
    sum = d_wave_sum64(sum);
    if (lane == 0) out[(size_t)k * P + s] = sum;
}


struct RecTP {
    RecBox b;
    const uint8_t *const *chunks;
    int F, P, R, tpf;                  // frames, seeds, half width of the window, frames per run
    const int2 *seeds;
    const int *q;                      // F x P, frame-major
    unsigned long long *out;           // P x (2R + 1)^2, zeroed by the caller
};

// out[s, p] += sum over a run of frames of v_k(p) q[k, s].  A workgroup takes 64 consecutive window pixels of one seed
// (blockIdx.x; a lane per pixel, so a wave reads a record row in runs of 2R + 1 bytes) and runs of tpf frames
// (blockIdx.y strides over them).  The run's q sits in LDS; the four waves take every fourth frame of the run, add
// their sums through LDS, and one wave adds the result to `out` with one 64-bit atomic per pixel: whole numbers mod
// 2^64, so the order of the adds does not matter.  A window pixel outside the box adds nothing.
__global__ __launch_bounds__(256) void k_rec_trace_products(RecTP g)
{
    __shared__ int qs[REC_TP_MAX];
    __shared__ long long part[3][64];
    const int S = 2 * g.R + 1, n = S * S, tiles = (n + 63) >> 6;
    const int s = blockIdx.x / tiles, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = (blockIdx.x - s * tiles) * 64 + lane;
    const int2 sd = g.seeds[s];
    bool in = false;
    size_t off = 0;
    if (i < n) {
        const int iy = i / S, dy = iy - g.R, dx = i - iy * S - g.R;
        const int x = sd.x + dx - g.b.c0, y = sd.y + dy - g.b.r0;
        in = x >= 0 && x < g.b.bw && y >= 0 && y < g.b.bh;
        if (in) off = (size_t)y * g.b.pitch + x;
    }
    long long acc = 0;
    const int runs = (g.F + g.tpf - 1) / g.tpf;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {         // (the same trips for the whole workgroup)
        const int k0 = run * g.tpf, m = min(g.tpf, g.F - k0);
        __syncthreads();                                               // the previous run's q has been read
        for (int j = threadIdx.x; j < m; j += 256) qs[j] = g.q[(size_t)(k0 + j) * g.P + s];
        __syncthreads();
        if (in)
            for (int j = w; j < m; j += 4) acc += (long long)d_rec_frame(g.b, g.chunks, k0 + j)[off] * (long long)qs[j];
    }
    if (w) part[w - 1][lane] = acc;
    __syncthreads();
    if (w == 0 && in) {
        acc += part[0][lane] + part[1][lane] + part[2][lane];
        atomicAdd(g.out + (size_t)s * n + i, (unsigned long long)acc);
    }
}
