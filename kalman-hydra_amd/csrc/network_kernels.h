// Every trace against every pixel of the kept registered video (hm_body_rec_trace_maps; hydra_mi/network.py; DESIGN.md
// section 17; tests/network_ref.py restates all of it in NumPy integers).
//
// For L whole-number traces q[k, s], |q| <= 32767, over the F recorded frames, v_k(p) the recorded value of box pixel p:
//   c[s, p] = sum_k v_k(p) q[k, s]        int64
//   w1[p]   = sum_k v_k(p)                uint64
//   w2[p]   = sum_k v_k(p)^2              uint64
// as planes of the box (rows of b.pitch values; the padding and the box pixels off the map are recorded as 0, so their
// sums are 0).  The host cuts the planes into the frame (record.hip).
#pragma once
#include "roi_kernels.h"         // (d_rec_frame; REC_MAP_MAX: hm_types.h)

#define REC_MAP_LMAX 1024              // the most traces of a call
#define REC_MAP_QMAX 32767             // the largest |q|: a product v q stays below 2^23
#define REC_MAP_GROUP 8                // traces a workgroup multiplies into a dword it has loaded
#define REC_MAP_UNROLL 4               // frames whose record dwords a lane loads before it works on them

struct RecMaps {
    RecBox b;
    const uint8_t *const *chunks;
    int F, L, run;                     // frames, traces, frames per run (<= REC_MAP_MAX)
    const int *q;                      // F x L, frame-major
    unsigned long long *c;             // L planes of pitch * bh, zeroed by the caller; NULL: no products
    unsigned long long *w1, *w2;       // a plane of pitch * bh each, zeroed by the caller; NULL (both): no sums
};

// A thread owns one dword of the box frame, four pixels (blockIdx.x * 256 + threadIdx.x), blockIdx.z a group of
// REC_MAP_GROUP traces (the last may be partial) and blockIdx.y strides over the runs of g.run frames.  The run's q of
// the group sits in LDS (every lane reads the same words: a broadcast); per frame a lane loads one dword of the record
// (REC_MAP_UNROLL frames' loads at a time) and adds 4 x 8 products to 32-bit accumulators: |v q| <= 255 x 32767 < 2^23 and
// a run has at most 256 frames, so they hold (255 x 32767 x 256 < 2^31; the sums of v^2: 255^2 x 256 < 2^24).  At the end
// of a run they are widened and added with one 64-bit atomic per (trace, pixel): whole numbers mod 2^64, the same result
// in any order and for any run length.  An accumulator that is 0 adds nothing (every pixel off the map).  w1 and w2 are
// added by the first group only.  No thread leaves before a barrier.  Integers only.
__global__ __launch_bounds__(256) void k_rec_trace_maps(RecMaps g)
{
    __shared__ int qs[REC_MAP_MAX * REC_MAP_GROUP];
    const int dw = blockIdx.x * 256 + threadIdx.x;
    const size_t nb = (size_t)g.b.pitch * g.b.bh;
    const bool in = (size_t)dw < nb >> 2;                          // (the last workgroup may end beyond the frame)
    const int g0 = blockIdx.z * REC_MAP_GROUP, ng = min(REC_MAP_GROUP, g.L - g0);
    const bool prod = g.c != nullptr, sums = blockIdx.z == 0 && g.w1 != nullptr;
    const int runs = (g.F + g.run - 1) / g.run;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {     // (the same trips for the whole workgroup)
        const int k0 = run * g.run, m = min(g.run, g.F - k0);
        __syncthreads();                                           // the previous run's q has been read
        if (prod)
            for (int e = threadIdx.x; e < m * REC_MAP_GROUP; e += 256) {
                const int j = e / REC_MAP_GROUP, t = e - j * REC_MAP_GROUP;
                qs[e] = t < ng ? g.q[(size_t)(k0 + j) * g.L + g0 + t] : 0;
            }
        __syncthreads();
        int acc[REC_MAP_GROUP][4];
        unsigned s1[4] = {0u, 0u, 0u, 0u}, s2[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < REC_MAP_GROUP; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) acc[t][i] = 0;
        for (int j4 = 0; j4 < m; j4 += REC_MAP_UNROLL) {
            unsigned vs[REC_MAP_UNROLL];                           // (the loads of REC_MAP_UNROLL frames are in flight together)
#pragma unroll
            for (int u = 0; u < REC_MAP_UNROLL; u++)
                vs[u] = in && j4 + u < m ? *(const unsigned *)(d_rec_frame(g.b, g.chunks, k0 + j4 + u) + 4 * (size_t)dw) : 0u;
#pragma unroll
            for (int u = 0; u < REC_MAP_UNROLL; u++) {
                if (j4 + u >= m) break;                            // (the whole workgroup)
                const int v[4] = {(int)(vs[u] & 255u), (int)((vs[u] >> 8) & 255u), (int)((vs[u] >> 16) & 255u), (int)(vs[u] >> 24)};
                if (prod) {
                    const int *qj = qs + (j4 + u) * REC_MAP_GROUP;
#pragma unroll
                    for (int t = 0; t < REC_MAP_GROUP; t++) {
                        const int qt = qj[t];
#pragma unroll
                        for (int i = 0; i < 4; i++) acc[t][i] += __mul24(v[i], qt);
                    }
                }
                if (sums) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        s1[i] += (unsigned)v[i];
                        s2[i] += (unsigned)__mul24(v[i], v[i]);
                    }
                }
            }
        }
        if (in) {
            const size_t p = 4 * (size_t)dw;
            if (prod) {
#pragma unroll
                for (int t = 0; t < REC_MAP_GROUP; t++) {
                    if (t >= ng) break;                            // (the whole workgroup)
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (acc[t][i] != 0) atomicAdd(g.c + (size_t)(g0 + t) * nb + p + i, (unsigned long long)(long long)acc[t][i]);
                }
            }
            if (sums) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (s1[i] != 0u) {
                        atomicAdd(g.w1 + p + i, (unsigned long long)s1[i]);
                        atomicAdd(g.w2 + p + i, (unsigned long long)s2[i]);
                    }
            }
        }
    }
}
