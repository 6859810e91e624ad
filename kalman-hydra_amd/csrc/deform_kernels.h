// The kept registered video against the deformation of its own tissue (hm_body_rec_tri_maps / _tri_gain;
// hydra_mi/deform.py; tests/deform_ref.py restates all of it in NumPy integers).
//
// t(p) is the body map's triangle of box pixel p, as a plane of the box (rows of b.pitch ints; -1 in the padding and off
// the map: k_rec_box_labels with the map as its own label image).  Such a pixel is recorded as 0, so it may be worked
// through under any triangle: its products and sums are 0, and every gain of 0 is 0.  The kernels read it under triangle 0
// and never branch on the map.
//   tri_maps   c[p] = sum_k v_k(p) q[k, t(p)]  (int64),  w1[p] = sum_k v_k(p),  w2[p] = sum_k v_k(p)^2  (uint64)
//   tri_gain   v_k(p) <- min(255, (v_k(p) m[k, t(p)] + 2048) >> 12) in unsigned 32-bit integers, in place
#pragma once
#include "roi_kernels.h"         // (d_rec_frame, d_wave_sum64; REC_TM_MAX: hm_types.h)

#define REC_TM_QMAX 32767              // the largest |q|: a product v q stays below 2^23
#define REC_TM_UNROLL 4                // frames whose record dwords a lane loads before it works on them
#define REC_TG_FRAMES 8                // frames a lane of k_rec_tri_gain rewrites: the triangles of its pixels are loaded once for them

struct RecTriMaps {
    RecBox b;
    const uint8_t *const *chunks;
    int F, T, run;                     // frames, triangles, frames per run (<= REC_TM_MAX)
    const int *tri;                    // t(p): a plane of pitch * bh
    const int16_t *q;                  // F x T, frame-major (the host has checked the range)
    unsigned long long *c, *w1, *w2;   // a plane of pitch * bh each, zeroed by the caller; c NULL: no products; w1, w2 NULL (both): no sums
};

// one frame's dword and the q of its four pixels into a lane's sums
__device__ __forceinline__ void d_tri_maps_add(unsigned w, const int (&q)[4], int (&acc)[4], unsigned (&s1)[4], unsigned (&s2)[4])
{
    const int v[4] = {(int)(w & 255u), (int)((w >> 8) & 255u), (int)((w >> 16) & 255u), (int)(w >> 24)};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        acc[i] += __mul24(v[i], q[i]);
        s1[i] += (unsigned)v[i];
        s2[i] += (unsigned)__mul24(v[i], v[i]);
    }
}

// A thread owns one dword of the box frame, four pixels (blockIdx.x * 256 + threadIdx.x), and blockIdx.y strides over the
// runs of g.run frames.  Per frame a lane loads one dword of the record and the q of its four pixels' triangles from the
// frame's row of 2T bytes -- neighbouring pixels share a triangle, so the lanes of a wave read a few 16-bit words of one
// or two cache lines -- REC_TM_UNROLL frames at a time with nothing conditional between their loads (a run is walked in
// the pieces that lie in one chunk each; what is left of a piece goes frame by frame), and adds into 32-bit accumulators: |v q| <= 255 x 32767 < 2^23 and a run has at most 256
// frames, so they hold (255 x 32767 x 256 < 2^31; v: 255 x 256; v^2: 65025 x 256 < 2^32).  At the end of a run they are
// widened and added with one 64-bit atomic per pixel and plane: whole numbers mod 2^64, the same result in any order and
// for any run length.  An accumulator that is 0 adds nothing (every pixel off the map).  PROD 0: no products, q is not
// read.  Integers only, no LDS, no barrier.
template <int PROD>
__global__ __launch_bounds__(256) void k_rec_tri_maps(RecTriMaps g)
{
    const int dw = blockIdx.x * 256 + threadIdx.x;
    const size_t nb = (size_t)g.b.pitch * g.b.bh;
    if ((size_t)dw >= nb >> 2) return;                             // (the last workgroup may end beyond the frame)
    const int4 t4 = *(const int4 *)(g.tri + 4 * (size_t)dw);
    const int t[4] = {max(t4.x, 0), max(t4.y, 0), max(t4.z, 0), max(t4.w, 0)};
    const bool sums = g.w1 != nullptr;
    const int runs = (g.F + g.run - 1) / g.run;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        const int k0 = run * g.run, m = min(g.run, g.F - k0);
        const int16_t *qk = g.q + (size_t)k0 * g.T;
        int acc[4] = {0, 0, 0, 0};
        unsigned s1[4] = {0u, 0u, 0u, 0u}, s2[4] = {0u, 0u, 0u, 0u};
        for (int k = k0; k < k0 + m;) {                            // the pieces of the run that lie in one chunk each
            const int ch = k / g.b.fpc, off = k - ch * g.b.fpc, n = min(g.b.fpc - off, k0 + m - k);
            const uint8_t *f = g.chunks[ch] + (size_t)off * g.b.fs + 4 * (size_t)dw;
            int j = 0;
            for (; j + REC_TM_UNROLL <= n; j += REC_TM_UNROLL) {
                unsigned vs[REC_TM_UNROLL];                        // (the loads of REC_TM_UNROLL frames are in flight together)
                int qs[REC_TM_UNROLL][4] = {};
#pragma unroll
                for (int u = 0; u < REC_TM_UNROLL; u++) vs[u] = *(const unsigned *)(f + (size_t)u * g.b.fs);
                if (PROD) {
#pragma unroll
                    for (int u = 0; u < REC_TM_UNROLL; u++)
#pragma unroll
                        for (int i = 0; i < 4; i++) qs[u][i] = (int)qk[(size_t)u * g.T + t[i]];
                }
#pragma unroll
                for (int u = 0; u < REC_TM_UNROLL; u++) d_tri_maps_add(vs[u], qs[u], acc, s1, s2);
                f += REC_TM_UNROLL * g.b.fs;
                qk += (size_t)REC_TM_UNROLL * g.T;
            }
            for (; j < n; j++) {
                const unsigned w = *(const unsigned *)f;
                int q1[4] = {0, 0, 0, 0};
                if (PROD) {
#pragma unroll
                    for (int i = 0; i < 4; i++) q1[i] = (int)qk[t[i]];
                }
                d_tri_maps_add(w, q1, acc, s1, s2);
                f += g.b.fs;
                qk += g.T;
            }
            k += n;
        }
        const size_t p = 4 * (size_t)dw;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (PROD && acc[i] != 0) atomicAdd(g.c + p + i, (unsigned long long)(long long)acc[i]);
            if (sums && s1[i] != 0u) {
                atomicAdd(g.w1 + p + i, (unsigned long long)s1[i]);
                atomicAdd(g.w2 + p + i, (unsigned long long)s2[i]);
            }
        }
    }
}

struct RecTriGain {
    RecBox b;
    uint8_t *const *chunks;            // the record, rewritten in place
    int F, T;                          // frames, triangles
    const int *tri;                    // t(p): a plane of pitch * bh
    const uint16_t *m;                 // F x T, frame-major
    unsigned long long *clipped;       // one counter, zeroed by the caller
};

// one dword of the record times the gains of its four pixels -> the dword rewritten; n: the values that were clipped
__device__ __forceinline__ unsigned d_tri_gain(unsigned w, const unsigned (&m)[4], unsigned &n)
{
    unsigned out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned r = (((w >> (8 * i)) & 255u) * m[i] + 2048u) >> 12;
        n += r > 255u;
        out |= min(r, 255u) << (8 * i);
    }
    return out;
}

// A thread owns one dword of the box frame in groups of REC_TG_FRAMES consecutive frames of one chunk (blockIdx.z: the
// chunk, blockIdx.y strides over its groups; both stride on where the grid is short), loads a group's dwords and the m of its four pixels' triangles with nothing
// conditional between the loads (the last group of a chunk, if it is partial, goes frame by frame), and stores every dword
// once: the rule is pointwise, so the frames are rewritten where they lie, the whole record in one launch.  A value
// whose unclamped result passes 255 is counted; the counts are summed over the wave and a wave that has any adds them
// with one 64-bit atomic.  No thread leaves before the wave's sum.
__global__ __launch_bounds__(256) void k_rec_tri_gain(RecTriGain g)
{
    const int dw = blockIdx.x * 256 + threadIdx.x;
    unsigned n = 0;
    if ((size_t)dw < ((size_t)g.b.pitch * g.b.bh) >> 2) {          // (the last workgroup may end beyond the frame)
        const int4 t4 = *(const int4 *)(g.tri + 4 * (size_t)dw);
        const int t[4] = {max(t4.x, 0), max(t4.y, 0), max(t4.z, 0), max(t4.w, 0)};
        for (int ch = blockIdx.z, k0 = ch * g.b.fpc; k0 < g.F; ch += gridDim.z, k0 = ch * g.b.fpc) {
            const int frames = min(g.b.fpc, g.F - k0);
            uint8_t *chunk = g.chunks[ch] + 4 * (size_t)dw;
            for (int j0 = blockIdx.y * REC_TG_FRAMES; j0 < frames; j0 += gridDim.y * REC_TG_FRAMES) {
                uint8_t *f = chunk + (size_t)j0 * g.b.fs;
                const uint16_t *mk = g.m + (size_t)(k0 + j0) * g.T;
                if (j0 + REC_TG_FRAMES <= frames) {                    // (the whole workgroup)
                    unsigned vs[REC_TG_FRAMES], ms[REC_TG_FRAMES][4];
#pragma unroll
                    for (int u = 0; u < REC_TG_FRAMES; u++) vs[u] = *(const unsigned *)(f + (size_t)u * g.b.fs);
#pragma unroll
                    for (int u = 0; u < REC_TG_FRAMES; u++)
#pragma unroll
                        for (int i = 0; i < 4; i++) ms[u][i] = (unsigned)mk[(size_t)u * g.T + t[i]];
#pragma unroll
                    for (int u = 0; u < REC_TG_FRAMES; u++) *(unsigned *)(f + (size_t)u * g.b.fs) = d_tri_gain(vs[u], ms[u], n);
                } else {
                    for (int u = 0; j0 + u < frames; u++) {
                        unsigned m1[4];
#pragma unroll
                        for (int i = 0; i < 4; i++) m1[i] = (unsigned)mk[(size_t)u * g.T + t[i]];
                        unsigned *d = (unsigned *)(f + (size_t)u * g.b.fs);
                        *d = d_tri_gain(*d, m1, n);
                    }
                }
            }
        }
    }
    if (g.clipped) {
        const unsigned long long sum = d_wave_sum64((unsigned long long)n);
        if (__lane_id() == 0 && sum != 0) atomicAdd(g.clipped, sum);
    }
}
