// The residual video of the kept registered video: what the demixed model of the cells leaves of every recorded frame
// (hm_body_rec_residual_planes, hm_body_rec_residual_stats_add; hydra_mi/residual.py; tests/residual_ref.py restates all
// of it in NumPy integers).
//
// For recorded frame k and map pixel p, v_k(p) the recorded value, the layers j = 0 .. n_layers - 1 with a label >= 0 at p:
//   acc      = sum_j weights[j][p] * traces[k][labels[j][p]]                  int64; 4 * 65535 * 2^31 < 2^50: no order matters
//   m        = (acc + 2^23) >> 24                                             arithmetic shift: floor, a tie goes up
//   r        = offset + v_k(p) - m
//   R_k(p)   = min(255, max(0, r));  0 where blank[p] != 0, outside the map and in the padding
//   clipped  counts the (frame, map pixel, not blanked) with r outside 0 .. 255
#pragma once
#include "detrend_kernels.h"     // (REC_RES_LMAX, REC_RES_MAX: hm_types.h)

#define REC_RES_UNROLL 4               // frames whose record dwords a lane loads before it works on them

struct RecResidual {
    RecBox b;
    const uint8_t *const *chunks;
    int k0, n;                         // the frames written: k0 .. k0 + n - 1
    int run;                           // frames per run
    int nl, L, offset;
    // The host packs all of these for the box (record.hip: res_pack_host), pixels as in a record's frame (row pitch b.pitch):
    const unsigned *lay;               // nl planes of pitch * bh dwords: label << 16 | weight; 0 (label 0, weight 0) for none
    const unsigned *live;              // pitch * bh bytes: 1 for a map pixel that is not blanked, else 0
    const uint8_t *seg_nl;             // per segment of 64 dwords: the layers 0 .. seg_nl - 1 carry a label somewhere in it
    const int *traces;                 // rows of L, row k for recorded frame k
    uint8_t *out;                      // n frames in the record's layout, fs bytes apart
    unsigned long long *clipped;
};

// One wave per segment of 64 dwords of the box frame (blockIdx.x) and run of frames (blockIdx.y strides over the runs): a
// lane owns one dword, four box pixels, for the whole run.  It loads their `live` bytes and, of the layers the segment
// needs, their packed labels and weights (one 16-byte load per layer) once per run; per frame it reads one dword of the
// record (REC_RES_UNROLL frames' loads at a time) and writes one of the result.  The trace rows are read through L1 / L2: a row is L * 4 bytes that every lane of
// every segment with cells reads in the same frame.  A segment without cells (seg_nl 0: wave-uniform) never looks at the
// layers or the traces.  Integers only.
__global__ __launch_bounds__(64) void k_rec_residual(RecResidual g)
{
    const int lane = threadIdx.x, dw = blockIdx.x * 64 + lane;
    const int npx = g.b.pitch * g.b.bh;
    const bool dw_ok = dw < npx >> 2;                              // (the last segment may end beyond the frame)
    const int runs = (g.n + g.run - 1) / g.run;
    const int nls = min((int)g.seg_nl[blockIdx.x], g.nl);
    const unsigned live = dw_ok ? g.live[dw] : 0u;
    uint4 lay[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        lay[j] = dw_ok && j < nls ? *(const uint4 *)(g.lay + (size_t)j * npx + 4 * (size_t)dw) : make_uint4(0u, 0u, 0u, 0u);
    int clip = 0;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        const int ks = g.k0 + run * g.run, ke = min(ks + g.run, g.k0 + g.n);
        for (int k4 = ks; k4 < ke; k4 += REC_RES_UNROLL) {
            unsigned vs[REC_RES_UNROLL];                           // (the loads of REC_RES_UNROLL frames are in flight together)
#pragma unroll
            for (int u = 0; u < REC_RES_UNROLL; u++)
                vs[u] = dw_ok && k4 + u < ke ? *(const unsigned *)(d_rec_frame(g.b, g.chunks, k4 + u) + 4 * (size_t)dw) : 0u;
#pragma unroll
            for (int u = 0; u < REC_RES_UNROLL; u++) {
                const int k = k4 + u;
                if (k >= ke) break;
                const unsigned v = vs[u];
                const int *tr = g.traces + (size_t)k * g.L;
                unsigned o = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    int m = 0;
                    if (nls > 0) {
                        long long acc = 0;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            if (j < nls) {
                                const unsigned e = i == 0 ? lay[j].x : i == 1 ? lay[j].y : i == 2 ? lay[j].z : lay[j].w;
                                acc += (long long)(e & 0xFFFFu) * (long long)tr[e >> 16];
                            }
                        }
                        m = (int)((acc + (1ll << 23)) >> 24);      // |acc| < 2^50: m fits 27 bits
                    }
                    const int r = g.offset + (int)((v >> (8 * i)) & 255u) - m;
                    if ((live >> (8 * i)) & 1u) {
                        clip += r < 0 || r > 255;
                        o |= (unsigned)min(255, max(0, r)) << (8 * i);
                    }
                }
                if (dw_ok) *(unsigned *)(g.out + (size_t)(k - g.k0) * g.b.fs + 4 * (size_t)dw) = o;
            }
        }
    }
    if (g.clipped == nullptr) return;
    const unsigned long long all = d_wave_sum64((unsigned long long)clip);   // (a lane's count: 4 x 2^24 frames at most)
    if (lane == 0 && all > 0) atomicAdd(g.clipped, all);
}
