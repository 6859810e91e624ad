// Full-depth traces (hm_deep_body_*, include/hydra_mi.h): the 16-bit frames of a run pulled back
// through the tracked mesh by k_body_warp's own rule (body_kernels.h, d_body_px), either at the pixels of a set of columns
// alone (k_deep_cols: the sparse readout, sums of weight x value in exact 64-bit integers) or at every pixel
// (k_body_warp16: the registered planes).  deep.hip alone compiles this header.  tests/deeptrace_ref.py restates all of it.
#pragma once
#include "hm_types.h"

#define DEEP_COL_WAVES 4               // waves of a workgroup of k_deep_cols: one piece of one frame each

struct DeepWarp {
    int n, W, H;                       // pixels, frame size
    int swap;                          // 1: the two bytes of a texel are exchanged at the gather
    const int *tri_of;                 // the body map of the filter handle (BodyMapView)
    const double2 *bary;
    const int4 *tidx;
    const double *X;                   // the run's states, frame k at X + k xstride; 2N positions are read of each
    size_t xstride;
    const uint16_t *frames;            // the run's frames, dense: frame k at frames + k n
};

// d_body_px with 16-bit texels: the same position, the same bilinear sample, the same rint; 0..65535
__device__ __forceinline__ unsigned d_deep_px(const DeepWarp &a, const double *__restrict__ X,
                                              const uint16_t *__restrict__ frame, int t, double2 l)
{
    if (t < 0) return 0u;
    const int4 v = a.tidx[t];
    const double x0 = X[2 * v.x], y0 = X[2 * v.x + 1];
    const double x1 = X[2 * v.y], y1 = X[2 * v.y + 1];
    const double x2 = X[2 * v.z], y2 = X[2 * v.z + 1];
    const double x = (x0 + l.x * (x1 - x0)) + l.y * (x2 - x0);
    const double y = (y0 + l.x * (y1 - y0)) + l.y * (y2 - y0);
    if (!(d_coord_ok(x) && d_coord_ok(y))) return 0u;
    const double u = x - 0.5, w = y - 0.5;
    const double fc = floor(u), fr = floor(w);
    const double ax = u - fc, b = w - fr;
    const int c0 = (int)fc, r0 = (int)fr;
    const int ca = min(max(c0, 0), a.W - 1), cb = min(max(c0 + 1, 0), a.W - 1);
    const int ra = min(max(r0, 0), a.H - 1), rb = min(max(r0 + 1, 0), a.H - 1);
    unsigned t00 = frame[ra * a.W + ca], t01 = frame[ra * a.W + cb];
    unsigned t10 = frame[rb * a.W + ca], t11 = frame[rb * a.W + cb];
    if (a.swap) {
        t00 = (t00 >> 8) | ((t00 & 255u) << 8); t01 = (t01 >> 8) | ((t01 & 255u) << 8);
        t10 = (t10 >> 8) | ((t10 & 255u) << 8); t11 = (t11 >> 8) | ((t11 & 255u) << 8);
    }
    const double f00 = t00, f01 = t01, f10 = t10, f11 = t11;
    const double val = (1.0 - b) * ((1.0 - ax) * f00 + ax * f01) + b * ((1.0 - ax) * f10 + ax * f11);
    return (unsigned)rint(val);
}

// A piece of a column: entries start .. start + len - 1 of pix / wt.  A column of at most "deep_col_entries" entries is
// one piece (an empty column too: len 0); a longer one is cut into pieces of that many, marked split.
struct DeepPiece {
    long long start;
    int len;
    int col;                           // the column; bit 31: one of several pieces, which meet in an atomic
};
#define DEEP_PIECE_SPLIT 0x80000000u

// The sparse readout.  Grid (pieces / DEEP_COL_WAVES, frames of the run): a wave takes one piece of one frame and strides
// through its entries, 64 at a time; per entry the map's triangle and barycentrics at the entry's pixel, three vertices
// of that frame's X and four texels.  Weight x value (< 2^32) and the wave's sum are 64-bit.  Lane 0 writes the sum of a
// whole column with one plain 8-byte store; the pieces of a split column add theirs to a word the caller has zeroed, with
// a 64-bit integer atomic -- integer sums, so the bytes do not depend on the order or on where the column was cut.
// sums: frames x C, frame k's at sums + k C.
__global__ __launch_bounds__(64 * DEEP_COL_WAVES) void k_deep_cols(DeepWarp a, int npieces, int C,
                                                                    const DeepPiece *__restrict__ pieces,
                                                                    const int *__restrict__ pix, const uint16_t *__restrict__ wt,
                                                                    unsigned long long *__restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const int pc = blockIdx.x * DEEP_COL_WAVES + (threadIdx.x >> 6);       // (the same in every lane of a wave)
    if (pc >= npieces) return;
    const int k = blockIdx.y;
    const DeepPiece piece = pieces[pc];
    const double *X = a.X + (size_t)k * a.xstride;
    const uint16_t *frame = a.frames + (size_t)k * (size_t)a.n;
    unsigned long long acc = 0ull;
    for (int e = lane; e < piece.len; e += 64) {
        const int p = pix[piece.start + e];
        const unsigned v = d_deep_px(a, X, frame, a.tri_of[p], a.bary[p]);
        acc += (unsigned long long)wt[piece.start + e] * (unsigned long long)v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) {
        const unsigned col = (unsigned)piece.col;
        unsigned long long *dst = sums + (size_t)k * (size_t)C + (col & ~DEEP_PIECE_SPLIT);
        if (col & DEEP_PIECE_SPLIT) atomicAdd(dst, acc);
        else *dst = acc;
    }
}

// The registered planes: k_body_warp's shape -- grid (blocks, frames of the run), 4 pixels a thread -- without sums.
// out: frame k's plane at out + k n, 0 outside the map; the four values go out as one 8-byte store where their address
// is a multiple of 8 (with an odd n every other frame's plane starts 2 bytes off), else as four 2-byte stores.
__global__ __launch_bounds__(256) void k_body_warp16(DeepWarp a, uint16_t *__restrict__ out)
{
    const int p0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (p0 >= a.n) return;
    const int k = blockIdx.y;
    const double *X = a.X + (size_t)k * a.xstride;
    const uint16_t *frame = a.frames + (size_t)k * (size_t)a.n;
    uint16_t *o = out + (size_t)k * (size_t)a.n + p0;
    const bool whole = p0 + 4 <= a.n;
    int key[4] = {-1, -1, -1, -1};
    unsigned val[4] = {0u, 0u, 0u, 0u};
    if (whole) {
        const int4 t = *(const int4 *)(a.tri_of + p0);
        key[0] = t.x; key[1] = t.y; key[2] = t.z; key[3] = t.w;
    } else {
        for (int j = 0; j < 4; j++)
            if (p0 + j < a.n) key[j] = a.tri_of[p0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (key[j] >= 0) val[j] = d_deep_px(a, X, frame, key[j], a.bary[p0 + j]);
    if (whole && ((uintptr_t)o & 7) == 0) {
        *(uint2 *)o = make_uint2(val[0] | (val[1] << 16), val[2] | (val[3] << 16));
    } else {
        for (int j = 0; j < 4 && p0 + j < a.n; j++) o[j] = (uint16_t)val[j];
    }
}
