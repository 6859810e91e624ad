// Residual motion of the kept registered video, found and taken out on the device (hm_body_rec_match / _frame_sums /
// _shift; hydra_mi/stabilize.py; tests/stab_ref.py restates all of it in NumPy).  DESIGN.md section 13.
//
// Patches of B x B box pixels tile the record's box from its top-left corner (the last column and row may be narrower),
// row-major.  The core of a patch is its pixels p for which every p + d, |dx| <= S and |dy| <= S, is in the map: the
// host marks it (one byte per box pixel, rows `pitch` apart), so every shift of a patch sums over the same pixels.
#pragma once
#include "roi_kernels.h"

#define STAB_BMIN 4
#define STAB_BMAX 64
#define STAB_SMAX 8                    // the widest search: |dx|, |dy| <= 8
#define STAB_DMAX 16                   // the largest shift applied

// dwords per row of a patch's template, and of its window: the window starts at the 4-byte boundary at or below the
// patch's first column - S (up to 3 bytes further left), and a shifted dword is put together from two neighbours
__host__ __device__ inline int stab_tw(int B) { return (B + 3) >> 2; }
__host__ __device__ inline int stab_ww(int B, int S) { return ((B + 2 * S + 6) >> 2) + 1; }
// row groups a shift's sum is split into: shifts x groups fill the 256 threads where they can
__host__ __device__ inline int stab_groups(int B, int S)
{
    const int nsh = (2 * S + 1) * (2 * S + 1), g = 256 / nsh;
    return g < 1 ? 1 : (g > B ? B : g);
}
__host__ __device__ inline size_t stab_lds_bytes(int B, int S)
{
    const int nsh = (2 * S + 1) * (2 * S + 1);
    return sizeof(unsigned) * ((size_t)2 * B * stab_tw(B) + (size_t)(B + 2 * S) * stab_ww(B, S) + (size_t)3 * nsh * stab_groups(B, S));
}

// c + sum of the four byte products of a and b
__device__ __forceinline__ unsigned d_dot4(unsigned a, unsigned b, unsigned c)
{
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) +
           (a >> 24) * (b >> 24);
#endif
}

struct StabMatch {
    RecBox b;
    const uint8_t *const *chunks;
    int W;                             // the frame's width: the template's rows
    int k0, F, tpf;                    // first frame, frames, frames per run
    int B, S, npx, np;                 // patch edge, search radius, patches per row, patches
    const uint8_t *tmpl;               // W x H, body coordinates
    const uint8_t *core;               // pitch x bh: 1 on core pixels
    unsigned *A, *V1, *V2;             // F x np x (2S + 1)^2; any may be NULL
};

// One workgroup per patch (blockIdx.x) and run of tpf frames (blockIdx.y strides over the runs).  The patch's template
// and core mask are packed four pixels to a dword in LDS once (0 off the core); per frame the (B + 2S)-row window is
// staged with aligned dword reads of the record, and a thread takes one shift and one group of patch rows: per four
// pixels one dword of the window put together from two neighbours and three byte dot products,
//   A += w . t,  V1 += w . m,  V2 += (w & 255 m) . w        (m: 1 on the core)
// The groups' partial sums meet in LDS in a fixed order; one slot of the output per (frame, patch, shift), no atomics.
// 255^2 64^2 < 2^32: every sum is exact.
__global__ __launch_bounds__(256) void k_stab_match(StabMatch g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned stab_lds[];
    const int B = g.B, S = g.S, n1 = 2 * S + 1, nsh = n1 * n1;
    const int tw = stab_tw(B), ww = stab_ww(B, S), G = stab_groups(B, S);
    unsigned *t4 = stab_lds, *m4 = t4 + B * tw, *win = m4 + B * tw, *part = win + (B + 2 * S) * ww;
    const int patch = blockIdx.x, py = patch / g.npx, px = patch - py * g.npx;
    const int x0 = px * B, y0 = py * B, pw = min(B, g.b.bw - x0), ph = min(B, g.b.bh - y0);
    const int a0 = (x0 - S) - ((x0 - S) & 3), off = x0 - S - a0;          // the window's first column, a multiple of 4
    const int twp = (pw + 3) >> 2, wh = ph + 2 * S, rpg = (ph + G - 1) / G;
    for (int i = threadIdx.x; i < B * tw; i += 256) {
        const int y = i / tw, q = i - y * tw;
        unsigned t = 0, m = 0;
        if (y < ph)
            for (int j = 0; j < 4; j++) {
                const int x = 4 * q + j;
                if (x < pw && g.core[(size_t)(y0 + y) * g.b.pitch + x0 + x]) {
                    m |= 1u << (8 * j);
                    t |= (unsigned)g.tmpl[(size_t)(g.b.r0 + y0 + y) * g.W + g.b.c0 + x0 + x] << (8 * j);
                }
            }
        t4[i] = t;
        m4[i] = m;
    }
    const int runs = (g.F + g.tpf - 1) / g.tpf;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {            // (the same trips for the whole workgroup)
        const int j0 = run * g.tpf, m = min(g.tpf, g.F - j0);
        for (int j = j0; j < j0 + m; j++) {
            const uint8_t *f = d_rec_frame(g.b, g.chunks, g.k0 + j);
            __syncthreads();                                              // the frame before has been read (first: t4, m4 are written)
            for (int i = threadIdx.x; i < wh * ww; i += 256) {
                const int r = i / ww, y = y0 - S + r, c = a0 + 4 * (i - r * ww);
                win[i] = y >= 0 && y < g.b.bh && c >= 0 && c < g.b.pitch ? *(const unsigned *)(f + (size_t)y * g.b.pitch + c) : 0u;
            }
            __syncthreads();
            for (int it = threadIdx.x; it < nsh * G; it += 256) {
                const int gi = it / nsh, s = it - gi * nsh, sdy = s / n1, sdx = s - sdy * n1;
                const int bo = sdx + off, sh = 8 * (bo & 3), qo = bo >> 2;
                const int ya = gi * rpg, yb = min(ph, ya + rpg);
                unsigned a = 0, v1 = 0, v2 = 0;
                for (int y = ya; y < yb; y++) {
                    const unsigned *wr = win + (y + sdy) * ww + qo, *tr = t4 + y * tw, *mr = m4 + y * tw;
                    for (int q = 0; q < twp; q++) {
                        const unsigned mm = mr[q];
                        if (!mm) continue;
                        const unsigned w = (unsigned)(((unsigned long long)wr[q + 1] << 32 | wr[q]) >> sh);
                        a = d_dot4(w, tr[q], a);
                        v1 = d_dot4(w, mm, v1);
                        v2 = d_dot4(w & (mm * 255u), w, v2);
                    }
                }
                part[3 * it] = a;
                part[3 * it + 1] = v1;
                part[3 * it + 2] = v2;
            }
            __syncthreads();
            for (int s = threadIdx.x; s < nsh; s += 256) {
                unsigned a = 0, v1 = 0, v2 = 0;
                for (int gi = 0; gi < G; gi++) {
                    const unsigned *p = part + 3 * (gi * nsh + s);
                    a += p[0]; v1 += p[1]; v2 += p[2];
                }
                const size_t o = ((size_t)j * g.np + patch) * nsh + s;
                if (g.A) g.A[o] = a;
                if (g.V1) g.V1[o] = v1;
                if (g.V2) g.V2[o] = v2;
            }
        }
    }
}

struct StabSum {
    RecBox b;
    const uint8_t *const *chunks;
    int W, k0, F;
    int B, npx, np;                    // (unused without shifts)
    const int *tri_of;
    const int8_t *shifts;              // F x np x 2 (dx, dy), or NULL: no shift
    unsigned *out;                     // W x H, zeroed by the caller
};

// out[p] = sum over the frames of v_k(p + d_k,patch(p)) for the map pixels p of the box, a thread per pixel; a source
// off the box counts 0 (off the map the record holds 0).  The host has refused F 255 >= 2^32.
__global__ __launch_bounds__(256) void k_stab_frame_sums(StabSum g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.b.bw * g.b.bh) return;
    const int y = i / g.b.bw, x = i - y * g.b.bw;
    const size_t p = (size_t)(g.b.r0 + y) * g.W + g.b.c0 + x;
    if (g.tri_of[p] < 0) return;
    const int8_t *sh = g.shifts ? g.shifts + 2 * (size_t)((y / g.B) * g.npx + x / g.B) : nullptr;
    unsigned sum = 0;
    for (int j = 0; j < g.F; j++) {
        int xs = x, ys = y;
        if (sh) {
            xs += sh[(size_t)j * g.np * 2];
            ys += sh[(size_t)j * g.np * 2 + 1];
        }
        if (xs >= 0 && xs < g.b.bw && ys >= 0 && ys < g.b.bh) sum += d_rec_frame(g.b, g.chunks, g.k0 + j)[(size_t)ys * g.b.pitch + xs];
    }
    g.out[p] = sum;
}

struct StabShift {
    RecBox b;
    int W, B, npx, np, frames;         // frames: of this run
    const int *tri_of;
    const int8_t *shifts;              // of the run's first frame on: frames x np x 2
    const uint8_t *src;                // the run's frames as they were (a copy)
    uint8_t *dst;                      // the run's frames in the record
};

// dst_k(p) = src_k(p + d_k,patch(p)) where p is in the map and p + d in the box, else 0 (padding included); a dword of
// the record per thread, blockIdx.y strides over the run's frames.
__global__ __launch_bounds__(256) void k_stab_shift(StabShift g)
{
    const int q = blockIdx.x * 256 + threadIdx.x, per_row = g.b.pitch >> 2;
    if (q >= per_row * g.b.bh) return;
    const int y = q / per_row, x = 4 * (q - y * per_row);
    int patch[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int xx = x + e;
        patch[e] = xx < g.b.bw && g.tri_of[(size_t)(g.b.r0 + y) * g.W + g.b.c0 + xx] >= 0 ? (y / g.B) * g.npx + xx / g.B : -1;
    }
    for (int j = blockIdx.y; j < g.frames; j += gridDim.y) {
        const uint8_t *f = g.src + (size_t)j * g.b.fs;
        unsigned w = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (patch[e] < 0) continue;
            const int8_t *sh = g.shifts + 2 * ((size_t)j * g.np + patch[e]);
            const int xs = x + e + sh[0], ys = y + sh[1];
            if (xs >= 0 && xs < g.b.bw && ys >= 0 && ys < g.b.bh) w |= (unsigned)f[(size_t)ys * g.b.pitch + xs] << (8 * e);
        }
        *(unsigned *)(g.dst + (size_t)j * g.b.fs + (size_t)y * g.b.pitch + x) = w;
    }
}

// ---- the smooth sub-pixel field (hm_body_rec_warp / _field_sums; tests/stabfield_ref.py) ------------------------------
// The shift of a (frame, patch) in 1/16 px and its validity, one dword: dx + 256 in bits 0..9, dy + 256 in bits 10..19,
// valid in bit 20 (the host packs it while it checks the range).
#define STAB_QMAX 256
__host__ __device__ inline unsigned stab_pack(int dx, int dy, int valid)
{
    return (unsigned)(dx + STAB_QMAX) | (unsigned)(dy + STAB_QMAX) << 10 | (valid ? 1u << 20 : 0u);
}

// One axis of the field at box coordinate x of a grid of n patches: the lower of the two patches the pixel lies between
// and the weight w1 of the upper one, min(i + 1, n - 1), out of 2B (the lower one has 2B - w1).  Patch i is centred at
// u = 2x + 1 - B = 2B i; the field is constant below the first centre and above the last.
__device__ __forceinline__ void d_stab_axis(int x, int B, int n, int &i, int &w1)
{
    const int u = 2 * x + 1 - B;
    i = u < 0 ? 0 : min(u / (2 * B), max(n - 2, 0));
    w1 = min(max(u - 2 * B * i, 0), 2 * B);
}

struct StabField {
    int p00, p01, p10, p11;            // the four patches (iy | iy1, ix | ix1)
    int w00, w01, w10, w11;            // their weights wy wx, which sum to 4 B^2 <= 16384
};

__device__ __forceinline__ StabField d_stab_field(int iy, int wy1, int ix, int wx1, int B, int npx, int npy)
{
    const int iy1 = min(iy + 1, npy - 1), ix1 = min(ix + 1, npx - 1), wy0 = 2 * B - wy1, wx0 = 2 * B - wx1;
    StabField f;
    f.p00 = iy * npx + ix; f.p01 = iy * npx + ix1; f.p10 = iy1 * npx + ix; f.p11 = iy1 * npx + ix1;
    f.w00 = wy0 * wx0; f.w01 = wy0 * wx1; f.w10 = wy1 * wx0; f.w11 = wy1 * wx1;
    return f;
}

// The shift of a pixel in 1/16 px from the four packed (q, valid) of its patches: per component
// floor((2 num + den) / (2 den)), num = sum w q, den = sum w over the valid ones; (0, 0) when none is valid.  With q + 256
// in place of q the numerator is not negative (w <= 16384, q + 256 <= 512, four terms: below 2^25), so the floor is the
// unsigned quotient, less 256.
__device__ __forceinline__ void d_stab_shift_at(const StabField &f, unsigned a, unsigned b, unsigned c, unsigned d, int &dx, int &dy)
{
    const unsigned wa = (a >> 20 & 1u) * f.w00, wb = (b >> 20 & 1u) * f.w01, wc = (c >> 20 & 1u) * f.w10, wd = (d >> 20 & 1u) * f.w11;
    const unsigned den = wa + wb + wc + wd;
    dx = dy = 0;
    if (!den) return;
    const unsigned nx = wa * (a & 1023u) + wb * (b & 1023u) + wc * (c & 1023u) + wd * (d & 1023u);
    const unsigned ny = wa * (a >> 10 & 1023u) + wb * (b >> 10 & 1023u) + wc * (c >> 10 & 1023u) + wd * (d >> 10 & 1023u);
    dx = (int)((2 * nx + den) / (2 * den)) - STAB_QMAX;
    dy = (int)((2 * ny + den) / (2 * den)) - STAB_QMAX;
}

// v'(p): the frame f (rows `pitch` apart, a box of bw x bh) sampled bilinearly at (16 x + dx, 16 y + dy) / 16; a source
// off the box counts 0
__device__ __forceinline__ unsigned d_stab_sample(const uint8_t *f, const RecBox &b, int x, int y, int dx, int dy)
{
    const int X = 16 * x + dx, Y = 16 * y + dy, x0 = X >> 4, y0 = Y >> 4, fx = X & 15, fy = Y & 15;
    const bool cx0 = x0 >= 0 && x0 < b.bw, cx1 = x0 + 1 >= 0 && x0 + 1 < b.bw;
    unsigned v00 = 0, v01 = 0, v10 = 0, v11 = 0;
    if (y0 >= 0 && y0 < b.bh) {
        const uint8_t *r = f + (size_t)y0 * b.pitch;
        if (cx0) v00 = r[x0];
        if (cx1) v01 = r[x0 + 1];
    }
    if (y0 + 1 >= 0 && y0 + 1 < b.bh) {
        const uint8_t *r = f + (size_t)(y0 + 1) * b.pitch;
        if (cx0) v10 = r[x0];
        if (cx1) v11 = r[x0 + 1];
    }
    return ((16 - fx) * (16 - fy) * v00 + fx * (16 - fy) * v01 + (16 - fx) * fy * v10 + fx * fy * v11 + 128) >> 8;
}

struct StabWarp {
    RecBox b;
    int W, B, npx, npy, np, frames;    // frames: of this run
    const int *tri_of;
    const unsigned *qv;                // of the run's first frame on: frames x np packed (q, valid)
    const uint8_t *src;                // the run's frames as they were (a copy)
    uint8_t *dst;                      // the run's frames in the record
};

// dst_k(p) = src_k sampled at the field of frame k where p is in the map, else 0 (padding included); a dword of the
// record per thread, blockIdx.y strides over the run's frames.  The patches and weights of the thread's four pixels do
// not depend on the frame; neighbouring pixels between the same two patch columns share the four loads of the field.
__global__ __launch_bounds__(256) void k_stab_warp(StabWarp g)
{
    const int q = blockIdx.x * 256 + threadIdx.x, per_row = g.b.pitch >> 2;
    if (q >= per_row * g.b.bh) return;
    const int y = q / per_row, x = 4 * (q - y * per_row);
    int iy, wy1, ix[4], wx1[4];
    bool in[4];
    d_stab_axis(y, g.B, g.npy, iy, wy1);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int xx = x + e;
        in[e] = xx < g.b.bw && g.tri_of[(size_t)(g.b.r0 + y) * g.W + g.b.c0 + xx] >= 0;
        d_stab_axis(xx, g.B, g.npx, ix[e], wx1[e]);
    }
    for (int j = blockIdx.y; j < g.frames; j += gridDim.y) {
        const uint8_t *f = g.src + (size_t)j * g.b.fs;
        const unsigned *qv = g.qv + (size_t)j * g.np;
        unsigned w = 0, a = 0, b = 0, c = 0, d = 0;
        int have = -1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (!in[e]) continue;
            const StabField fl = d_stab_field(iy, wy1, ix[e], wx1[e], g.B, g.npx, g.npy);
            if (ix[e] != have) {
                a = qv[fl.p00]; b = qv[fl.p01]; c = qv[fl.p10]; d = qv[fl.p11];
                have = ix[e];
            }
            int dx, dy;
            d_stab_shift_at(fl, a, b, c, d, dx, dy);
            w |= d_stab_sample(f, g.b, x + e, y, dx, dy) << (8 * e);
        }
        *(unsigned *)(g.dst + (size_t)j * g.b.fs + (size_t)y * g.b.pitch + x) = w;
    }
}

struct StabFieldSum {
    RecBox b;
    const uint8_t *const *chunks;
    int W, k0, F;
    int B, npx, npy, np;
    const int *tri_of;
    const unsigned *qv;                // F x np packed (q, valid)
    unsigned *out;                     // W x H, zeroed by the caller
};

// out[p] = sum over the frames of v'_k(p), the frame sampled at its field, for the map pixels p of the box, a thread per
// pixel.  The host has refused F 255 >= 2^32.
__global__ __launch_bounds__(256) void k_stab_field_sums(StabFieldSum g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.b.bw * g.b.bh) return;
    const int y = i / g.b.bw, x = i - y * g.b.bw;
    const size_t p = (size_t)(g.b.r0 + y) * g.W + g.b.c0 + x;
    if (g.tri_of[p] < 0) return;
    int iy, wy1, ix, wx1;
    d_stab_axis(y, g.B, g.npy, iy, wy1);
    d_stab_axis(x, g.B, g.npx, ix, wx1);
    const StabField fl = d_stab_field(iy, wy1, ix, wx1, g.B, g.npx, g.npy);
    unsigned sum = 0;
    for (int j = 0; j < g.F; j++) {
        const unsigned *qv = g.qv + (size_t)j * g.np;
        int dx, dy;
        d_stab_shift_at(fl, qv[fl.p00], qv[fl.p01], qv[fl.p10], qv[fl.p11], dx, dy);
        sum += d_stab_sample(d_rec_frame(g.b, g.chunks, g.k0 + j), g.b, x, y, dx, dy);
    }
    g.out[p] = sum;
}
