// Plain types, constants and __device__ inline helpers that more than one translation unit of libhydra_mi.so needs: what
// the filter handle (ctx.h) holds by value, and what kernels on both sides of the filter / readout split use.  No
// __global__ function lives here, so any translation unit may include it -- unlike the *_kernels.h headers, whose kernels
// are not static: each of those is compiled by exactly one translation unit (the Makefile lists them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// ---- the rasteriser's triangle setup and coverage rules (kernels: ekf_kernels.h, body_kernels.h) -------------------

#define EKF_SUB 256
#define EKF_MAX_STAR 24        // triangles around one vertex
#define EKF_TILE 16
#define EKF_MAX_TRI 4096

struct TriSetup {              // one triangle in one configuration
    // edge function E_k = ea*c + eb*r + ec at pixel (col c, row r).  Whole numbers kept as doubles:
    // for coordinates within +-2^24 px every product and sum stays below 2^53, so binary64 evaluates
    // them exactly -- the same values as 64-bit integers at the cost of two full-rate v_fma_f64
    // (64-bit integer multiplies are built from quarter-rate 32-bit ones on gfx950).
    double ea[3], eb[3], ec[3];
    // ec + (1 if a zero edge value counts as inside, the top-left rule): E is a whole number, so
    // "E > 0 or (E == 0 and top-left)" is the single comparison ea*c + eb*r + ecb > 0
    double ecb[3];
    int cmin, cmax, rmin, rmax;  // pixel bounding box (inclusive), empty if cmin > cmax (16-byte aligned: one scalar load)
    int tl[3];                 // 1 if a zero edge value counts as inside (top-left edge)
    float inv;                 // 1 / (2 area)
    int i0, i1, i2;            // vertex ids after orientation normalisation
    // attributes of the three vertices in that order: texture coordinates (pixels of the initial
    // frame) and the two velocity render attributes vx, -vy.  Kept here so that a covered pixel
    // needs no dependent global loads besides its texel.
    float ux[3], uy[3], ax[3], ay[3];
};

__device__ __forceinline__ void d_tri_attr(TriSetup &s, const float *__restrict__ uv, const double *__restrict__ X, int N)
{
    const int id[3] = {s.i0, s.i1, s.i2};
    for (int k = 0; k < 3; k++) {
        s.ux[k] = uv[2 * id[k]];
        s.uy[k] = uv[2 * id[k] + 1];
        s.ax[k] = (float)X[2 * N + 2 * id[k]];
        s.ay[k] = (float)(-X[2 * N + 2 * id[k] + 1]);
    }
}

__device__ __forceinline__ long long d_snap(double x) { return (long long)rint(x * (double)EKF_SUB); }

// Pixel bounding box (inclusive) of the triangle with snapped integer positions, as d_tri_setup keeps it: empty
// (cmin > cmax) for a degenerate or out-of-range triangle.  One function for every caller: a tile that asks "can
// this triangle reach me" gets the answer the setup itself would give.
__device__ __forceinline__ bool d_tri_sane(long long x0, long long y0, long long x1, long long y1, long long x2, long long y2)
{
    const long long lim = (long long)1 << 32;     // 2^24 px in 1/256 px units: the exact range of the edge functions
    return x0 > -lim && x0 < lim && y0 > -lim && y0 < lim && x1 > -lim && x1 < lim && y1 > -lim && y1 < lim &&
           x2 > -lim && x2 < lim && y2 > -lim && y2 < lim;
}
__device__ __forceinline__ void d_tri_bbox(long long x0, long long y0, long long x1, long long y1, long long x2, long long y2,
                                           int W, int H, int &cmin, int &cmax, int &rmin, int &rmax)
{
    cmin = 1; cmax = 0; rmin = 1; rmax = 0;
    const long long area = d_tri_sane(x0, y0, x1, y1, x2, y2) ? (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) : 0;
    if (area == 0) return;
    long long xmin = x0 < x1 ? (x0 < x2 ? x0 : x2) : (x1 < x2 ? x1 : x2);
    long long xmax = x0 > x1 ? (x0 > x2 ? x0 : x2) : (x1 > x2 ? x1 : x2);
    long long ymin = y0 < y1 ? (y0 < y2 ? y0 : y2) : (y1 < y2 ? y1 : y2);
    long long ymax = y0 > y1 ? (y0 > y2 ? y0 : y2) : (y1 > y2 ? y1 : y2);
    // floor division by 256 (arithmetic shift), as in the oracle
    long long cl = (xmin - 128) >> 8, ch = ((xmax - 128) >> 8) + 1;
    long long rl = (ymin - 128) >> 8, rh = ((ymax - 128) >> 8) + 1;
    if (cl < 0) cl = 0;
    if (rl < 0) rl = 0;
    if (ch > W - 1) ch = W - 1;
    if (rh > H - 1) rh = H - 1;
    cmin = (int)cl; cmax = (int)ch; rmin = (int)rl; rmax = (int)rh;
}

// Build the setup of triangle (v0,v1,v2) with snapped integer positions p[3][2].
__device__ inline void d_tri_setup(TriSetup &s, int v0, int v1, int v2, long long x0, long long y0,
                                   long long x1, long long y1, long long x2, long long y2, int W, int H)
{
    s.cmin = 1; s.cmax = 0; s.rmin = 1; s.rmax = 0;
    const bool sane = d_tri_sane(x0, y0, x1, y1, x2, y2);
    long long area = sane ? (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) : 0;
    s.i0 = v0; s.i1 = v1; s.i2 = v2;
    s.inv = 0.0f;
    for (int k = 0; k < 3; k++) { s.ea[k] = 0.0; s.eb[k] = 0.0; s.ec[k] = -1.0; s.ecb[k] = -1.0; s.tl[k] = 0; }
    if (area == 0) return;
    d_tri_bbox(x0, y0, x1, y1, x2, y2, W, H, s.cmin, s.cmax, s.rmin, s.rmax);      // (the box does not depend on the orientation)
    if (area < 0) {
        long long t;
        t = x1; x1 = x2; x2 = t;
        t = y1; y1 = y2; y2 = t;
        s.i1 = v2; s.i2 = v1;
        area = -area;
    }
    // E0: edge 1->2 (weight of vertex 0), E1: edge 2->0, E2: edge 0->1
    const long long ex[3] = {x2 - x1, x0 - x2, x1 - x0};
    const long long ey[3] = {y2 - y1, y0 - y2, y1 - y0};
    const long long ox[3] = {x1, x2, x0};
    const long long oy[3] = {y1, y2, y0};
    for (int k = 0; k < 3; k++) {
        // E(px,py) = ex*(py-oy) - ey*(px-ox), px = 256 c + 128, py = 256 r + 128
        s.ea[k] = (double)(-ey[k] * EKF_SUB);
        s.eb[k] = (double)(ex[k] * EKF_SUB);
        s.ec[k] = (double)(ex[k] * (128 - oy[k]) - ey[k] * (128 - ox[k]));
        s.tl[k] = (ey[k] > 0) || (ey[k] == 0 && ex[k] < 0);
        s.ecb[k] = s.ec[k] + (double)s.tl[k];
    }
    s.inv = 1.0f / (float)area;
}

// coverage of the pixel centre (dc, dr) without the bounding-box shortcut and without branches (for
// pixels inside the frame the three edge tests imply the box); barycentrics separately
__device__ __forceinline__ bool d_tri_cover(const TriSetup &s, double dc, double dr)
{
    const double e0 = fma(s.ea[0], dc, fma(s.eb[0], dr, s.ecb[0]));
    const double e1 = fma(s.ea[1], dc, fma(s.eb[1], dr, s.ecb[1]));
    const double e2 = fma(s.ea[2], dc, fma(s.eb[2], dr, s.ecb[2]));
    return (e0 > 0.0) & (e1 > 0.0) & (e2 > 0.0);
}
// the same, handing back the values of edges 1 and 2 (with the top-left bias in: ecb): the barycentrics of a covered pixel
// follow from them by taking the bias out again -- whole numbers below 2^53, so e - bias IS ea c + eb r + ec, exactly
__device__ __forceinline__ bool d_tri_cover2(const TriSetup &s, double dc, double dr, double &e1, double &e2)
{
    const double e0 = fma(s.ea[0], dc, fma(s.eb[0], dr, s.ecb[0]));
    e1 = fma(s.ea[1], dc, fma(s.eb[1], dr, s.ecb[1]));
    e2 = fma(s.ea[2], dc, fma(s.eb[2], dr, s.ecb[2]));
    return (e0 > 0.0) & (e1 > 0.0) & (e2 > 0.0);
}
__device__ __forceinline__ void d_tri_bary2(const TriSetup &s, double e1, double e2, float &l1, float &l2)
{
    l1 = (float)(e1 - (s.tl[1] ? 1.0 : 0.0)) * s.inv;
    l2 = (float)(e2 - (s.tl[2] ? 1.0 : 0.0)) * s.inv;
}
__device__ __forceinline__ void d_tri_bary(const TriSetup &s, double dc, double dr, float &l1, float &l2)
{
    l1 = (float)fma(s.ea[1], dc, fma(s.eb[1], dr, s.ec[1])) * s.inv;
    l2 = (float)fma(s.ea[2], dc, fma(s.eb[2], dr, s.ec[2])) * s.inv;
}

// coverage + barycentrics of pixel (c, r)
__device__ __forceinline__ bool d_tri_eval(const TriSetup &s, int c, int r, float &l1, float &l2)
{
    if (c < s.cmin || c > s.cmax || r < s.rmin || r > s.rmax) return false;
    const double dc = (double)c, dr = (double)r;
    const double e0 = fma(s.ea[0], dc, fma(s.eb[0], dr, s.ec[0]));      // exact: see TriSetup
    const double e1 = fma(s.ea[1], dc, fma(s.eb[1], dr, s.ec[1]));
    const double e2 = fma(s.ea[2], dc, fma(s.eb[2], dr, s.ec[2]));
    bool in = (e0 > 0 || (e0 == 0 && s.tl[0])) && (e1 > 0 || (e1 == 0 && s.tl[1])) &&
              (e2 > 0 || (e2 == 0 && s.tl[2]));
    if (!in) return false;
    l1 = (float)e1 * s.inv;
    l2 = (float)e2 * s.inv;
    return true;
}

__device__ __forceinline__ float d_lerp(float a0, float a1, float a2, float l1, float l2)
{
    return (a0 + l1 * (a1 - a0)) + l2 * (a2 - a0);
}

// offset of the nearest texel in the initial frame
__device__ __forceinline__ int d_texel_at(const TriSetup &s, float l1, float l2, int W, int H)
{
    float tx = d_lerp(s.ux[0], s.ux[1], s.ux[2], l1, l2);
    float ty = d_lerp(s.uy[0], s.uy[1], s.uy[2], l1, l2);
    int cx = (int)floorf(tx), cy = (int)floorf(ty);
    cx = cx < 0 ? 0 : (cx > W - 1 ? W - 1 : cx);
    cy = cy < 0 ? 0 : (cy > H - 1 ? H - 1 : cy);
    return cy * W + cx;
}
__device__ __forceinline__ int d_texel(const uint8_t *__restrict__ tex, const TriSetup &s, float l1, float l2, int W,
                                       int H)
{
    return tex[d_texel_at(s, l1, l2, W, H)];
}

struct Mesh {
    int W, H, N, T;
    const int *tri;           // T*3
    const float *uv;          // N*2
    const uint8_t *tex;       // W*H
};

// unclamped render targets: im = min(255, acc), m = cnt > 0 ? 255 : 0
struct Targets {
    int *acc;                 // sum of texels
    float *fx, *fy;           // sums of interpolated vx, -vy
    int *cnt;                 // covering triangles
};

// ---- the pool of parked difference images (layout and kernels: ekf_kernels.h) -------------------------------------
struct DPool {
    int *hdr;                 // N x 4: c0, r0, rw, rh of the region (all multiples of 8)
    int *live;                // one word per tile of the pool (cap / 64)
    const int *area;          // N region areas (k_star_regions); a region's offset is the sum of those before it
    short2 *xi, *yi;          // (image, mask) numerators of D_{v,x} and D_{v,y}
    float *xfx, *xfy, *yfx, *yfy, *vxfx, *vyfy;
    long long cap;            // pixels in the pool
    int *overflow;            // set to 1 if the regions do not fit
};

#define RI_H 16                        // strip height of the default launch (hm_ctx_tune "render_rows": 16 or 8)

// ---- what the measurement (ekf_kernels.h: ekf.hip) hands to the dense update (dense_kernels.h, chol_flow_kernels.h: update.hip) ----
#define MEAS_OUT 40                    // doubles of one workgroup's job sums (ekf_kernels.h has the layout)
#define MEAS_VSPLIT_MAX 16             // most workgroups per vertex job (their partial sums are added in order)
// vertex job output layout (doubles): only the non-zero terms are accumulated, and only in the
// combinations KFState.update uses -- 19 sums per thread instead of 38 keep the kernel under 128
// VGPRs (four waves per SIMD):
enum {
    // jz, plus minus minus (the central difference of kalman.py:499-515 is linear in the sums): x and y
    // per channel (Hzc wants the components), vx only has an fx term, vy only an fy term
    A_X = 0, A_Y = 4, A_VX = 8, A_VY = 9,
    // self block of HTH (forward differences): the four channels already weighted by 1/eps and added
    A_XX = 10, A_XY = 11, A_YY = 12,
    A_XVX = 13, A_YVX = 14,               // fx channel only (not weighted)
    A_XVY = 15, A_YVY = 16,               // fy channel only
    A_VXVX = 17, A_VYVY = 18,
    A_NV = 19
};
enum {
    // edge job (v,w): D_v,a * D_w,b
    B_XX = 0, B_XY = 1, B_YX = 2, B_YY = 3,        // geometry x geometry: channels weighted by 1/eps and added
    B_XVX = 4, B_YVX = 5, B_VXX = 6, B_VXY = 7, B_VXVX = 8,        // fx channel (not weighted)
    B_XVY = 9, B_YVY = 10, B_VYX = 11, B_VYY = 12, B_VYVY = 13,    // fy channel
    B_NV = 14
};
#define PREP_MAX_ENTRIES (4 * (EKF_MAX_STAR + 2))      // most terms of a row of the system (k_solve_prep)
#define RES_HEAD 10                    // doubles behind the step in a result block (k_iter_result)
#define RI_GROUPS 256
#define RI_NV 6               // image, flow x, flow y, mask terms against `o`, then flow x, flow y against the raw flow

// The RI_NV error sums from the per-strip partials of k_render_iter, in a fixed order: thread g of RI_GROUPS adds the partials g,
// g + RI_GROUPS, ... in ascending order, then the group sums are added in ascending order (hm_tile_partial_sums on
// the host does the same additions).  sp: RI_GROUPS x RI_NV doubles of LDS; out[0..RI_NV-1] written by threads
// 0..RI_NV-1 after a barrier inside.
__device__ __forceinline__ void d_tile_partial_sums(const double *__restrict__ partial, int ntiles, double *sp, double *out)
{
    const int t = threadIdx.x;
    if (t < RI_GROUPS) {
        double s[RI_NV];
#pragma unroll
        for (int k = 0; k < RI_NV; k++) s[k] = 0.0;
#pragma unroll 4
        for (int i = t; i < ntiles; i += RI_GROUPS) {
            const double2 *q = (const double2 *)(partial + RI_NV * (size_t)i);
#pragma unroll
            for (int k = 0; k < RI_NV / 2; k++) { const double2 v = q[k]; s[2 * k] += v.x; s[2 * k + 1] += v.y; }
        }
#pragma unroll
        for (int k = 0; k < RI_NV; k++) sp[RI_NV * t + k] = s[k];
    }
    __syncthreads();
    if (t < RI_NV) {
        double s = 0.0;
        for (int g = 0; g < RI_GROUPS; g++) s += sp[RI_NV * g + t];
        out[t] = s;
    }
}

// ---- the dense f64 algebra (kernels: dense_kernels.h, chol_flow_kernels.h in update.hip; smooth_kernels.h in smooth.hip) ----
#define DNB 32          // block size

// the accumulator of v_mfma_f64_16x16x4_f64 (dense_kernels.h has the layout)
typedef double d4_t __attribute__((ext_vector_type(4)));

// One 16x16 tile of X Y for 32x32 blocks X, Y in LDS on the f64 matrix cores (v_mfma_f64_16x16x4_f64, eight k-steps):
// wave wv computes tile (wv >> 1, wv & 1); element e of the result sits at row 16 (wv >> 1) + (lane >> 4) + 4 e, column
// 16 (wv & 1) + (lane & 15).  (X Y^T: d_mfma_nt, dense_kernels.h)
__device__ __forceinline__ d4_t d_mfma_nn(double (*X)[DNB + 1], double (*Y)[DNB + 1], int wv, int lane, d4_t c)
{
    const int i = 16 * (wv >> 1) + (lane & 15), j = 16 * (wv & 1) + (lane & 15), kq = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < DNB / 4; kk++)
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(X[i][4 * kk + kq], Y[4 * kk + kq][j], c, 0, 0, 0);
    return c;
}
// the same for X^T Y
__device__ __forceinline__ d4_t d_mfma_tn(double (*X)[DNB + 1], double (*Y)[DNB + 1], int wv, int lane, d4_t c)
{
    const int i = 16 * (wv >> 1) + (lane & 15), j = 16 * (wv & 1) + (lane & 15), kq = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < DNB / 4; kk++)
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(X[4 * kk + kq][i], Y[4 * kk + kq][j], c, 0, 0, 0);
    return c;
}

// the springs of every vertex, as the covariance prediction's kernels read them (k_fw_rows / k_pft_cols, dense_kernels.h)
struct SpringTopo {
    const int *off;           // N+1: springs of each vertex
    const int *bar;           // spring id
    const int *other;         // the vertex at the other end
    const double *blk;        // I x 3: Bxx, Bxy, Byy
};

// the factorisation as one persistent launch (k_flow_fill / k_chol_flow, chol_flow_kernels.h)
struct FlowArgs {
    const double *A;          // n x n matrix (+ right-hand-side rows up to nrows), read only
    double *L;                // nrows x n: blocks below the block diagonal
    double *Lt;               // nb x 32 x 32: T_c
    double *Tinv;             // n x n: L^-1
    double *P;                // 3 x nb x 32 x 32: block (c, c-1) before its triangular solve; Q_c; block (c, c-2) likewise (Y_c)
    int n, nrows, nb, nbr;    // nbr: block rows including the right-hand-side rows
    unsigned *ctl;            // [0] next task, [1] set when a wait timed out
    int stall;                // test knob (hm_ctx_tune "chol_flow_stall"): the chain sleeps ~4 us x stall before every diagonal block
};

// ---- working arrays of the mask's contour pruning (project_kernels.h) ------------------------------------------------
struct Ccl {
    int *L;          // W*H: labels (pixel indices)
    int *cnt;        // W*H, used at roots: pixels inside or on the component's contour
    int *bnd;        // W*H, used at roots: boundary points of the contour (object: pixels 4-adjacent to the outside;
                     // hole: pixels of the enclosing object 4-adjacent to it)
    uint8_t *edge;   // W*H, used at background roots: 1 = reaches the frame edge
    unsigned long long *best;     // [0]: (2 A << 32) | ~root of the best level-0 object so far
    int W, H;
};

// ---- the body-frame readout and the kept record (body_kernels.h; roi_kernels.h and the record's other kernels) -------
// most frames of one statistics accumulation: 65536 * 255^2 < 2^32, every sum is an exact uint32
#define BODY_STATS_CAP 65536

// Sums of val over the lanes of a wave by key, NK keys per lane (-1: none), one integer atomic per distinct key: the
// first lane with a key left names it, the lanes add what they hold under it, a wave reduction, the atomic.  Exact and
// independent of the order.  Every lane of the wave must call it (a wave's sum of at most 64 NK values of <= 255 fits
// 32 bits).
template <int NK, typename S>
__device__ __forceinline__ void d_peel_add(const int (&key)[NK], const unsigned (&val)[NK], S *__restrict__ sums)
{
    unsigned pend = 0;
#pragma unroll
    for (int j = 0; j < NK; j++)
        if (key[j] >= 0) pend |= 1u << j;
    const int lane = __lane_id();
    for (;;) {
        const unsigned long long act = __ballot(pend != 0);
        if (act == 0) break;
        const int lead = __ffsll((unsigned long long)act) - 1;
        int mine = -1;
#pragma unroll
        for (int j = NK - 1; j >= 0; j--)
            if ((pend >> j) & 1u) mine = key[j];
        const int k = __shfl(mine, lead);
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < NK; j++)
            if (((pend >> j) & 1u) && key[j] == k) { s += val[j]; pend &= ~(1u << j); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (unsigned)__shfl_xor((int)s, o);
        if (lane == lead) atomicAdd(&sums[k], (S)s);
    }
}

// A coordinate of a diverged state: beyond +-2^20 px (or not finite) a segment is not drawn (view_kernels.h) and a body
// pixel reads as 0 (body_kernels.h d_body_px, deeptrace_kernels.h d_deep_px: one rule, one helper)
#define VIEW_COORD_MAX 1048576.0
__device__ __forceinline__ bool d_coord_ok(double a) { return a >= -VIEW_COORD_MAX && a <= VIEW_COORD_MAX; }

// What hm_deep_body_* (deep.hip) borrows of a filter handle: its device and sizes and the finished body map, which stay
// the filter handle's.  body_map_view (readout.hip) waits for the handle's helper, builds the map on first use -- that
// ends with the handle's stream idle, so the map is whole for any stream from then on -- and changes nothing else.
struct BodyMapView {
    int device, W, H, N, T;
    const int *tri;                    // triangle per pixel (W*H), -1: none
    const double2 *bary;
    const int4 *tidx;                  // vertex ids per triangle
    int col_entries;                   // hm_ctx_tune "deep_col_entries"
};
#define DEEP_COL_ENTRIES_MIN 64        // hm_ctx_tune "deep_col_entries": one stride of a wave at least
#define DEEP_COL_ENTRIES_MAX (1 << 30) // ... and a column's most entries at most (never split)
struct hm_ctx;
__attribute__((visibility("hidden"))) int body_map_view(hm_ctx *h, BodyMapView *v);

// the box of the body map that the record keeps per frame (roi_kernels.h has the layout)
struct RecBox {
    int c0, r0, bw, bh;                // the box in the frame: columns c0 .. c0 + bw - 1, rows r0 .. r0 + bh - 1
    int pitch, fpc;                    // bytes per row, frames per chunk
    size_t fs;                         // bytes per frame
};
#define REC_TP_MAX 1024                // the most frames of a workgroup's run (hm_ctx_tune "rec_tp_frames")
#define REC_BL_MAX (1 << 24)           // the most frames of a run of k_rec_running (hm_ctx_tune "rec_bl_frames"; REC_MAX_FRAMES)
#define REC_RES_MAX (1 << 24)          // the most frames of a run of k_rec_residual (hm_ctx_tune "rec_res_frames"; REC_MAX_FRAMES)
#define REC_MAP_MAX 256                // the most frames of a run of k_rec_trace_maps (hm_ctx_tune "rec_map_frames"): 32-bit sums hold
#define REC_NULL_MAX 256               // the most frames of a run of k_rec_trace_null (hm_ctx_tune "rec_null_frames"): 255 x 32767 x 256 < 2^31
#define REC_WV_MAX 65535               // the most events of a launch of k_rec_wv_lat (hm_ctx_tune "rec_wv_frames"): its blockIdx.y
#define REC_TM_MAX 256                 // the most frames of a run of k_rec_tri_maps (hm_ctx_tune "rec_tm_frames"): 255 x 32767 x 256 < 2^31
// hm_body_rec_gram: the most frames of one Gram matrix (G is 8192^2 x 8 bytes = 512 MiB there), and the most bytes of a run of
// k_rec_gram (hm_ctx_tune "rec_gram_bytes", multiples of 64).  The run's 32-bit sums hold products of signed bytes x = v - 128,
// |x_i x_j| <= 128^2: 128^2 x 131008 = 2 146 435 072 < 2^31, while 131072 bytes would be exactly 2^31 and a black frame (x = -128
// everywhere) against itself reaches the bound.
#define REC_GRAM_MAX 8192
#define REC_GRAM_BYTES_MAX 131008
#define REC_RES_LMAX 65536             // hm_body_rec_residual_*: a label 0 .. L - 1 shares a dword with its 16-bit weight
