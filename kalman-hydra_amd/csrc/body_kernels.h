// The body-frame readout: frames pulled back through the tracked mesh into the coordinates of its texture (the frame-0
// pixel grid of the initial vertices), with sums of the registered values over triangles and over caller labels.
//
// The body map (k_body_map, once per handle): every pixel (r, c) takes the lowest-indexed triangle of the mesh at
// X = uv whose coverage -- the render's rule, snapped positions, exact integer edge functions at the pixel centre,
// top-left ties -- includes it, or -1, and its barycentrics l1 = e1 / area, l2 = e2 / area as correctly rounded binary64
// divisions of whole numbers (the vertex order after the render's orientation swap).
// The warp (k_body_warp, per frame): the pixel's position in frame k, x = (X[i0] + l1 (X[i1] - X[i0])) + l2 (X[i2] - X[i0])
// in binary64 (the library builds with -ffp-contract=off), a bilinear sample of the frame at (x - 0.5, y - 0.5) with the
// texels clamped to the frame, rint half to even; 0 outside the map or for a position that is not finite or beyond
// +-2^20 px.  tests/body_ref.py restates all of it in NumPy.
#pragma once
#include "hm_types.h"
#include "view_kernels.h"

// X = uv (binary32 promoted), velocities 0: the configuration the body map is taken at
__global__ __launch_bounds__(256) void k_body_uvX(const float *__restrict__ uv, int N, double *__restrict__ X)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * N) X[i] = i < 2 * N ? (double)uv[i] : 0.0;
}

// One 16 x 16 tile per workgroup, the triangles binned as in k_render and visited in ascending order: the first that
// covers the pixel is its triangle.  Writes the triangle per pixel (-1: none), its barycentrics, the pixels per triangle
// (cnt, zeroed by the caller), and -- workgroup (0, 0) -- the vertex ids of every triangle in the setup's order.
__global__ __launch_bounds__(EKF_TILE *EKF_TILE) void k_body_map(int W, int H, int T, const TriSetup *__restrict__ setup,
                                                                 int *__restrict__ tri_of, double2 *__restrict__ bary,
                                                                 int4 *__restrict__ tidx, unsigned *__restrict__ cnt)
{
    __shared__ unsigned s_mask[EKF_MAX_TRI / 32];
    const int tid = threadIdx.y * EKF_TILE + threadIdx.x;
    const int words = (T + 31) / 32;
    for (int i = tid; i < words; i += EKF_TILE * EKF_TILE) s_mask[i] = 0;
    __syncthreads();
    const int c0 = blockIdx.x * EKF_TILE, r0 = blockIdx.y * EKF_TILE;
    for (int t = tid; t < T; t += EKF_TILE * EKF_TILE) {
        const TriSetup &s = setup[t];
        if (s.cmin <= s.cmax && s.cmax >= c0 && s.cmin < c0 + EKF_TILE && s.rmax >= r0 && s.rmin < r0 + EKF_TILE)
            atomicOr(&s_mask[t >> 5], 1u << (t & 31));
        if (blockIdx.x == 0 && blockIdx.y == 0) tidx[t] = make_int4(s.i0, s.i1, s.i2, 0);
    }
    __syncthreads();
    const int c = c0 + threadIdx.x, r = r0 + threadIdx.y;
    int found = -1;
    if (c < W && r < H) {
        const double dc = (double)c, dr = (double)r;
        double2 l = make_double2(0.0, 0.0);
        for (int wd = 0; wd < words && found < 0; wd++) {
            unsigned bits = s_mask[wd];
            while (bits) {
                const int b = __ffs(bits) - 1;
                bits &= bits - 1;
                const TriSetup &s = setup[wd * 32 + b];
                double e1, e2;
                if (!d_tri_cover2(s, dc, dr, e1, e2)) continue;
                // whole numbers below 2^53 throughout (TriSetup): the edge values without the top-left bias and their
                // sum, which is the area of the swapped vertex order, are exact
                e1 -= s.tl[1] ? 1.0 : 0.0;
                e2 -= s.tl[2] ? 1.0 : 0.0;
                const double e0 = fma(s.ea[0], dc, fma(s.eb[0], dr, s.ec[0]));
                const double area = (e0 + e1) + e2;
                l = make_double2(e1 / area, e2 / area);
                found = wd * 32 + b;
                break;
            }
        }
        const int p = r * W + c;
        tri_of[p] = found;
        bary[p] = l;
    }
    const int key[1] = {found};
    const unsigned one[1] = {1u};
    d_peel_add(key, one, cnt);
}

// pixels per label: labels of pixels of the map (-1 and pixels outside the map count nowhere); cnt zeroed by the caller
__global__ __launch_bounds__(256) void k_body_label_count(const int *__restrict__ tri_of, const int *__restrict__ labels, int n,
                                                          unsigned *__restrict__ cnt)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int key[1] = {p < n && tri_of[p] >= 0 ? labels[p] : -1};
    const unsigned one[1] = {1u};
    d_peel_add(key, one, cnt);
}

struct BodyWarpArgs {
    int n, W, H, ch;                   // pixels, frame size, output channels (1, or 3: B = G = R)
    const int *tri_of;                 // the body map
    const double2 *bary;
    const int4 *tidx;                  // vertex ids per triangle
    const double *X;                   // positions of frame k (2N)
    const uint8_t *frame;              // frame k, W x H
    const int *labels;                 // the label image (W x H, -1: none), NULL: no label sums
    uint8_t *out;                      // n x ch, NULL: sums only
    uint8_t *reg;                      // n, the plane k_body_stats_add reads; NULL: no statistics
    unsigned long long *tsum, *lsum;   // sums per triangle / per label (zeroed by the caller), NULL: none
};

__device__ __forceinline__ unsigned d_body_px(const BodyWarpArgs &a, int t, double2 l)
{
    if (t < 0) return 0u;
    const int4 v = a.tidx[t];
    const double x0 = a.X[2 * v.x], y0 = a.X[2 * v.x + 1];
    const double x1 = a.X[2 * v.y], y1 = a.X[2 * v.y + 1];
    const double x2 = a.X[2 * v.z], y2 = a.X[2 * v.z + 1];
    const double x = (x0 + l.x * (x1 - x0)) + l.y * (x2 - x0);
    const double y = (y0 + l.x * (y1 - y0)) + l.y * (y2 - y0);
    if (!(d_coord_ok(x) && d_coord_ok(y))) return 0u;
    const double u = x - 0.5, w = y - 0.5;
    const double fc = floor(u), fr = floor(w);
    const double ax = u - fc, b = w - fr;
    const int c0 = (int)fc, r0 = (int)fr;
    const int ca = min(max(c0, 0), a.W - 1), cb = min(max(c0 + 1, 0), a.W - 1);
    const int ra = min(max(r0, 0), a.H - 1), rb = min(max(r0 + 1, 0), a.H - 1);
    const double f00 = a.frame[ra * a.W + ca], f01 = a.frame[ra * a.W + cb];
    const double f10 = a.frame[rb * a.W + ca], f11 = a.frame[rb * a.W + cb];
    const double val = (1.0 - b) * ((1.0 - ax) * f00 + ax * f01) + b * ((1.0 - ax) * f10 + ax * f11);
    return (unsigned)rint(val);
}

// one gather per pixel, 4 pixels per thread; the region sums in the same pass.  No thread leaves before the sums: the
// peeling loop needs every lane of its wave.
__global__ __launch_bounds__(256) void k_body_warp(BodyWarpArgs a)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int p0 = 4 * q;
    int key[4] = {-1, -1, -1, -1};
    unsigned val[4] = {0u, 0u, 0u, 0u};
    const bool whole = p0 + 4 <= a.n;
    if (whole) {
        const int4 t = *(const int4 *)(a.tri_of + p0);
        key[0] = t.x; key[1] = t.y; key[2] = t.z; key[3] = t.w;
    } else {
        for (int j = 0; j < 4; j++)
            if (p0 + j < a.n) key[j] = a.tri_of[p0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (key[j] >= 0) val[j] = d_body_px(a, key[j], a.bary[p0 + j]);
    if (a.out) {
        if (whole && a.ch == 1) {
            *(unsigned *)(a.out + p0) = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
        } else if (whole) {            // B = G = R: 12 bytes as three dwords
            unsigned *o = (unsigned *)(a.out + 12 * (size_t)q);
            o[0] = val[0] * 0x010101u | (val[1] << 24);
            o[1] = val[1] * 0x0101u | (val[2] * 0x0101u << 16);
            o[2] = val[2] | (val[3] * 0x010101u << 8);
        } else {
            for (int j = 0; j < 4 && p0 + j < a.n; j++)
                for (int k = 0; k < a.ch; k++) a.out[(size_t)a.ch * (p0 + j) + k] = (uint8_t)val[j];
        }
    }
    if (a.reg) {
        if (whole) *(unsigned *)(a.reg + p0) = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
        else
            for (int j = 0; j < 4 && p0 + j < a.n; j++) a.reg[p0 + j] = (uint8_t)val[j];
    }
    if (a.tsum) d_peel_add(key, val, a.tsum);
    if (a.lsum) {
        int lab[4];
        if (whole) {
            const int4 t = *(const int4 *)(a.labels + p0);
            lab[0] = t.x; lab[1] = t.y; lab[2] = t.z; lab[3] = t.w;
        } else {
            for (int j = 0; j < 4; j++) lab[j] = p0 + j < a.n ? a.labels[p0 + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (key[j] < 0) lab[j] = -1;
        d_peel_add(lab, val, a.lsum);
    }
}

// ---- statistics of the registered video (hm_body_stats_*) -------------------------------------------------------------
// Integer sums over the frames added since hm_body_stats_begin, per pixel p of the map, v the registered value:
//   s1 = sum v(p), s2 = sum v(p)^2, cross[d] = sum v(p) v(p + d) for d = right, down-right, down, down-left (0 where
//   p + d is off the frame or outside the map), vmax = max v(p).
// Pixels outside the map are registered as 0 (k_body_warp), so a product with one is 0 without a look at the map, and
// their own sums stay 0.  At most BODY_STATS_CAP frames: 65536 * 255^2 < 2^32, every sum is an exact uint32.
// (BODY_STATS_CAP: hm_types.h)

struct BodyStats {
    unsigned *s1, *s2, *cross;         // n, n, 4 planes of n values `stride` apart; every plane 16-byte aligned
    size_t stride;
    uint8_t *vmax;                     // n
};

// 4 pixels per thread (p0 = 4 q, linear as in k_body_warp: they may straddle a row end when W is not a multiple of 4).
// Each pixel's sums belong to its thread alone: plain read-modify-write in 16-byte vectors.  A thread whose pixels are
// all outside the map loads its four map entries and nothing else.  reg: the registered plane the warp has just written.
__global__ __launch_bounds__(256) void k_body_stats_add(int n, int W, const int *__restrict__ tri_of,
                                                        const uint8_t *__restrict__ reg, BodyStats st)
{
    const int p0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (p0 >= n) return;
    const bool whole = p0 + 4 <= n;
    int t[4] = {-1, -1, -1, -1};
    if (whole) {
        const int4 k = *(const int4 *)(tri_of + p0);
        t[0] = k.x; t[1] = k.y; t[2] = k.z; t[3] = k.w;
    } else {
        for (int j = 0; j < 4 && p0 + j < n; j++) t[j] = tri_of[p0 + j];
    }
    if ((t[0] & t[1] & t[2] & t[3]) < 0) return;           // (all four negative)
    // a[j] = reg[p0 + j], j = 0..4; b[j] = reg[p0 + W - 1 + j], j = 0..5; 0 beyond the plane
    unsigned a[5], b[6];
    if (whole) {
        const unsigned w = *(const unsigned *)(reg + p0);
        a[0] = w & 255u; a[1] = (w >> 8) & 255u; a[2] = (w >> 16) & 255u; a[3] = w >> 24;
    } else {
        for (int j = 0; j < 4; j++) a[j] = p0 + j < n ? reg[p0 + j] : 0u;
    }
    a[4] = p0 + 4 < n ? reg[p0 + 4] : 0u;
    const int q0 = p0 + W;
    if ((W & 3) == 0 && q0 + 4 <= n) {
        const unsigned w = *(const unsigned *)(reg + q0);
        b[1] = w & 255u; b[2] = (w >> 8) & 255u; b[3] = (w >> 16) & 255u; b[4] = w >> 24;
    } else {
        for (int j = 1; j < 5; j++) b[j] = q0 - 1 + j < n ? reg[q0 - 1 + j] : 0u;
    }
    b[0] = q0 - 1 < n ? reg[q0 - 1] : 0u;
    b[5] = q0 + 4 < n ? reg[q0 + 4] : 0u;
    unsigned add[6][4];
    const int c0 = p0 % W;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int c = c0 + j;
        while (c >= W) c -= W;
        const unsigned v = a[j];                           // 0 outside the map and beyond the plane
        const bool right = c + 1 < W, left = c > 0;        // the row below exists where its index is < n: b is 0 there
        add[0][j] = v;
        add[1][j] = v * v;
        add[2][j] = right ? v * a[j + 1] : 0u;
        add[3][j] = right ? v * b[j + 2] : 0u;
        add[4][j] = v * b[j + 1];
        add[5][j] = left ? v * b[j] : 0u;
    }
    unsigned *plane[6] = {st.s1, st.s2, st.cross, st.cross + st.stride, st.cross + 2 * st.stride, st.cross + 3 * st.stride};
    if (whole) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            uint4 s = *(uint4 *)(plane[k] + p0);
            s.x += add[k][0]; s.y += add[k][1]; s.z += add[k][2]; s.w += add[k][3];
            *(uint4 *)(plane[k] + p0) = s;
        }
        const unsigned m = *(const unsigned *)(st.vmax + p0);
        *(unsigned *)(st.vmax + p0) = max(m & 255u, a[0]) | (max((m >> 8) & 255u, a[1]) << 8) |
                                      (max((m >> 16) & 255u, a[2]) << 16) | (max(m >> 24, a[3]) << 24);
    } else {
        for (int j = 0; j < 4 && p0 + j < n; j++) {
            for (int k = 0; k < 6; k++) plane[k][p0 + j] += add[k][j];
            st.vmax[p0 + j] = (uint8_t)max((unsigned)st.vmax[p0 + j], a[j]);
        }
    }
}

struct BodyImages {
    int n, W, H;
    double F;                          // frames added, >= 1
    const int *tri_of;
    BodyStats st;
    double *mean, *sd, *corr;          // n each; NaN outside the map
};

// The summary images, one pixel per thread, binary64, every step one correctly rounded operation in this order (the
// integers and their products F s2, s1^2, F cross, s1(p) s1(q) are below 2^53: exact):
//   var = F s2 - s1 s1;  mean = s1 / F;  std = sqrt(var) / F;
//   rho(p, q) = (F cross(p, q) - s1(p) s1(q)) / sqrt(var(p) var(q)) for the neighbours q in the frame and the map with
//   var(p) > 0 and var(q) > 0, in the order E, SE, S, SW, W, NW, N, NE (the last four from the sums stored at q);
//   corr = their sum in that order / their number, 0 when there is none.
__global__ __launch_bounds__(256) void k_body_stats_images(BodyImages g)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n) return;
    if (g.tri_of[p] < 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        g.mean[p] = nan; g.sd[p] = nan; g.corr[p] = nan;
        return;
    }
    const int r = p / g.W, c = p - r * g.W;
    const double s1 = (double)g.st.s1[p];
    const double var = g.F * (double)g.st.s2[p] - s1 * s1;
    g.mean[p] = s1 / g.F;
    g.sd[p] = sqrt(var) / g.F;
    double sum = 0.0;
    int cnt = 0;
    if (var > 0.0) {
        const int dc[8] = {1, 1, 0, -1, -1, -1, 0, 1}, dr[8] = {0, 1, 1, 1, 0, -1, -1, -1};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int cq = c + dc[k], rq = r + dr[k];
            if (cq < 0 || cq >= g.W || rq < 0 || rq >= g.H) continue;
            const int q = rq * g.W + cq;
            if (g.tri_of[q] < 0) continue;
            const double t1 = (double)g.st.s1[q];
            const double vq = g.F * (double)g.st.s2[q] - t1 * t1;
            if (!(vq > 0.0)) continue;
            const double x = (double)(k < 4 ? g.st.cross[k * g.st.stride + p] : g.st.cross[(k - 4) * g.st.stride + q]);
            sum += (g.F * x - s1 * t1) / sqrt(var * vq);
            cnt++;
        }
    }
    g.corr[p] = cnt ? sum / (double)cnt : 0.0;
}

struct BodyPeaks {
    int W, H, which, radius, cap;      // which: 0 corr, 1 std, 2 max - mean; 1 <= radius <= BODY_PEAK_RMAX
    double min_score;
    const int *tri_of;
    const double *mean, *sd, *corr;
    const uint8_t *vmax;
    int *count;                        // peaks found (zeroed by the caller)
    int *index;                        // cap entries: raster index, in the order the waves arrive
    double *score;
};

#define BODY_PEAK_RMAX 16
#define BODY_PEAK_TILE 16

// A map pixel p is a peak when score(p) >= min_score and no map pixel q != p of the (2 radius + 1)^2 window around it has
// score(q) > score(p), or score(q) == score(p) and a lower raster index.  One 16 x 16 tile per workgroup, its scores with
// a halo of `radius` staged in LDS -- NaN off the frame and outside the map, which loses every comparison --, the peaks
// compacted with one atomic per wave as k_outline does.
__global__ __launch_bounds__(BODY_PEAK_TILE *BODY_PEAK_TILE) void k_body_peaks(BodyPeaks g)
{
    constexpr int S = BODY_PEAK_TILE + 2 * BODY_PEAK_RMAX;
    __shared__ double s_sc[S * S];
    const int tid = threadIdx.y * BODY_PEAK_TILE + threadIdx.x;
    const int R = g.radius, side = BODY_PEAK_TILE + 2 * R;
    const int c0 = blockIdx.x * BODY_PEAK_TILE - R, r0 = blockIdx.y * BODY_PEAK_TILE - R;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < side * side; i += BODY_PEAK_TILE * BODY_PEAK_TILE) {
        const int lr = i / side, lc = i - lr * side;
        const int r = r0 + lr, c = c0 + lc;
        double s = nan;
        if (r >= 0 && r < g.H && c >= 0 && c < g.W) {
            const int q = r * g.W + c;
            if (g.tri_of[q] >= 0) s = g.which == 0 ? g.corr[q] : g.which == 1 ? g.sd[q] : (double)g.vmax[q] - g.mean[q];
        }
        s_sc[lr * S + lc] = s;
    }
    __syncthreads();
    const int c = c0 + R + threadIdx.x, r = r0 + R + threadIdx.y;
    const int lane = tid & 63;
    bool peak = false;
    double mine = 0.0;
    if (c < g.W && r < g.H && g.tri_of[r * g.W + c] >= 0) {
        mine = s_sc[(threadIdx.y + R) * S + threadIdx.x + R];
        peak = mine >= g.min_score;
        for (int dy = -R; dy <= R && peak; dy++) {
            const double *row = s_sc + (threadIdx.y + R + dy) * S + threadIdx.x + R;
            for (int dx = -R; dx <= R; dx++) {
                const double s = row[dx];
                // before p in raster order: an equal score wins as well
                if (dy < 0 || (dy == 0 && dx < 0) ? s >= mine : s > mine) peak = false;
            }
        }
    }
    const unsigned long long bo = __ballot(peak);
    if (!bo) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(g.count, __popcll(bo));
    base = __shfl(base, 0);
    const int slot = base + __popcll(bo & ((1ull << lane) - 1ull));
    if (peak && slot < g.cap) {
        g.index[slot] = r * g.W + c;
        g.score[slot] = mine;
    }
}
