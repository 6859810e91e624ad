// The tracker's views (reference renderer.py:344-373, 436-475, 595-628; kalman.py:638-674) and the flow preview of the
// flow tool (reference src/optical_flow_ext.cpp:172-281, 336-389) as kernels.  Every view is H x W x 3 uint8, B, G, R,
// rows top to bottom.  Everything below is exact integer or f64 arithmetic (the library builds with -ffp-contract=off),
// except atan2f in the colour wheel, so a NumPy restatement reproduces it bit for bit (tests/view_ref.py).
// The flow views (flowx, flowy) show floor(255 (p - min) / (max - min)) with min and max over the FINITE pixels of the
// plane: a pixel that is NaN or +-inf takes no part in them and shows 0; with no finite pixel, or max == min (-0 == +0),
// every pixel shows 0.  No conversion of a NaN or an infinity to an integer is ever formed.
#pragma once
#include "hm_common.h"
#include "hm_types.h"

#define VIEW_SEG_WAVE 64               // lanes per segment: a segment's pixels are spread over one wave
// (VIEW_COORD_MAX and d_coord_ok: hm_types.h -- segments with an end point beyond +-2^20 px are not drawn)

// pixel i (0..n) of the segment (x0, y0) -> (x0 + dx, y0 + dy), n = max(|dx|, |dy|): x0 + floor((2 i dx + n) / (2 n))
__device__ __forceinline__ long long d_floordiv(long long a, long long b)
{
    long long q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

template <typename F>
__device__ __forceinline__ void d_segment(long long x0, long long y0, long long x1, long long y1, int lane, int W, int H, F &&put)
{
    const long long dx = x1 - x0, dy = y1 - y0;
    const long long n = max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy);
    for (long long i = lane; i <= n; i += VIEW_SEG_WAVE) {
        const long long x = n ? x0 + d_floordiv(2 * i * dx + n, 2 * n) : x0;
        const long long y = n ? y0 + d_floordiv(2 * i * dy + n, 2 * n) : y0;
        if (x >= 0 && x < W && y >= 0 && y < H) put((int)y * W + (int)x);
    }
}

// The wireframe: the three edges of every triangle (interior edges twice, as the reference's outline buffer has them,
// renderer.py:595-605), end points rint(vertex), one wave per segment; every covered pixel counts one (integer atomics:
// the counts do not depend on the order).
__global__ __launch_bounds__(256) void k_view_wire(const int *__restrict__ tri, int T, const double *__restrict__ X, int W, int H,
                                                   unsigned *__restrict__ count)
{
    const int seg = blockIdx.x * (256 / VIEW_SEG_WAVE) + threadIdx.x / VIEW_SEG_WAVE;
    const int lane = threadIdx.x % VIEW_SEG_WAVE;
    if (seg >= 3 * T) return;
    const int t = seg / 3, k = seg % 3;
    const int a = tri[3 * t + k], b = tri[3 * t + (k + 1) % 3];
    const double ax = rint(X[2 * a]), ay = rint(X[2 * a + 1]), bx = rint(X[2 * b]), by = rint(X[2 * b + 1]);
    if (!(d_coord_ok(ax) && d_coord_ok(ay) && d_coord_ok(bx) && d_coord_ok(by))) return;
    d_segment((long long)ax, (long long)ay, (long long)bx, (long long)by, lane, W, H,
              [&](int p) { atomicAdd(&count[p], 1u); });
}

// min / max of a float plane as order-preserving unsigned keys (mm[0] = min key, mm[1] = max key).  A value that is not
// finite (NaN, +-inf: a diverged state's velocities) takes no part; with no finite value at all mm[0] > mm[1] stays.
__device__ __forceinline__ bool d_ffinite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ unsigned d_fkey(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float d_funkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void k_view_minmax(const float *__restrict__ p, int n, unsigned *__restrict__ mm)
{
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float v = p[i];
        if (!d_ffinite(v)) continue;
        const unsigned k = d_fkey(v);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

enum { VIEW_RAW = 0, VIEW_OVERLAY = 1, VIEW_TEXTURE = 2, VIEW_MASK = 3, VIEW_FLOWX = 4, VIEW_FLOWY = 5, VIEW_FORCES_BASE = 6 };

struct ViewArgs {
    int n, which;
    const int *acc, *cnt, *ids;        // the render's targets (ids: the mask palette's G, B as 256 G + B)
    const float *flow;                 // flowx / flowy: the plane, mm its min / max keys
    const unsigned *mm;
    const unsigned *wire;              // wireframe counts
    const uint8_t *obs;                // the observed frame (overlay)
    uint8_t *out;                      // n x 3, B G R
};

__device__ __forceinline__ unsigned d_sat(unsigned v) { return v > 255u ? 255u : v; }

__device__ __forceinline__ unsigned d_view_px(const ViewArgs &a, int p, float fmin, float fmax)
{
    unsigned b, g, r;
    const unsigned gray = d_sat((unsigned)max(a.acc[p], 0));
    const unsigned wire = a.wire ? a.wire[p] : 0u;
    const unsigned w = wire > 2u ? 256u : 128u * wire;
    switch (a.which) {
    case VIEW_RAW: b = g = r = gray; break;
    case VIEW_TEXTURE: b = d_sat(gray + w); g = r = gray; break;
    case VIEW_MASK: {
        const int id = a.ids[p];
        r = a.cnt[p] > 0 ? 255u : 0u;
        g = (unsigned)(id >> 8);
        b = d_sat((unsigned)(id & 255) + w);
        break;
    }
    case VIEW_FLOWX:
    case VIEW_FLOWY: {
        unsigned v = 0;
        const float f = a.flow[p];
        if (fmax != fmin && d_ffinite(f)) v = (unsigned)floor(255.0 * ((double)f - (double)fmin) / ((double)fmax - (double)fmin));
        b = g = r = v;
        break;
    }
    default: {                         // overlay; the forces start from it with every channel halved
        b = d_sat(w); g = gray; r = a.obs[p];
        if (a.which == VIEW_FORCES_BASE) { b >>= 1; g >>= 1; r >>= 1; }
    }
    }
    return b | (g << 8) | (r << 16);
}

// one pass over the image: 4 pixels (12 bytes, three dwords) per thread
__global__ __launch_bounds__(256) void k_view_compose(ViewArgs a)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int p0 = 4 * q;
    if (p0 >= a.n) return;
    float fmin = 0.0f, fmax = 0.0f;
    if (a.which == VIEW_FLOWX || a.which == VIEW_FLOWY) {
        if (a.mm[0] <= a.mm[1]) { fmin = d_funkey(a.mm[0]); fmax = d_funkey(a.mm[1]); }
    }
    if (p0 + 4 <= a.n) {
        const unsigned c0 = d_view_px(a, p0, fmin, fmax), c1 = d_view_px(a, p0 + 1, fmin, fmax);
        const unsigned c2 = d_view_px(a, p0 + 2, fmin, fmax), c3 = d_view_px(a, p0 + 3, fmin, fmax);
        uint3 v;
        v.x = c0 | (c1 << 24);
        v.y = (c1 >> 8) | (c2 << 16);
        v.z = (c2 >> 16) | (c3 << 8);
        unsigned *o = (unsigned *)(a.out + 12 * (size_t)q);
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    } else {
        for (int p = p0; p < a.n; p++) {
            const unsigned c = d_view_px(a, p, fmin, fmax);
            a.out[3 * (size_t)p] = (uint8_t)c;
            a.out[3 * (size_t)p + 1] = (uint8_t)(c >> 8);
            a.out[3 * (size_t)p + 2] = (uint8_t)(c >> 16);
        }
    }
}

// One layer of the force arrows (reference kalman.py:638-674 without the 2x upscale, thickness 1, no legend): arrow v
// from from[v] to from[v] + scale * vec[v] (vec NULL: to to[v]), end points truncated as C int() does; the head is two
// segments from the tip at +-45 degrees to the shaft, 0.1 of its length: tip + rint(K (dx -+ dy)), tip + rint(K (dy +- dx)),
// K = 0.1 sqrt(1/2), (dx, dy) = start - tip.  Three segments per arrow, one wave per segment; the layer's colour wins
// over what is below it (each layer is a launch of its own).
#define VIEW_HEAD_K 0.070710678118654752
__global__ __launch_bounds__(256) void k_view_arrows(const double *__restrict__ from, const double *__restrict__ to,
                                                     const double *__restrict__ vec, double scale, int N, int W, int H,
                                                     uchar3 colour, uint8_t *__restrict__ out)
{
    const int seg = blockIdx.x * (256 / VIEW_SEG_WAVE) + threadIdx.x / VIEW_SEG_WAVE;
    const int lane = threadIdx.x % VIEW_SEG_WAVE;
    if (seg >= 3 * N) return;
    const int v = seg / 3, k = seg % 3;
    const double sx = from[2 * v], sy = from[2 * v + 1];
    const double ex = vec ? sx + scale * vec[2 * v] : to[2 * v], ey = vec ? sy + scale * vec[2 * v + 1] : to[2 * v + 1];
    if (!(d_coord_ok(sx) && d_coord_ok(sy) && d_coord_ok(ex) && d_coord_ok(ey))) return;
    const long long x0 = (long long)sx, y0 = (long long)sy, x1 = (long long)ex, y1 = (long long)ey;
    long long ax = x0, ay = y0, bx = x1, by = y1;
    if (k > 0) {
        const double dx = (double)(x0 - x1), dy = (double)(y0 - y1);
        ax = x1; ay = y1;
        if (k == 1) { bx = x1 + (long long)rint(VIEW_HEAD_K * (dx - dy)); by = y1 + (long long)rint(VIEW_HEAD_K * (dy + dx)); }
        else { bx = x1 + (long long)rint(VIEW_HEAD_K * (dx + dy)); by = y1 + (long long)rint(VIEW_HEAD_K * (dy - dx)); }
    }
    d_segment(ax, ay, bx, by, lane, W, H, [&](int p) {
        out[3 * (size_t)p] = colour.x; out[3 * (size_t)p + 1] = colour.y; out[3 * (size_t)p + 2] = colour.z;
    });
}

// ---- the cell overlay (hm_view_cells*): what roi / demix know about the body, painted onto the moving animal ----------
// The inverse of k_body_warp: per pixel of the IMAGE at state X the body pixel under it, then that pixel's cells.  In this
// order (include/hydra_mi.h has the rules in full; tests/cellview_ref.py restates them in NumPy, bit for bit):
//   base      B = G = R = frame[r, c];
//   triangle  the lowest-indexed triangle that covers the pixel centre at X, by the render's rule (d_snap, d_tri_setup,
//             d_tri_cover2: nothing of it is restated here); skipped: area 0, a vertex that is not finite or outside
//             d_tri_sane.  l1 = e1 / area, l2 = e2 / area in binary64 as k_body_map forms them;
//   body pixel  (floor(bx), floor(by)), bx = (Ux[i0] + l1 (Ux[i1] - Ux[i0])) + l2 (Ux[i2] - Ux[i0]), U the binary32 uv
//             widened; none when not finite or off the frame;
//   layers    j = 0 .. n_layers - 1: s = labels[j][body pixel] >= 0: a = weights[j][body pixel] levels[s], D = 65535 * 255,
//             ch = (ch (D - a) + colour[s][ch] a + D / 2) / D in unsigned 64-bit integers;
//   outline   (CV_OUTLINE) an outline pixel of layer 0 (k_view_cell_outline) takes colour[s] outright;
//   wire      (CV_WIRE) B = min(255, B + 128 count) of k_view_wire.
// The markers are a launch of their own behind it (k_view_cell_marks).
//
// One CV_W x CV_H strip of the image per workgroup, four pixels per thread (column c0 + lane, rows r0 + wave + 4 j: a wave
// gathers along a row), as k_render_iter's strips: every thread tests its share of the triangles' boxes against the
// strip into an LDS bit set; the candidates -- in ascending index order, the rank among the set bits is the slot -- are set
// up CV_CAP at a time into LDS by the threads that tested them, and every pixel without a triangle yet walks the batch in
// order and keeps the first that covers it.  A strip with more candidates than CV_CAP takes more batches: there is no cap
// (the bit set holds EKF_MAX_TRI triangles, all a handle can have).  The strip's colours are then staged in LDS and written
// as whole dwords wherever a dword lies inside the strip's bytes of a row (3 CV_W = 192 bytes: 48 dwords when the row
// starts on one), single bytes at the two ends where it does not -- any W, no tail of the image treated apart.
#define CV_W 64
#define CV_H 16
#define CV_CAP 32                      // candidate triangles set up in LDS at a time
#define CV_MAX_LAYERS 4
#define CV_OUTLINE 1
#define CV_WIRE 2
#define CV_ROW_WORDS (3 * CV_W / 4 + 1)     // most dwords that 3 CV_W bytes starting anywhere touch

struct CellViewArgs {
    int W, H, T, n_layers, flags, tiles_x;      // T 0: no cells set (markers over the frame)
    const int *tri;
    const float *uv;
    const double *X;                   // 2N positions
    const uint8_t *frame;              // W x H gray
    const int *labels;                 // n_layers planes of W*H, -1: none
    const uint16_t *weights;           // the same planes, NULL: 65535 everywhere
    const uint8_t *colours;            // L x 3, B G R
    const uint8_t *levels;             // L, NULL: 255 everywhere
    const uint8_t *outline;            // W*H: 1 on the outline pixels of layer 0
    const unsigned *wire;              // wireframe counts (CV_WIRE)
    uint8_t *out;                      // W*H*3, 4-byte aligned
};

struct CellShared {
    unsigned mask[EKF_MAX_TRI / 32];
    TriSetup cand[CV_CAP];
    unsigned px[CV_H][CV_W];           // B | G << 8 | R << 16
};

// a vertex the snap may take: finite and within the range d_tri_sane accepts (anything beyond fails that test anyway)
__device__ __forceinline__ bool d_cv_vertex_ok(double x, double y) { return fabs(x) <= 16777216.0 && fabs(y) <= 16777216.0; }

// The two ends of a strip's workgroup, shared with k_view_strain (strain_kernels.h); all 256 threads call them.
// The candidates of the strip at (c0, r0) into the bit set `mask` (LDS, cleared here): every thread tests its share of the
// triangles' boxes at X; a triangle with a vertex the snap may not take is no candidate.
__device__ __forceinline__ void d_cv_candidates(unsigned *mask, int T, const int *__restrict__ tri, const double *__restrict__ X,
                                                int W, int H, int c0, int r0)
{
    const int tid = threadIdx.x;
    const int words = (T + 31) / 32;
    for (int i = tid; i < words; i += 256) mask[i] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const int v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
        const double x0 = X[2 * v0], y0 = X[2 * v0 + 1], x1 = X[2 * v1], y1 = X[2 * v1 + 1], x2 = X[2 * v2], y2 = X[2 * v2 + 1];
        if (!(d_cv_vertex_ok(x0, y0) && d_cv_vertex_ok(x1, y1) && d_cv_vertex_ok(x2, y2))) continue;
        int cmin, cmax, rmin, rmax;
        d_tri_bbox(d_snap(x0), d_snap(y0), d_snap(x1), d_snap(y1), d_snap(x2), d_snap(y2), W, H, cmin, cmax, rmin, rmax);
        if (cmin <= cmax && cmax >= c0 && cmin < c0 + CV_W && rmax >= r0 && rmin < r0 + CV_H)
            atomicOr(&mask[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
}

// The strip's colours px (LDS, B | G << 8 | R << 16; a barrier since they were written) into out: the strip's bytes of row r
// are [3 (r W + c0), + 3 wv); whole dwords inside them as dwords, the ends byte by byte.
__device__ __forceinline__ void d_cv_store(const unsigned (&px)[CV_H][CV_W], int W, int H, int c0, int r0, uint8_t *__restrict__ out)
{
    const int wv = min(CV_W, W - c0), hv = min(CV_H, H - r0), nb = 3 * wv;
    for (int i = threadIdx.x; i < hv * CV_ROW_WORDS; i += 256) {
        const int rr = i / CV_ROW_WORDS, k = i - rr * CV_ROW_WORDS;
        const size_t b0 = 3 * ((size_t)(r0 + rr) * W + c0);
        const size_t start = ((b0 >> 2) + k) << 2;
        if (start >= b0 + nb) continue;
        unsigned v = 0, in = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const long long rel = (long long)(start + q) - (long long)b0;
            if (rel < 0 || rel >= nb) continue;
            const int pi = (int)rel / 3, cq = (int)rel - 3 * pi;
            v |= ((px[rr][pi] >> (8 * cq)) & 255u) << (8 * q);
            in |= 1u << q;
        }
        if (in == 15u) *(unsigned *)(out + start) = v;
        else
            for (int q = 0; q < 4; q++)
                if ((in >> q) & 1u) out[start + q] = (uint8_t)(v >> (8 * q));
    }
}

__global__ __launch_bounds__(256) void k_view_cells(CellViewArgs a)
{
    __shared__ CellShared sh;
    const int tid = threadIdx.x;
    const int words = (a.T + 31) / 32;
    const int c0 = ((int)blockIdx.x % a.tiles_x) * CV_W, r0 = ((int)blockIdx.x / a.tiles_x) * CV_H;
    const double *__restrict__ X = a.X;
    d_cv_candidates(sh.mask, a.T, a.tri, X, a.W, a.H, c0, r0);
    int total = 0;
    for (int w = 0; w < words; w++) total += __popc(sh.mask[w]);
    const int c = c0 + (tid & 63), rb = r0 + (tid >> 6);
    constexpr int NPX = CV_W * CV_H / 256;
    int bp[NPX];                       // the body pixel, -1: none; -2: no triangle found yet
#pragma unroll
    for (int j = 0; j < NPX; j++) bp[j] = -2;
    for (int base = 0; base < total; base += CV_CAP) {
        const int nch = min(CV_CAP, total - base);
        for (int tb = tid; tb < a.T; tb += 256) {
            const unsigned word = sh.mask[tb >> 5], bit = 1u << (tb & 31);
            if (!(word & bit)) continue;
            int rank = __popc(word & (bit - 1u));
            for (int w = 0; w < (tb >> 5); w++) rank += __popc(sh.mask[w]);
            if (rank < base || rank >= base + nch) continue;
            const int v0 = a.tri[3 * tb], v1 = a.tri[3 * tb + 1], v2 = a.tri[3 * tb + 2];
            TriSetup su;
            d_tri_setup(su, v0, v1, v2, d_snap(X[2 * v0]), d_snap(X[2 * v0 + 1]), d_snap(X[2 * v1]), d_snap(X[2 * v1 + 1]),
                        d_snap(X[2 * v2]), d_snap(X[2 * v2 + 1]), a.W, a.H);
            const int id[3] = {su.i0, su.i1, su.i2};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                su.ux[k] = a.uv[2 * id[k]]; su.uy[k] = a.uv[2 * id[k] + 1];
                su.ax[k] = 0.0f; su.ay[k] = 0.0f;
            }
            sh.cand[rank - base] = su;
        }
        __syncthreads();
        if (c < a.W)
            for (int q = 0; q < nch; q++) {                // ascending triangle order
                const TriSetup &su = sh.cand[q];
#pragma unroll
                for (int j = 0; j < NPX; j++) {
                    const int r = rb + 4 * j;
                    if (bp[j] != -2 || r >= a.H || c < su.cmin || c > su.cmax || r < su.rmin || r > su.rmax) continue;
                    const double dc = (double)c, dr = (double)r;
                    double e1, e2;
                    if (!d_tri_cover2(su, dc, dr, e1, e2)) continue;
                    // as k_body_map: whole numbers below 2^53, the area of the swapped order is their exact sum
                    e1 -= su.tl[1] ? 1.0 : 0.0;
                    e2 -= su.tl[2] ? 1.0 : 0.0;
                    const double e0 = fma(su.ea[0], dc, fma(su.eb[0], dr, su.ec[0]));
                    const double area = (e0 + e1) + e2;
                    const double l1 = e1 / area, l2 = e2 / area;
                    const double ux0 = (double)su.ux[0], uy0 = (double)su.uy[0];
                    const double bx = (ux0 + l1 * ((double)su.ux[1] - ux0)) + l2 * ((double)su.ux[2] - ux0);
                    const double by = (uy0 + l1 * ((double)su.uy[1] - uy0)) + l2 * ((double)su.uy[2] - uy0);
                    // (a NaN fails every comparison; floor(b) in 0 .. W - 1 is 0 <= b < W)
                    bp[j] = (bx >= 0.0 && bx < (double)a.W && by >= 0.0 && by < (double)a.H) ? (int)floor(by) * a.W + (int)floor(bx) : -1;
                }
            }
        __syncthreads();
    }
    const size_t n = (size_t)a.W * a.H;
    const unsigned long long D = 65535ull * 255ull;
#pragma unroll
    for (int j = 0; j < NPX; j++) {
        const int r = rb + 4 * j;
        if (c >= a.W || r >= a.H) continue;
        const int p = r * a.W + c;
        unsigned long long ch[3];
        ch[0] = ch[1] = ch[2] = a.frame[p];
        if (bp[j] >= 0) {
            for (int k = 0; k < a.n_layers; k++) {
                const int s = a.labels[k * n + bp[j]];
                if (s < 0) continue;
                const unsigned long long al = (unsigned long long)(a.weights ? a.weights[k * n + bp[j]] : 65535u) *
                                              (unsigned long long)(a.levels ? a.levels[s] : 255u);
#pragma unroll
                for (int q = 0; q < 3; q++) ch[q] = (ch[q] * (D - al) + (unsigned long long)a.colours[3 * s + q] * al + D / 2) / D;
            }
            if ((a.flags & CV_OUTLINE) && a.outline[bp[j]]) {
                const int s = a.labels[bp[j]];
#pragma unroll
                for (int q = 0; q < 3; q++) ch[q] = a.colours[3 * s + q];
            }
        }
        unsigned b = (unsigned)ch[0];
        if (a.flags & CV_WIRE) {
            const unsigned wire = a.wire[p];
            b = d_sat(b + (wire > 2u ? 256u : 128u * wire));
        }
        sh.px[r - r0][c - c0] = b | ((unsigned)ch[1] << 8) | ((unsigned)ch[2] << 16);
    }
    __syncthreads();
    d_cv_store(sh.px, a.W, a.H, c0, r0, a.out);
}

// The outline plane of layer 0, once per hm_view_set_cells: a body pixel with label s >= 0 is an outline pixel when one
// of its four neighbours has another label; a neighbour off the frame counts as another.
__global__ __launch_bounds__(256) void k_view_cell_outline(const int *__restrict__ lab, int W, int H, uint8_t *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const int r = p / W, c = p - r * W, s = lab[p];
    out[p] = s >= 0 && (c == 0 || lab[p - 1] != s || c == W - 1 || lab[p + 1] != s || r == 0 || lab[p - W] != s || r == H - 1 ||
                        lab[p + W] != s);
}

// The markers (reference synth.py:268-279, cv2.circle filled): point i at ((int)x, (int)y), truncated as C does, the pixels
// with dx^2 + dy^2 <= radius^2 in integers in its colour, pixels off the frame left out; a point that is not finite or
// beyond +-2^20 px is skipped.  A later point wins over an earlier one: one wave per point, all in one launch, and a pixel
// that a later point covers as well is left to that point -- every pixel has one writer, whatever order the waves run in.
__global__ __launch_bounds__(256) void k_view_cell_marks(int W, int H, int P, int radius, const double *__restrict__ pts,
                                                         const uint8_t *__restrict__ col, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * (256 / VIEW_SEG_WAVE) + threadIdx.x / VIEW_SEG_WAVE;
    const int lane = threadIdx.x % VIEW_SEG_WAVE;
    if (i >= P) return;
    const double x = pts[2 * i], y = pts[2 * i + 1];
    if (!(d_coord_ok(x) && d_coord_ok(y))) return;
    const long long cx = (long long)x, cy = (long long)y, R = radius, R2 = R * R;
    const long long xa = max(cx - R, 0ll), xb = min(cx + R, (long long)W - 1), ya = max(cy - R, 0ll), yb = min(cy + R, (long long)H - 1);
    if (xa > xb || ya > yb) return;
    const long long bw = xb - xa + 1, n = bw * (yb - ya + 1);
    for (long long k = lane; k < n; k += VIEW_SEG_WAVE) {
        const long long py = ya + k / bw, px = xa + k % bw;
        if ((px - cx) * (px - cx) + (py - cy) * (py - cy) > R2) continue;
        bool later = false;
        for (int j = i + 1; j < P && !later; j++) {
            const double xj = pts[2 * j], yj = pts[2 * j + 1];
            if (!(d_coord_ok(xj) && d_coord_ok(yj))) continue;
            const long long dx = px - (long long)xj, dy = py - (long long)yj;
            later = dx * dx + dy * dy <= R2;
        }
        if (later) continue;
        const size_t o = 3 * ((size_t)py * W + (size_t)px);
        out[o] = col[3 * i]; out[o + 1] = col[3 * i + 1]; out[o + 2] = col[3 * i + 2];
    }
}

// ---- the flow tool's preview: frame blended with the flow in the Middlebury colour code ------------------------------
// The 55-entry wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow", the colour code of its
// evaluation page): RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 steps, R G B, integer divisions.
#define VIEW_NCOLS 55
#define VIEW_FLOW_SAT 15.0f            // px of flow at full saturation
__device__ __forceinline__ void d_wheel_entry(int k, int c[3])
{
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    int s = 0;
    while (k >= seg[s]) { k -= seg[s]; s++; }
    const int up = 255 * k / seg[s], down = 255 - 255 * k / seg[s];
    switch (s) {
    case 0: c[0] = 255; c[1] = up; c[2] = 0; break;
    case 1: c[0] = down; c[1] = 255; c[2] = 0; break;
    case 2: c[0] = 0; c[1] = 255; c[2] = up; break;
    case 3: c[0] = 0; c[1] = down; c[2] = 255; break;
    case 4: c[0] = up; c[1] = 0; c[2] = 255; break;
    default: c[0] = 255; c[1] = 0; c[2] = down; break;
    }
}

// the wheel colour of a flow vector, B G R; 0 for a non-finite or absurd vector
__device__ __forceinline__ void d_wheel(float fx, float fy, unsigned bgr[3])
{
    bgr[0] = bgr[1] = bgr[2] = 0;
    if (fx != fx || fy != fy || !(fabsf(fx) < 1e9f) || !(fabsf(fy) < 1e9f)) return;
    const float ux = fx / VIEW_FLOW_SAT, uy = fy / VIEW_FLOW_SAT;
    const float rad = sqrtf(ux * ux + uy * uy);
    const float a = atan2f(-uy, -ux) / 3.14159265358979323846f;
    const float fk = (a + 1.0f) / 2.0f * (float)(VIEW_NCOLS - 1);
    const int k0 = (int)fk, k1 = (k0 + 1) % VIEW_NCOLS;
    const float f = fk - (float)k0;
    int c0[3], c1[3];
    d_wheel_entry(k0, c0);
    d_wheel_entry(k1, c1);
    for (int b = 0; b < 3; b++) {
        float col = (1.0f - f) * ((float)c0[b] / 255.0f) + f * ((float)c1[b] / 255.0f);
        if (rad <= 1.0f) col = rad * col;
        else col = col * 0.75f;
        bgr[2 - b] = (unsigned)(uint8_t)(int)(255.0 * (double)col);
    }
}

// out = round((2 frame + 3 wheel) / 5) per channel (the reference's addWeighted 0.4 / 0.6); frames gray (ch 1) or B G R
__global__ __launch_bounds__(256) void k_flow_preview(const uint8_t *__restrict__ frames, int ch, const float *__restrict__ fx,
                                                      const float *__restrict__ fy, long long n, uint8_t *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    unsigned w[3];
    d_wheel(fx[p], fy[p], w);
    for (int c = 0; c < 3; c++) {
        const unsigned f = frames[ch == 1 ? p : 3 * p + c];
        out[3 * p + c] = (uint8_t)((2 * (2 * f + 3 * w[c]) + 5) / 10);
    }
}
