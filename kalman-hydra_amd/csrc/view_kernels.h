// The tracker's views (reference renderer.py:344-373, 436-475, 595-628; kalman.py:638-674) and the flow preview of the
// flow tool (reference src/optical_flow_ext.cpp:172-281, 336-389) as kernels.  Every view is H x W x 3 uint8, B, G, R,
// rows top to bottom.  Everything below is exact integer or f64 arithmetic (the library builds with -ffp-contract=off),
// except atan2f in the colour wheel, so a NumPy restatement reproduces it bit for bit (tests/view_ref.py).
#pragma once
#include "hm_common.h"

#define VIEW_SEG_WAVE 64               // lanes per segment: a segment's pixels are spread over one wave
#define VIEW_COORD_MAX 1048576.0       // segments with an end point beyond +-2^20 px are not drawn (a diverged state)

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

__device__ __forceinline__ bool d_coord_ok(double a) { return a >= -VIEW_COORD_MAX && a <= VIEW_COORD_MAX; }

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

// min / max of a float plane as order-preserving unsigned keys (mm[0] = min key, mm[1] = max key; NaNs are skipped)
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
        if (v != v) continue;
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
        if (fmax != fmin && f == f) v = (unsigned)floor(255.0 * ((double)f - (double)fmin) / ((double)fmax - (double)fmin));
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
