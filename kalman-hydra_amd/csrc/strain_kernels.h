// The deformation of the tracked mesh (hm_strain_*, hm_view_strain*): per triangle and frame the deformation gradient of
// the map body -> frame, its area ratio, principal stretches, their axis and the rotation; the same averaged over the body
// pixels of caller labels; and a view that paints one of them onto the animal.  include/hydra_mi.h has the rules in full,
// tests/strain_ref.py restates the three kernels in NumPy, bit for bit: everything below is binary64, one correctly rounded
// operation at a time in the order written (the library builds with -ffp-contract=off), + - * / sqrt fabs rint only.
#pragma once
#include "hm_types.h"
#include "view_kernels.h"

#define STRAIN_VALS 7                  // J, l1, l2, c2, s2, rc, rs

// One triangle in one frame.  v: its vertex ids in the body map's order (i0, i1, i2 after the orientation swap at X = uv),
// uv: the binary32 texture coordinates, X: the 2N positions of the frame (x of vertex i at X[2 i], y at X[2 i + 1]).
//   p = U1 - U0, q = U2 - U0, a = x1 - x0, b = x2 - x0;  d0 = p.x q.y - p.y q.x
//   F = [a b] [p q]^-1, J = det [a b] / d0, C = F^T F, m +- r its eigenvalues: l1 = sqrt(m + r), l2 = |J| / l1;
//   (c2, s2) the double angle of the l1 axis in the body frame, (rc, rs) the rotation of the polar factor.
// d0 == 0 or a position that is not finite: seven NaNs.
__device__ __forceinline__ void d_strain(int4 v, const float *__restrict__ uv, const double *__restrict__ X, double (&o)[STRAIN_VALS])
{
    const double u0x = (double)uv[2 * v.x], u0y = (double)uv[2 * v.x + 1];
    const double px = (double)uv[2 * v.y] - u0x, py = (double)uv[2 * v.y + 1] - u0y;
    const double qx = (double)uv[2 * v.z] - u0x, qy = (double)uv[2 * v.z + 1] - u0y;
    const double x0 = X[2 * v.x], y0 = X[2 * v.x + 1], x1 = X[2 * v.y], y1 = X[2 * v.y + 1], x2 = X[2 * v.z], y2 = X[2 * v.z + 1];
    const double d0 = px * qy - py * qx;
    const double big = 1.7976931348623157e308;
    const bool finite = fabs(x0) <= big && fabs(y0) <= big && fabs(x1) <= big && fabs(y1) <= big && fabs(x2) <= big &&
                        fabs(y2) <= big;                   // (a NaN fails its comparison)
    if (d0 == 0.0 || !finite) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
        for (int j = 0; j < STRAIN_VALS; j++) o[j] = nan;
        return;
    }
    const double ax = x1 - x0, ay = y1 - y0, bx = x2 - x0, by = y2 - y0;
    const double F11 = (ax * qy - bx * py) / d0, F12 = (bx * px - ax * qx) / d0;
    const double F21 = (ay * qy - by * py) / d0, F22 = (by * px - ay * qx) / d0;
    const double J = (ax * by - ay * bx) / d0;
    const double c11 = F11 * F11 + F21 * F21, c12 = F11 * F12 + F21 * F22, c22 = F12 * F12 + F22 * F22;
    const double m = (c11 + c22) / 2.0, d = (c11 - c22) / 2.0;
    const double r = sqrt(d * d + c12 * c12);
    const double l1 = sqrt(m + r);
    const double tr = F11 + F22, sk = F21 - F12;
    const double s = sqrt(tr * tr + sk * sk);
    o[0] = J;
    o[1] = l1;
    o[2] = l1 == 0.0 ? 0.0 : fabs(J) / l1;
    o[3] = r == 0.0 ? 1.0 : d / r;
    o[4] = r == 0.0 ? 0.0 : c12 / r;
    o[5] = s == 0.0 ? 1.0 : tr / s;
    o[6] = s == 0.0 ? 0.0 : sk / s;
}

// All frames of a call in one launch: one thread per (frame, triangle), g = frame * T + triangle, so a wave reads the ids
// and uv of 64 consecutive triangles, gathers their positions out of one or two frames' rows of X, and writes 64 * 56
// contiguous bytes.  Its traffic: every frame's positions are read once from HBM (the vertices shared between triangles
// come out of the cache), the seven doubles are written once.  X: rows of `stride` doubles, the 2N positions first.
__global__ __launch_bounds__(256) void k_strain_tri(long long total, int T, size_t stride, const int4 *__restrict__ tidx,
                                                    const float *__restrict__ uv, const double *__restrict__ X,
                                                    double *__restrict__ out)
{
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const long long k = g / T;
        const int t = (int)(g - k * T);
        double o[STRAIN_VALS];
        d_strain(tidx[t], uv, X + (size_t)k * stride, o);
        double *dst = out + (size_t)g * STRAIN_VALS;
#pragma unroll
        for (int j = 0; j < STRAIN_VALS; j++) dst[j] = o[j];
    }
}

// trace[k, s, j] = (sum over t of cnt[s, t] v[k, t, j]) / n_s, j = J, l1, l2: the mean over the body-map pixels of label s
// of the piecewise constant field.  cnt as compressed rows: the triangles with a pixel of label s in ascending order
// (off[s] .. off[s + 1]), their pixel counts, n_s their sum.  One thread per (frame, label) walks its row in that order
// with one accumulator per value, starting from 0.0 -- no atomics, the order is the result's bits.  n_s == 0: NaN.
__global__ __launch_bounds__(256) void k_strain_label(long long total, int L, int T, const int *__restrict__ off,
                                                      const int *__restrict__ ent_t, const unsigned *__restrict__ ent_c,
                                                      const unsigned *__restrict__ n_s, const double *__restrict__ v,
                                                      double *__restrict__ out)
{
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const long long k = g / L;
        const int s = (int)(g - k * L);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const double *vk = v + (size_t)k * T * STRAIN_VALS;
        for (int e = off[s]; e < off[s + 1]; e++) {
            const double c = (double)ent_c[e];
            const double *vt = vk + (size_t)ent_t[e] * STRAIN_VALS;
            a0 = a0 + c * vt[0];
            a1 = a1 + c * vt[1];
            a2 = a2 + c * vt[2];
        }
        const unsigned n = n_s[s];
        const double nan = __longlong_as_double(0x7ff8000000000000ll), dn = (double)n;
        double *dst = out + (size_t)g * 3;
        dst[0] = n ? a0 / dn : nan;
        dst[1] = n ? a1 / dn : nan;
        dst[2] = n ? a2 / dn : nan;
    }
}

// ---- the strain view ---------------------------------------------------------------------------------------------------
// Per pixel of the image at state X: the base B = G = R = frame[r, c]; the lowest-indexed triangle over the pixel centre,
// found exactly as k_view_cells finds it (the same strips, the candidates by its d_cv_candidates, batches of CV_CAP setups
// in LDS walked in ascending order, the same skips -- here the batch keeps the triangle's level instead of its texture
// coordinates); the triangle's level
//   level = clamp(128 + rint(gain (value - 1)), 0, 255), value = J, l1 or l2 (which = 0, 1, 2) of d_strain,
// computed by the thread that sets the triangle up; a level that is NaN keeps the base; else every channel becomes
//   (ch (255 - alpha) + lut[level][ch] alpha + 127) / 255 in integers;
// then (flags bit 1) B = min(255, B + 128 count) of k_view_wire.  The strip is written by k_view_cells' d_cv_store.
struct StrainViewArgs {
    int W, H, T, which, alpha, flags, tiles_x;
    double gain;
    const int *tri;
    const int4 *tidx;                  // vertex ids in the body map's order
    const float *uv;
    const double *X;                   // 2N positions
    const uint8_t *frame;              // W x H gray
    const uint8_t *lut;                // 256 x 3, B G R
    const unsigned *wire;              // wireframe counts (CV_WIRE)
    uint8_t *out;                      // W*H*3, 4-byte aligned
};

struct StrainShared {
    unsigned mask[EKF_MAX_TRI / 32];
    TriSetup cand[CV_CAP];
    int level[CV_CAP];                 // 0..255, -1: NaN
    unsigned px[CV_H][CV_W];           // B | G << 8 | R << 16
};

// -1: keep the base
__device__ __forceinline__ int d_strain_level(double value, double gain)
{
    const double l = 128.0 + rint(gain * (value - 1.0));
    if (l != l) return -1;
    return l < 0.0 ? 0 : l > 255.0 ? 255 : (int)l;
}

__global__ __launch_bounds__(256) void k_view_strain(StrainViewArgs a)
{
    __shared__ StrainShared sh;
    const int tid = threadIdx.x;
    const int words = (a.T + 31) / 32;
    const int c0 = ((int)blockIdx.x % a.tiles_x) * CV_W, r0 = ((int)blockIdx.x / a.tiles_x) * CV_H;
    const double *__restrict__ X = a.X;
    d_cv_candidates(sh.mask, a.T, a.tri, X, a.W, a.H, c0, r0);
    int total = 0;
    for (int w = 0; w < words; w++) total += __popc(sh.mask[w]);
    const int c = c0 + (tid & 63), rb = r0 + (tid >> 6);
    constexpr int NPX = CV_W * CV_H / 256;
    int lev[NPX];                      // the level, -1: keep the base; -2: no triangle found yet
#pragma unroll
    for (int j = 0; j < NPX; j++) lev[j] = -2;
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
#pragma unroll
            for (int k = 0; k < 3; k++) { su.ux[k] = 0.0f; su.uy[k] = 0.0f; su.ax[k] = 0.0f; su.ay[k] = 0.0f; }
            sh.cand[rank - base] = su;
            double o[STRAIN_VALS];
            d_strain(a.tidx[tb], a.uv, X, o);
            sh.level[rank - base] = d_strain_level(a.which == 0 ? o[0] : a.which == 1 ? o[1] : o[2], a.gain);
        }
        __syncthreads();
        if (c < a.W)
            for (int q = 0; q < nch; q++) {                // ascending triangle order
                const TriSetup &su = sh.cand[q];
#pragma unroll
                for (int j = 0; j < NPX; j++) {
                    const int r = rb + 4 * j;
                    if (lev[j] != -2 || r >= a.H || c < su.cmin || c > su.cmax || r < su.rmin || r > su.rmax) continue;
                    double e1, e2;
                    if (!d_tri_cover2(su, (double)c, (double)r, e1, e2)) continue;
                    lev[j] = sh.level[q];
                }
            }
        __syncthreads();
    }
    const unsigned al = (unsigned)a.alpha;
#pragma unroll
    for (int j = 0; j < NPX; j++) {
        const int r = rb + 4 * j;
        if (c >= a.W || r >= a.H) continue;
        const int p = r * a.W + c;
        unsigned ch[3];
        ch[0] = ch[1] = ch[2] = a.frame[p];
        if (lev[j] >= 0) {
#pragma unroll
            for (int q = 0; q < 3; q++) ch[q] = (ch[q] * (255u - al) + (unsigned)a.lut[3 * lev[j] + q] * al + 127u) / 255u;
        }
        if (a.flags & CV_WIRE) {
            const unsigned wire = a.wire[p];
            ch[0] = d_sat(ch[0] + (wire > 2u ? 256u : 128u * wire));
        }
        sh.px[r - r0][c - c0] = ch[0] | (ch[1] << 8) | (ch[2] << 16);
    }
    __syncthreads();
    d_cv_store(sh.px, a.W, a.H, c0, r0, a.out);
}
