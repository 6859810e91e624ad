// Kernels of the Rauch-Tung-Striebel smoother (hm_smooth_*, smooth.hip): dense f64 products at n x n on the matrix cores
// and the matrix-vector products of the mean recursion.  gfx950 only.
//
// The products work on 32 x 32 output tiles, one workgroup of four waves per tile, each wave one 16 x 16 quarter
// (v_mfma_f64_16x16x4_f64 through the LDS helpers of hm_types.h: element e of a lane sits at row
// 16 (wv >> 1) + (lane >> 4) + 4 e, column 16 (wv & 1) + (lane & 15)).  The k loop takes 32-wide slabs of both
// operands into LDS; entries past n are zeros, so n need not be a multiple of 16 or 32 and nothing is read or written
// outside the n x n arrays.
#pragma once
#include "hm_types.h"

#define SM_NT 256       // threads of a product workgroup

// which product (hm_op_smooth_gemm `which`):
//   SM_TN   out = A^T B
//   SM_LN   out = tril(A) B         Y = T (F P)             (T = L^-1 of Pp = L L^T; F P from k_fw_rows)
//   SM_TL   out = A^T tril(B)       G = Y^T T               (= (F P)^T T^T T = P F^T inv(Pp); P symmetric)
//                                   tril: the entries right of the diagonal are not read (the factorisation leaves them
//                                   unset) and the slabs that lie wholly right of it are skipped.  G is formed through
//                                   the factor, never through inv(Pp) = T^T T: the rounding of T^T T is of the size of
//                                   |T^T| |T|, which T (F P) -- the whitened F P -- is far below when Pp is badly scaled
//                                   or F P nearly cancels against it, and Ps = P + E G^T is a difference of that size.
//   SM_NND  out = A (B - C)         E = G (Ps' - Pp)
//   SM_SYM  out = C + A B^T         Ps = P + E G^T: lower tiles only, each mirrored, so the result is exactly
//                                   symmetric; out may be C (every element is read by the thread that writes it and
//                                   by nobody else: the upper triangle is written, never read)
enum { SM_TN = 0, SM_NND = 1, SM_SYM = 2, SM_LN = 3, SM_TL = 4 };

template <int MODE>
__global__ __launch_bounds__(SM_NT) void k_sm_gemm(const double *__restrict__ A, const double *__restrict__ B,
                                                  const double *C, double *out, int n)
{
    const int I = blockIdx.y, J = blockIdx.x;
    if (MODE == SM_SYM && J > I) return;
    __shared__ double X[DNB][DNB + 1];
    __shared__ double Y[DNB][DNB + 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int i0 = I * DNB, j0 = J * DNB;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    // (the triangular operand: column k <= row i0 + i of A, row k >= column j0 + j of B)
    const int k_begin = MODE == SM_TL ? j0 : 0, k_end = MODE == SM_LN ? min(n, i0 + DNB) : n;
    for (int k0 = k_begin; k0 < k_end; k0 += DNB) {
#pragma unroll
        for (int q = 0; q < DNB * DNB / SM_NT; q++) {
            const int e = t + SM_NT * q, r = e / DNB, c = e % DNB;
            double x = 0.0, y = 0.0;
            if (MODE == SM_TN || MODE == SM_TL) {   // X[k][i] = A[k0 + k][i0 + i], Y[k][j] = B[k0 + k][j0 + j]
                if (k0 + r < n && i0 + c < n) x = A[(size_t)(k0 + r) * n + i0 + c];
                if (k0 + r < n && j0 + c < n && (MODE == SM_TN || j0 + c <= k0 + r)) y = B[(size_t)(k0 + r) * n + j0 + c];
            } else if (MODE == SM_LN) {     // X[i][k] = A[i0 + i][k0 + k] (k <= i), Y[k][j] = B[k0 + k][j0 + j]
                if (i0 + r < n && k0 + c <= i0 + r) x = A[(size_t)(i0 + r) * n + k0 + c];
                if (k0 + r < n && j0 + c < n) y = B[(size_t)(k0 + r) * n + j0 + c];
            } else if (MODE == SM_NND) {    // X[i][k] = A[i0 + i][k0 + k], Y[k][j] = B - C at [k0 + k][j0 + j]
                if (i0 + r < n && k0 + c < n) x = A[(size_t)(i0 + r) * n + k0 + c];
                if (k0 + r < n && j0 + c < n) {
                    const size_t o = (size_t)(k0 + r) * n + j0 + c;
                    y = B[o] - C[o];
                }
            } else {                        // X[i][k] = A[i0 + i][k0 + k], Y[j][k] = B[j0 + j][k0 + k]
                if (i0 + r < n && k0 + c < n) x = A[(size_t)(i0 + r) * n + k0 + c];
                if (j0 + r < n && k0 + c < n) y = B[(size_t)(j0 + r) * n + k0 + c];
            }
            X[r][c] = x;
            Y[r][c] = y;
        }
        __syncthreads();
        if (MODE == SM_TN || MODE == SM_TL) {
            acc = d_mfma_tn(X, Y, wv, lane, acc);
        } else if (MODE == SM_NND || MODE == SM_LN) {
            acc = d_mfma_nn(X, Y, wv, lane, acc);
        } else {
            const int i = 16 * (wv >> 1) + (lane & 15), j = 16 * (wv & 1) + (lane & 15), kq = lane >> 4;
#pragma unroll
            for (int kk = 0; kk < DNB / 4; kk++)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[i][4 * kk + kq], Y[j][4 * kk + kq], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int jj = j0 + 16 * (wv & 1) + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int ii = i0 + 16 * (wv >> 1) + (lane >> 4) + 4 * e;
        if (ii >= n || jj >= n) continue;
        if (MODE == SM_SYM) {
            if (jj > ii) continue;          // (the diagonal tile: its upper half is the mirror of its lower)
            const double v = C[(size_t)ii * n + jj] + acc[e];
            out[(size_t)ii * n + jj] = v;
            out[(size_t)jj * n + ii] = v;
        } else {
            out[(size_t)ii * n + jj] = acc[e];
        }
    }
}

// y = T x for the lower triangle of T (n x n; the entries right of the diagonal are not read: the factorisation leaves
// them unset), one workgroup per row, the partial sums added in a fixed tree
__global__ __launch_bounds__(256) void k_sm_trmv(const double *__restrict__ T, const double *__restrict__ x,
                                                 double *__restrict__ y, int n)
{
    __shared__ double s[256];
    const int i = blockIdx.x, t = threadIdx.x;
    double v = 0.0;
    for (int j = t; j <= i; j += 256) v += T[(size_t)i * n + j] * x[j];
    s[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    if (t == 0) y[i] = s[0];
}

// y = base + A^T x (base may be NULL: y = A^T x); lower = 1: A is lower triangular (rows i >= j only), one thread per
// column, the rows in order
__global__ __launch_bounds__(256) void k_sm_mvt(const double *__restrict__ A, const double *__restrict__ x,
                                                const double *__restrict__ base, double *__restrict__ y, int n, int lower)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double v = 0.0;
    for (int i = lower ? j : 0; i < n; i++) v += A[(size_t)i * n + j] * x[i];
    y[j] = base ? base[j] + v : v;
}

// d = a - b (n)
__global__ void k_sm_sub(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ d, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = a[i] - b[i];
}

// d = diag(P) (n)
__global__ void k_sm_diag(const double *__restrict__ P, double *__restrict__ d, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = P[(size_t)i * n + i];
}

// the factorisation of Pp failed (a pivot that was not positive, or a non-finite input): some diagonal entry of
// T = L^-1 is not a positive finite number -> *flag = 1 + the frame it belongs to (the first such frame is kept)
__global__ void k_sm_check(const double *__restrict__ T, int n, int frame, int *flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = T[(size_t)i * n + i];
    if (!(d > 0.0) || !isfinite(d)) atomicCAS(flag, 0, frame + 1);
}
