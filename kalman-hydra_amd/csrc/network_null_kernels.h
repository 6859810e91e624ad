// A trace and its surrogates against every pixel of the kept registered video, reduced on the device to what a
// significance test needs (hm_body_rec_trace_null; hydra_mi/network.py map_null; DESIGN.md section 18;
// tests/network_null_ref.py restates all of it in Python integers).
//
// Column 0 of q[k, s] is the observed trace, columns 1 .. L - 1 its surrogates (the device does not know how they were
// made).  With c_s(p), w1(p), w2(p) as in network_kernels.h, u1_s = sum_k q[k, s] and vb[s] the host's F u2_s - u1_s^2:
//   num_s(p) = F c_s(p) - w1(p) u1_s            int64
//   a(p)     = F w2(p) - w1(p)^2                int64
//   rho_s(p) = (double)num_s(p) / sqrt((double)a(p) * vb[s]),  0.0 where a(p) = 0 or vb[s] = 0
//   tmax[s], tmin[s] = the largest and smallest rho_s(p) over the map pixels
//   ge[p], le[p]     = the number of s >= 1 with num_s(p) >= num_0(p), with num_s(p) <= num_0(p)
// The only floating point is rho: one conversion each, one product, one square root, one division, one operation at a
// time (the library builds with -ffp-contract=off; binary64 sqrt and / are correctly rounded).
#pragma once
#include "network_kernels.h"     // (REC_MAP_GROUP, REC_MAP_QMAX; d_rec_frame: roi_kernels.h; REC_NULL_MAX: hm_types.h)

#define REC_NULL_LMAX 4096             // the most columns of a call
#define REC_NULL_UNROLL 8              // frames whose record dwords a lane loads before it works on them (even)

struct RecNull {
    RecBox b;
    const uint8_t *const *chunks;
    int F, L, run, W;                  // frames, columns, frames per run (<= REC_NULL_MAX), the frame's width
    const int *q;                      // F x L, frame-major
    const long long *u1;               // L: the columns' sums
    const double *vb;                  // L: F u2 - u1^2 as the host rounded it, >= 0 and finite
    const int *tri;                    // the body map, W x H (< 0: off the map)
    const unsigned long long *c0, *w1, *w2;    // column 0's products and the pixels' sums, planes of pitch * bh (k_rec_trace_maps)
    unsigned long long *kmax, *kmin;   // L keys each (d_null_key), set to the lowest / highest key by the caller; NULL (both): no rho
    unsigned *ge, *le;                 // a plane of pitch * bh each, zeroed by the caller; NULL: not counted
};

// a dword of the record, which is global memory (a chunk's address comes out of a table: the compiler cannot know)
typedef __attribute__((address_space(1))) unsigned rec_gdword;

// two whole numbers of 16 bits in a dword, what v_dot2_i32_i16 multiplies; byte `sel & 7` of `even` and byte `(sel >> 16) & 3`
// of `odd`, each zero-extended (v_perm_b32: selector bytes 0..3 are the second operand's, 4..7 the first's, 0x0c is 0)
typedef short rec_pair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ rec_pair d_null_pair(unsigned even, unsigned odd, unsigned sel)
{
    return __builtin_bit_cast(rec_pair, __builtin_amdgcn_perm(odd, even, sel));
}

// binary64 without NaN -> a 64-bit key in the same order (the host undoes it: record.hip)
__device__ __forceinline__ unsigned long long d_null_key(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : u | (1ull << 63);
}

// The work split of k_rec_trace_maps: a thread owns one dword of the box frame, four pixels, and a workgroup 256 of them
// and a group of REC_MAP_GROUP columns (the last may be partial; blockIdx.x = tile * groups + group).  A workgroup walks
// all F frames in runs of g.run: the run's q of the group and its frames' addresses sit in LDS, the 4 x 8 products of a
// frame are added to 32-bit accumulators, two frames at a time (v_dot2_i32_i16; they hold a run: 255 x 32767 x 256 <
// 2^31), and between runs these are widened into 64-bit registers -- no partial sum leaves the thread, so nothing here
// adds to memory per run.  At the end a thread has c_s(p) of its pixels and columns
// whole; it reads c_0, w1, w2 of its pixels once and forms, per map pixel, the two counts (one 32-bit atomic add per pixel
// and plane where the count is not 0: the groups meet there) and rho per column, whose largest and smallest go across the
// wave by shuffles, across the workgroup through LDS, and into one 64-bit atomic max and min per workgroup and column on
// an order-preserving key.  Sums of whole numbers and max / min of doubles without NaN do not depend on the order (num = 0
// gives +0.0: -0.0 never occurs), so the result is the same bytes for every run length.  Dwords past pitch * bh / 4 are
// neither read nor counted, box pixels off the map (the row's padding included) enter neither counts nor max / min.  No
// thread leaves before a barrier.
__global__ __launch_bounds__(256) void k_rec_trace_null(RecNull g)
{
    __shared__ unsigned qs[REC_NULL_MAX / 2 * REC_MAP_GROUP];
    __shared__ const uint8_t *fp[REC_NULL_MAX];                    // the run's frames in the record
    __shared__ double red[2][4][REC_MAP_GROUP];
    // (the column group is the fast index of the grid: the workgroups that read the same dwords of the record are
    // dispatched together, and all but the first of them on a die find those dwords in its L2)
    const int groups = (g.L + REC_MAP_GROUP - 1) / REC_MAP_GROUP, tile = blockIdx.x / groups;
    const int dw = tile * 256 + threadIdx.x;
    const size_t nb = (size_t)g.b.pitch * g.b.bh;
    const bool in = (size_t)dw < nb >> 2;                          // (the last workgroup may end beyond the frame)
    const int g0 = (blockIdx.x - tile * groups) * REC_MAP_GROUP, ng = min(REC_MAP_GROUP, g.L - g0);
    const size_t off = in ? 4 * (size_t)dw : 0;                    // (a lane past the box frame reads dword 0; its sums are never looked at)
    long long wide[REC_MAP_GROUP][4];
#pragma unroll
    for (int t = 0; t < REC_MAP_GROUP; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) wide[t][i] = 0;
    for (int k0 = 0; k0 < g.F; k0 += g.run) {                      // (the same trips for the whole workgroup)
        const int m = min(g.run, g.F - k0);
        const int mu = (m + REC_NULL_UNROLL - 1) / REC_NULL_UNROLL * REC_NULL_UNROLL;     // (<= REC_NULL_MAX, a multiple itself)
        __syncthreads();                                           // the previous run's q has been read
        // The run in LDS, filled up to whole blocks of REC_NULL_UNROLL frames: a frame past the run has q = 0 and adds
        // nothing, and its address is the record's last frame again, so the loop below has no condition in it.  The q of
        // two consecutive frames share a dword (|q| <= 32767 is 16 bits): the lower half is the even frame's.
        for (int e = threadIdx.x; e < (mu >> 1) * REC_MAP_GROUP; e += 256) {
            const int j = 2 * (e / REC_MAP_GROUP), t = e % REC_MAP_GROUP;
            const int lo = j < m && t < ng ? g.q[(size_t)(k0 + j) * g.L + g0 + t] : 0;
            const int hi = j + 1 < m && t < ng ? g.q[(size_t)(k0 + j + 1) * g.L + g0 + t] : 0;
            qs[e] = ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16);
        }
        for (int j = threadIdx.x; j < mu; j += 256) fp[j] = d_rec_frame(g.b, g.chunks, min(k0 + j, g.F - 1));
        __syncthreads();
        int acc[REC_MAP_GROUP][4];
#pragma unroll
        for (int t = 0; t < REC_MAP_GROUP; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) acc[t][i] = 0;
        for (int j0 = 0; j0 < mu; j0 += REC_NULL_UNROLL) {
            unsigned vs[REC_NULL_UNROLL];                          // (the loads of REC_NULL_UNROLL frames are in flight together)
#pragma unroll
            for (int u = 0; u < REC_NULL_UNROLL; u++) vs[u] = *(const rec_gdword *)(fp[j0 + u] + off);
#pragma unroll
            for (int u = 0; u < REC_NULL_UNROLL; u += 2) {
                // pixel i of the two frames as two 16-bit halves (bytes i of vs[u] and of vs[u + 1], zero-extended), then
                // per column one v_dot2: acc += v_even q_even + v_odd q_odd, exact in 32 bits like the single products
                const rec_pair v[4] = {d_null_pair(vs[u], vs[u + 1], 0x0c040c00u), d_null_pair(vs[u], vs[u + 1], 0x0c050c01u),
                                       d_null_pair(vs[u], vs[u + 1], 0x0c060c02u), d_null_pair(vs[u], vs[u + 1], 0x0c070c03u)};
                const unsigned *qj = qs + ((j0 + u) >> 1) * REC_MAP_GROUP;
#pragma unroll
                for (int t = 0; t < REC_MAP_GROUP; t++) {
                    const rec_pair qt = __builtin_bit_cast(rec_pair, qj[t]);
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[t][i] = __builtin_amdgcn_sdot2(v[i], qt, acc[t][i], false);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < REC_MAP_GROUP; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) wide[t][i] += (long long)acc[t][i];
    }
    // the thread's four pixels: on the map?  their sums and column 0's numerator
    const size_t p = 4 * (size_t)dw;
    const int y = in ? (int)(p / (size_t)g.b.pitch) : 0, x0 = in ? (int)(p - (size_t)y * g.b.pitch) : 0;
    const long long F = g.F, u10 = g.u1[0];
    bool on[4];
    long long w1[4], a[4], num0[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        on[i] = in && x0 + i < g.b.bw && g.tri[(size_t)(g.b.r0 + y) * g.W + g.b.c0 + x0 + i] >= 0;
        w1[i] = on[i] ? (long long)g.w1[p + i] : 0;
        a[i] = on[i] ? F * (long long)g.w2[p + i] - w1[i] * w1[i] : 0;
        num0[i] = on[i] ? F * (long long)g.c0[p + i] - w1[i] * u10 : 0;
    }
    const bool rho = g.kmax != nullptr, count = g.ge != nullptr || g.le != nullptr;      // (the same for the whole grid)
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    unsigned nge[4] = {0u, 0u, 0u, 0u}, nle[4] = {0u, 0u, 0u, 0u};
    double mx[REC_MAP_GROUP], mn[REC_MAP_GROUP];
#pragma unroll
    for (int t = 0; t < REC_MAP_GROUP; t++) {
        mx[t] = -inf;
        mn[t] = inf;
        if (t >= ng) continue;                                     // (the whole workgroup)
        const long long u1 = g.u1[g0 + t];
        const double vb = g.vb[g0 + t];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!on[i]) continue;
            const long long num = F * wide[t][i] - w1[i] * u1;
            if (count && g0 + t >= 1) {
                nge[i] += num >= num0[i];
                nle[i] += num <= num0[i];
            }
            if (rho) {
                double r = 0.0;
                if (a[i] != 0 && vb != 0.0) {
                    const double prod = (double)a[i] * vb;
                    r = (double)num / sqrt(prod);
                }
                mx[t] = r > mx[t] ? r : mx[t];
                mn[t] = r < mn[t] ? r : mn[t];
            }
        }
    }
    if (count) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (g.ge && nge[i] != 0u) atomicAdd(g.ge + p + i, nge[i]);         // (a count that is not 0: the pixel is on the map)
            if (g.le && nle[i] != 0u) atomicAdd(g.le + p + i, nle[i]);
        }
    }
    if (rho) {                                                     // (the whole grid)
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int t = 0; t < REC_MAP_GROUP; t++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double hi = __shfl_xor(mx[t], o), lo = __shfl_xor(mn[t], o);
                mx[t] = hi > mx[t] ? hi : mx[t];
                mn[t] = lo < mn[t] ? lo : mn[t];
            }
            if (lane == 0) {
                red[0][wave][t] = mx[t];
                red[1][wave][t] = mn[t];
            }
        }
        __syncthreads();
        if (threadIdx.x < ng) {
            const int t = threadIdx.x;
            double hi = red[0][0][t], lo = red[1][0][t];
            for (int w = 1; w < 4; w++) {
                hi = red[0][w][t] > hi ? red[0][w][t] : hi;
                lo = red[1][w][t] < lo ? red[1][w][t] : lo;
            }
            if (hi != -inf) {                                      // (a workgroup without a map pixel has nothing to say)
                atomicMax(g.kmax + g0 + t, d_null_key(hi));
                atomicMin(g.kmin + g0 + t, d_null_key(lo));
            }
        }
    }
}
