// The running baseline per pixel of the kept registered video (hm_body_rec_planes, hm_body_rec_stats_add;
// hydra_mi/detrend.py; tests/detrend_ref.py restates all of it in NumPy integers).
//
// For frame k of a record of F frames and box pixel p, v_k(p) the recorded value:
//   window    frames a = max(0, k - half) .. b = min(F - 1, k + half), n = b - a + 1 of them
//   baseline  B_k(p): the value at 0-based rank (q (n - 1)) / 100 (integer division) of the window's n values sorted
//             ascending -- np.percentile(method="lower"), a uint8
//   excess    E_k(p) = max(v_k(p) - B_k(p), 0)
//   dF/F byte D_k(p) = min(255, (gain E_k(p)) / max(B_k(p), floor)), unsigned integer division
// Off the map and in the padding v = 0, so B = E = D = 0 without a look at the map.
#pragma once
#include "roi_kernels.h"

#define DET_HALF_MAX 1024              // 2 * 1024 + 1 values of a window at most: a bin's count fits 16 bits
#define DET_STAGE 4                    // frames staged at a time: 4 segments of 16 dwords, one dword per lane
// dynamic LDS of a workgroup (one wave): the histograms, then four staging rows (entering, leaving, current, result)
#define DET_HIST_DWORDS (128 * 64)
#define DET_LDS_BYTES ((DET_HIST_DWORDS + 4 * 64) * 4)

struct RecRunning {
    RecBox b;
    const uint8_t *const *chunks;
    int F;                             // frames of the record: the windows reach over all of them
    int k0, n;                         // the frames written: k0 .. k0 + n - 1
    int run;                           // frames per run
    int seg0;                          // the first segment of the launch: blockIdx.x counts from it
    int what, half, q, floor, gain;    // what: 1 baseline, 2 excess, 3 dF/F byte
    uint8_t *out;                      // n frames in the record's layout, fs bytes apart
};

// One wave per 64-byte segment of the box frame (blockIdx.x) and run of frames (blockIdx.y strides over the runs): a lane
// per box pixel.  Each lane keeps the 256-bin histogram of its window in LDS -- counts of 16 bits, the two bins 2i and
// 2i + 1 of a lane in the dword i * 64 + lane, so no two lanes share a dword and a wave's access is one dword per bank --
// with the baseline bin B and the number of window values below it.  A run fills the histogram from the window of its
// first frame, then slides: per frame one value enters and one leaves, and B steps up or down until the rank falls into
// its bin.  Frames are read a dword per lane, DET_STAGE frames at a time (lane = 16 * frame + dword of the segment), and
// handed to the pixels' lanes through LDS; the results go back the same way and are stored as dwords.  Integers only.
// No lane leaves before the last barrier.
__global__ __launch_bounds__(64) void k_rec_running(RecRunning g)
{
    extern __shared__ unsigned det_lds[];
    const int lane = threadIdx.x;
    unsigned *hist = det_lds + lane;
    unsigned *st_in = det_lds + DET_HIST_DWORDS, *st_out = st_in + 64, *st_cur = st_out + 64, *st_res = st_cur + 64;
    const uint8_t *b_in = (const uint8_t *)st_in, *b_out = (const uint8_t *)st_out, *b_cur = (const uint8_t *)st_cur;
    uint8_t *b_res = (uint8_t *)st_res;
    const int sub = lane >> 4, dw = (g.seg0 + blockIdx.x) * 16 + (lane & 15);
    const bool dw_ok = dw < (g.b.pitch * g.b.bh) >> 2;             // (the last segment may end beyond the frame)
    const int runs = (g.n + g.run - 1) / g.run;
    // dword `dw` of frame f where it is wanted, else 0
    auto load = [&](int f, bool wanted) -> unsigned {
        return dw_ok && wanted ? *(const unsigned *)(d_rec_frame(g.b, g.chunks, f) + 4 * (size_t)dw) : 0u;
    };
    auto count = [&](int bin) -> int { return (int)((hist[(bin >> 1) * 64] >> (16 * (bin & 1))) & 0xFFFFu); };
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        const int ks = g.k0 + run * g.run, ke = min(ks + g.run, g.k0 + g.n);
        for (int i = 0; i < 128; i++) hist[i * 64] = 0u;
        // the window of the run's first frame
        const int a0 = max(0, ks - g.half), b0 = min(g.F - 1, ks + g.half);
        for (int f = a0; f <= b0; f += DET_STAGE) {
            __syncthreads();                                       // (the rows staged before have been read)
            st_in[lane] = load(f + sub, f + sub <= b0);
            __syncthreads();
            for (int j = 0; j < DET_STAGE && f + j <= b0; j++) {
                const unsigned v = b_in[64 * j + lane];
                hist[(v >> 1) * 64] += 1u << (16 * (v & 1u));
            }
        }
        int n = b0 - a0 + 1, B = 0, below = 0;                     // B's bin holds the rank once the walk below has run
        for (int k = ks; k < ke; k += DET_STAGE) {
            __syncthreads();
            // frame kk > ks: frame kk + half enters the window and frame kk - half - 1 leaves it, where they exist
            const int kl = k + sub, fi = kl + g.half, fo = kl - g.half - 1;
            st_in[lane] = load(fi, kl > ks && kl < ke && fi <= g.F - 1);
            st_out[lane] = load(fo, kl > ks && kl < ke && fo >= 0);
            st_cur[lane] = load(kl, kl < ke);
            __syncthreads();
            for (int j = 0; j < DET_STAGE && k + j < ke; j++) {
                const int kk = k + j;
                if (kk > ks) {
                    if (kk + g.half <= g.F - 1) {
                        const unsigned v = b_in[64 * j + lane];
                        hist[(v >> 1) * 64] += 1u << (16 * (v & 1u));
                        below += (int)v < B;
                        n++;
                    }
                    if (kk - g.half - 1 >= 0) {
                        const unsigned v = b_out[64 * j + lane];
                        hist[(v >> 1) * 64] -= 1u << (16 * (v & 1u));    // (the count was >= 1: no borrow)
                        below -= (int)v < B;
                        n--;
                    }
                }
                const int r = g.q * (n - 1) / 100;
                while (below > r && B > 0) {
                    B--;
                    below -= count(B);
                }
                for (int c = count(B); below + c <= r && B < 255; c = count(B)) {
                    below += c;
                    B++;
                }
                const unsigned v = b_cur[64 * j + lane], base = (unsigned)B, e = v > base ? v - base : 0u;
                unsigned o = base;
                if (g.what == 2) o = e;
                else if (g.what == 3) o = min(255u, (unsigned)g.gain * e / max(base, (unsigned)g.floor));
                b_res[64 * j + lane] = (uint8_t)o;
            }
            __syncthreads();
            if (dw_ok && k + sub < ke) *(unsigned *)(g.out + (size_t)(k + sub - g.k0) * g.b.fs + 4 * (size_t)dw) = st_res[lane];
        }
    }
}

// One box frame in the record's layout -> the registered plane (W x H, 0 outside the box), as k_body_warp leaves it for
// k_body_stats_add: 4 pixels per thread, linear as there.
__global__ __launch_bounds__(256) void k_rec_paste(int n, int W, RecBox b, const uint8_t *__restrict__ src, uint8_t *__restrict__ reg)
{
    const int p0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (p0 >= n) return;
    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int p = p0 + j;
        if (p >= n) break;
        const int y = p / W, x = p - y * W - b.c0, yb = y - b.r0;
        if (x >= 0 && x < b.bw && yb >= 0 && yb < b.bh) v[j] = src[(size_t)yb * b.pitch + x];
    }
    if (p0 + 4 <= n) *(unsigned *)(reg + p0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    else
        for (int j = 0; j < 4 && p0 + j < n; j++) reg[p0 + j] = (uint8_t)v[j];
}
