// Activity waves on the kept record (hm_body_rec_waves; include/hydra_mi.h has the rule, DESIGN.md section 27 the
// reasons; hydra_mi/waves.py; tests/waves_ref.py restates all of it in NumPy and Python integers).  Exact integers throughout.
//
// Per event and box pixel: the binned value Y_k(p) over the event's window of frames, its baseline sum, its maximum, the
// frame at which it crosses half of its rise and the sub-frame latency of that crossing (k_rec_wv_lat); per pixel the
// count and the sums of the valid latencies over the events (k_rec_wv_sums); per event and node of a grid the nine sums
// of a local plane fit of the latency (k_rec_wv_fit).  All planes here are in the record's layout: bh rows of `pitch`
// values, the padding off the map.
#pragma once
#include "roi_kernels.h"         // (d_rec_frame, d_wave_sum64; REC_WV_MAX: hm_types.h)

#define REC_WV_BMAX 8                  // the largest bin radius: windows of 17 x 17
#define REC_WV_PRE_MAX 64
#define REC_WV_LEAD_MAX 64
#define REC_WV_POST_MAX 256
#define REC_WV_EMAX 65536              // the most events of a call: sum Lat^2 < 2^33 x 2^16 stays below 2^63
#define REC_WV_STEP_MAX 64
#define REC_WV_RF_MAX 16
#define REC_WV_NONE INT32_MIN          // the latency where there is none (why >= 2)
#define WV_TW 32                       // a workgroup's tile of box pixels: 32 columns x 8 rows, a pixel per thread
#define WV_TH 8
#define WV_HW (WV_TW + 2 * REC_WV_BMAX)          // the tile with its halo at the largest bin
#define WV_HH (WV_TH + 2 * REC_WV_BMAX)

// m(p): 1 on the map, 0 off it and in the padding; a thread per value of a box plane
__global__ __launch_bounds__(256) void k_rec_wv_mask(int W, RecBox b, const int *__restrict__ tri_of, uint8_t *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= b.pitch * b.bh) return;
    const int y = i / b.pitch, x = i - y * b.pitch;
    mask[i] = x < b.bw && tri_of[(size_t)(b.r0 + y) * W + b.c0 + x] >= 0;          // (the padding may lie beyond the frame)
}

// n(p): the map pixels of the (2 bin + 1)^2 window round p, 0 where p is off the map.  Once per call: no tile needed.
__global__ __launch_bounds__(256) void k_rec_wv_nbin(RecBox b, int bin, const uint8_t *__restrict__ mask, uint16_t *__restrict__ nbin)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= b.pitch * b.bh) return;
    const int y = i / b.pitch, x = i - y * b.pitch;
    int n = 0;
    if (mask[i])
        for (int yy = max(y - bin, 0); yy <= min(y + bin, b.bh - 1); yy++)
            for (int xx = max(x - bin, 0); xx <= min(x + bin, b.bw - 1); xx++) n += mask[yy * b.pitch + xx];
    nbin[i] = (uint16_t)n;
}

struct RecWaves {
    RecBox b;
    const uint8_t *const *chunks;      // kind 0: the record's chunks
    const uint8_t *src;                // kinds 1..3: the planes of the frames ks, ks + 1, ... in the record's layout; NULL: the record
    int ks;
    int bin, pre, lead, post, min_rise;
    const int *trig;                   // the launch's trigger frames, one per blockIdx.y
    const uint8_t *mask;               // m(p)
    const uint16_t *nbin;              // n(p)
    int *lat, *rise;                   // per event of the launch a plane of pitch * bh each
    uint8_t *why;
};

// (a) Latency, rise and code of every box pixel of a tile (blockIdx.x) in one event (blockIdx.y).  A frame's tile with
// its halo of `bin` goes through LDS, masked by the map: rows are summed first (sh), then columns, so a pixel reads
// 2 (2 bin + 1) values and not (2 bin + 1)^2.  The window is walked twice -- S, M and k_M first, then the crossing, whose
// threshold needs M -- and nothing of Y is kept between the walks.  Every thread stays to the end (the barriers).
__global__ __launch_bounds__(256) void k_rec_wv_lat(RecWaves g)
{
    __shared__ uint8_t sm[WV_HW * WV_HH];          // the map over the tile and its halo (0 beyond the box)
    __shared__ uint8_t sy[WV_HW * WV_HH];          // a frame's values there, 0 off the map
    __shared__ uint16_t sh[WV_TW * WV_HH];         // their sums along the rows: <= 17 x 255
    const RecBox &b = g.b;
    const int tiles_x = (b.bw + WV_TW - 1) / WV_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * WV_TW - g.bin, y0 = ty * WV_TH - g.bin;          // the halo's corner in the box
    const int hw = WV_TW + 2 * g.bin, hh = WV_TH + 2 * g.bin, n1 = 2 * g.bin + 1;
    const int tid = threadIdx.x, lx = tid & (WV_TW - 1), ly = tid / WV_TW;
    const int x = tx * WV_TW + lx, y = ty * WV_TH + ly;
    const bool in = x < b.bw && y < b.bh;
    const int e = blockIdx.y, t = g.trig[e];
    const size_t nb = (size_t)b.pitch * b.bh, pi = in ? (size_t)y * b.pitch + x : 0;

    for (int i = tid; i < hw * hh; i += 256) {
        const int yy = y0 + i / hw, xx = x0 + i % hw;
        sm[i] = xx >= 0 && xx < b.bw && yy >= 0 && yy < b.bh ? g.mask[yy * b.pitch + xx] : (uint8_t)0;
    }
    __syncthreads();
    // Y_k of this thread's pixel; all threads call it together
    auto binned = [&](int k) -> int {
        const uint8_t *f = g.src ? g.src + (size_t)(k - g.ks) * b.fs : d_rec_frame(b, g.chunks, k);
        for (int i = tid; i < hw * hh; i += 256) {
            const int yy = y0 + i / hw, xx = x0 + i % hw;
            sy[i] = sm[i] ? f[yy * b.pitch + xx] : (uint8_t)0;            // (sm is 0 beyond the box: nothing read there)
        }
        __syncthreads();
        for (int i = tid; i < WV_TW * hh; i += 256) {
            const int r = i / WV_TW, c = i - r * WV_TW;
            int s = 0;
            for (int d = 0; d < n1; d++) s += sy[r * hw + c + d];
            sh[i] = (uint16_t)s;
        }
        __syncthreads();          // (the next frame's sy is written behind this barrier, its sh behind the next one)
        int Y = 0;
        for (int d = 0; d < n1; d++) Y += sh[(ly + d) * WV_TW + lx];
        return Y;
    };

    const int kb = t - g.lead, kc = t + g.post;
    int S = 0, M = -1, kM = kb;
    for (int k = kb - g.pre; k < kb; k++) S += binned(k);
    for (int k = kb; k <= kc; k++) {
        const int Y = binned(k);
        if (Y > M) { M = Y; kM = k; }          // (the first frame that attains the maximum)
    }
    const int R = g.pre * M - S, theta = S + g.pre * M, p2 = 2 * g.pre;
    int kx = -1, Yx = 0, Y1 = 0, prev = 0;
    for (int k = kb; k <= kc; k++) {
        const int Y = binned(k);
        if (kx < 0 && p2 * Y >= theta) { kx = k; Yx = Y; Y1 = prev; }
        prev = Y;
    }
    if (!in) return;
    const int n = g.nbin[pi];
    int why, lat = REC_WV_NONE, rise = R;
    if (!g.mask[pi]) { why = 255; rise = 0; }
    else if (R < g.pre * n * g.min_rise) why = 2;          // (R < 0 has no crossing and ends here)
    else if (kx == kb) why = 3;
    else {
        why = kM == kc ? 1 : 0;
        const unsigned d0 = (unsigned)(theta - p2 * Y1), d1 = (unsigned)(p2 * (Yx - Y1));      // d1 >= d0 > 0; 256 d0 < 2^32
        lat = 256 * (kx - 1 - t) + (int)(256u * d0 / d1);
    }
    const size_t o = (size_t)e * nb + pi;
    g.lat[o] = lat; g.rise[o] = rise; g.why[o] = (uint8_t)why;
}

// (b) The valid latencies of a launch's events added to the call's sums: a thread owns a pixel, so any order of the
// events and of the launches gives the same integers.  The padding of a row, which k_rec_wv_lat does not write, is not read.
__global__ __launch_bounds__(256) void k_rec_wv_sums(RecBox b, int events, const int *__restrict__ lat, unsigned *__restrict__ cnt,
                                                    long long *__restrict__ s1, long long *__restrict__ s2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t nb = (size_t)b.pitch * b.bh;
    if ((size_t)i >= nb || i % b.pitch >= b.bw) return;
    unsigned c = 0;
    long long a1 = 0, a2 = 0;
    for (int e = 0; e < events; e++) {
        const int l = lat[(size_t)e * nb + i];
        if (l != REC_WV_NONE) { c++; a1 += l; a2 += (long long)l * l; }
    }
    cnt[i] += c; s1[i] += a1; s2[i] += a2;
}

// (c) The nine sums of a node (blockIdx.x) in an event (blockIdx.y) over its window of (2 Rf + 1)^2 pixels: a wave per
// node, the lanes stride over the window, then the wave adds up.  The node itself may lie off the map or, with its
// window, beyond the box: only pixels of the box can be valid.
__global__ __launch_bounds__(64) void k_rec_wv_fit(RecBox b, int step, int Rf, int nx, const int *__restrict__ lat,
                                                   long long *__restrict__ fit)
{
    const int j = blockIdx.x / nx, i = blockIdx.x - j * nx, e = blockIdx.y;
    const int cx = i * step, cy = j * step, n1 = 2 * Rf + 1;
    const size_t nb = (size_t)b.pitch * b.bh;
    const int *l = lat + (size_t)e * nb;
    long long s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = threadIdx.x; w < n1 * n1; w += 64) {
        const int dy = w / n1 - Rf, dx = w % n1 - Rf;
        const int x = cx + dx, y = cy + dy;
        if (x < 0 || x >= b.bw || y < 0 || y >= b.bh) continue;
        const int v = l[(size_t)y * b.pitch + x];
        if (v == REC_WV_NONE) continue;
        s[0] += 1; s[1] += dx; s[2] += dy; s[3] += dx * dx; s[4] += dx * dy; s[5] += dy * dy;
        s[6] += v; s[7] += (long long)dx * v; s[8] += (long long)dy * v;
    }
#pragma unroll
    for (int q = 0; q < 9; q++) s[q] = (long long)d_wave_sum64((unsigned long long)s[q]);
    if (threadIdx.x < 9) {
        long long v = s[0];
#pragma unroll
        for (int q = 1; q < 9; q++) v = (int)threadIdx.x == q ? s[q] : v;
        fit[((size_t)e * gridDim.x + blockIdx.x) * 9 + threadIdx.x] = v;
    }
}
