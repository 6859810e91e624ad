// 16-bit input mapped to 8 bits on the device (include/hydra_mi.h, "16-bit input").
//
//   k_deep_map   grid (blocks, frames of the run) x 256 threads.  A run is one dense block of 16-bit pixels, frame k at
//                element k n (n = W H), so with n odd a frame starts on a 2-byte boundary only.  The frame is therefore
//                cut where the *run's* 16-byte vectors lie: vector i of frame k is the elements [a0 + 8 i, a0 + 8 i + 8)
//                with a0 = k n rounded down to 8, clipped to the frame.  A vector that lies wholly inside the frame is
//                one 16-byte load; the clipped ones at a frame's two ends (and all of a 1 x 1 frame) are read an element
//                at a time.  Per pixel: the bytes exchanged when swap is set, the clip tests against lo and hi, the table
//                at min(max(v, lo), hi) -- only lut[lo .. hi] is ever read, hi - lo + 1 bytes that stay in the vector L1
//                -- then mask and shown.  Eight bytes of a plane go out as one 8-byte store where the address is a
//                multiple of 8 (the plane's base is, and k stride - k n is: always so in the frame ring, where stride =
//                n), else as bytes.  The clip counts are summed over the thread's pixels, then over the wave by
//                shuffles, then over the workgroup in two LDS words, and two threads add the non-zero sums to the
//                frame's two words.  A thread maps four vectors or more (the grid is at most 256 blocks a frame).
//   k_deep_hist  grid (chunks, 4) x 1024 threads, 64 KiB of LDS: 16384 32-bit bins, the quarter blockIdx.y of the range.
//                Workgroup (c, q) reads chunk c of the run and counts the pixels with v >> 14 == q, so every pixel is
//                read four times (from L2 after the first) and counted once.  Eight pixels a thread and round; for
//                pixel j of the eight the wave takes the value of its first counting lane, ballots the lanes that hold
//                the same value, and that lane adds their number in one LDS atomic; only the lanes with another value
//                add 1 each.  A constant frame thus costs one LDS atomic per wave and pixel slot, not 64 on one bin.
//                At the end the non-zero bins are added to the 64-bit global counts (global_atomic_add_x2).
//
// Integers only; plain HIP; every store is a vector store.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define DEEP_MAP_THREADS 256
#define DEEP_HIST_THREADS 1024
#define DEEP_HIST_BINS 16384                 // a quarter of the range: 64 KiB of 32-bit bins
#define DEEP_VEC 8                           // pixels per 16-byte vector

struct DeepOut {
    uint8_t *frame, *mask, *shown;           // mask and shown may be NULL
    size_t stride;                           // bytes from a frame's plane to the next frame's
    size_t n;                                // pixels of a frame
    unsigned lo, hi;
    int threshold;                           // mask = raw > threshold
    int swap;                                // exchange the two bytes of a pixel first
    int base8;                               // every plane's base address is a multiple of 8
};

__device__ __forceinline__ uint32_t deep_swap2(uint32_t w) { return ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu); }

__global__ __launch_bounds__(DEEP_MAP_THREADS) void k_deep_map(const uint16_t *__restrict__ in, const uint8_t *__restrict__ lut,
                                                                 DeepOut o, unsigned *__restrict__ clip)
{
    const size_t k = blockIdx.y, n = o.n;
    const size_t start = k * n, end = start + n;
    const size_t a0 = start & ~(size_t)(DEEP_VEC - 1);
    const size_t nvec = (end - a0 + DEEP_VEC - 1) / DEEP_VEC;
    const size_t plane = k * o.stride;
    const bool wide = o.base8 && ((plane - start) & 7) == 0;       // (plane + (a - start)) % 8 == 0 for a % 8 == 0
    __shared__ unsigned wg_clip[2];
    if (threadIdx.x < 2) wg_clip[threadIdx.x] = 0;
    __syncthreads();
    unsigned below = 0, above = 0;
    for (size_t i = (size_t)blockIdx.x * DEEP_MAP_THREADS + threadIdx.x; i < nvec; i += (size_t)gridDim.x * DEEP_MAP_THREADS) {
        const size_t a = a0 + i * DEEP_VEC;
        const bool full = a >= start && a + DEEP_VEC <= end;
        uint32_t w[4] = {0, 0, 0, 0};
        if (full) {
            const uint4 q = *reinterpret_cast<const uint4 *>(in + a);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            for (int j = 0; j < DEEP_VEC; j++)
                if (a + j >= start && a + j < end) w[j >> 1] |= (uint32_t)in[a + j] << (16 * (j & 1));
        }
        uint32_t raw[2] = {0, 0}, msk[2] = {0, 0}, shw[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < DEEP_VEC; j++) {
            const uint32_t ww = o.swap ? deep_swap2(w[j >> 1]) : w[j >> 1];
            const unsigned v = (ww >> (16 * (j & 1))) & 0xffffu;
            const bool live = full || (a + j >= start && a + j < end);
            below += (live && v < o.lo) ? 1u : 0u;
            above += (live && v > o.hi) ? 1u : 0u;
            const unsigned r = live ? lut[min(max(v, o.lo), o.hi)] : 0u;
            const unsigned m = (int)r > o.threshold ? 1u : 0u;
            raw[j >> 2] |= r << (8 * (j & 3));
            msk[j >> 2] |= m << (8 * (j & 3));
            shw[j >> 2] |= (m ? r : 0u) << (8 * (j & 3));
        }
        if (full && wide) {
            const size_t at = plane + (a - start);
            *reinterpret_cast<uint2 *>(o.frame + at) = make_uint2(raw[0], raw[1]);
            if (o.mask) *reinterpret_cast<uint2 *>(o.mask + at) = make_uint2(msk[0], msk[1]);
            if (o.shown) *reinterpret_cast<uint2 *>(o.shown + at) = make_uint2(shw[0], shw[1]);
        } else {
            for (int j = 0; j < DEEP_VEC; j++) {
                if (a + j < start || a + j >= end) continue;
                const size_t at = plane + (a + j - start);
                o.frame[at] = (uint8_t)(raw[j >> 2] >> (8 * (j & 3)));
                if (o.mask) o.mask[at] = (uint8_t)(msk[j >> 2] >> (8 * (j & 3)));
                if (o.shown) o.shown[at] = (uint8_t)(shw[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {                             // the wave's sums, before any atomic
        below += __shfl_xor(below, d);
        above += __shfl_xor(above, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (below) atomicAdd(&wg_clip[0], below);
        if (above) atomicAdd(&wg_clip[1], above);
    }
    __syncthreads();
    // one global atomic per workgroup and count: every frame's two words lie in one 64-byte line, and an add per wave
    // (16384 a frame at 1024 x 1024) onto that line took 377 us a run of 8 frames, all of it waiting for the line
    if (threadIdx.x < 2 && wg_clip[threadIdx.x]) atomicAdd(&clip[2 * k + threadIdx.x], wg_clip[threadIdx.x]);
}

__global__ __launch_bounds__(DEEP_HIST_THREADS) void k_deep_hist(const uint16_t *__restrict__ in, size_t total, size_t per, int swap,
                                                                   unsigned long long *__restrict__ hist)
{
    __shared__ unsigned bins[DEEP_HIST_BINS];
    const unsigned q = blockIdx.y;
    for (unsigned i = threadIdx.x; i < DEEP_HIST_BINS; i += DEEP_HIST_THREADS) bins[i] = 0;
    __syncthreads();
    const size_t c0 = (size_t)blockIdx.x * per;                    // per is a multiple of 8: c0 is a vector's start
    const size_t c1 = c0 + per < total ? c0 + per : total;
    const unsigned lane = threadIdx.x & 63;
    // (the same number of rounds for every thread of the workgroup: the ballots below need whole waves)
    for (size_t r0 = c0; r0 < c1; r0 += (size_t)DEEP_HIST_THREADS * DEEP_VEC) {
        const size_t a = r0 + (size_t)threadIdx.x * DEEP_VEC;
        uint32_t w[4] = {0, 0, 0, 0};
        if (a + DEEP_VEC <= c1) {
            const uint4 x = *reinterpret_cast<const uint4 *>(in + a);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else {
            for (int j = 0; j < DEEP_VEC; j++)
                if (a + j < c1) w[j >> 1] |= (uint32_t)in[a + j] << (16 * (j & 1));
        }
#pragma unroll
        for (int j = 0; j < DEEP_VEC; j++) {
            const uint32_t ww = swap ? deep_swap2(w[j >> 1]) : w[j >> 1];
            const unsigned v = (ww >> (16 * (j & 1))) & 0xffffu;
            const bool mine = a + j < c1 && (v >> 14) == q;
            const unsigned long long counting = __ballot(mine);
            if (counting == 0) continue;                           // (the whole wave)
            const int leader = __ffsll((long long)counting) - 1;
            const unsigned first = (unsigned)__shfl((int)v, leader);
            const unsigned long long same = __ballot(mine && v == first);
            if (lane == (unsigned)leader) atomicAdd(&bins[first & (DEEP_HIST_BINS - 1)], (unsigned)__popcll(same));
            else if (mine && v != first) atomicAdd(&bins[v & (DEEP_HIST_BINS - 1)], 1u);
        }
    }
    __syncthreads();
    unsigned long long *dst = hist + (size_t)q * DEEP_HIST_BINS;
    for (unsigned i = threadIdx.x; i < DEEP_HIST_BINS; i += DEEP_HIST_THREADS) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&dst[i], (unsigned long long)c);
    }
}
