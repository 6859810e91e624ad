// Events per pixel of the kept registered video: AR(1) deconvolution of every box pixel's sequence of planes
// (hm_body_rec_event_planes, hm_body_rec_event_stats_add, hm_body_rec_event_sums; hydra_mi/events.py; tests/events_ref.py
// restates all of it in Python floats).  include/hydra_mi.h has the rule word for word; binary64 in exactly its order, the
// library is built with -ffp-contract=off, and a lane works through its pixel frame by frame.
//
// The pool stack of a pass of P = 64 nseg pixels lies in a device work buffer of frame-major planes (pixel pl of frame t at
// t P + pl, so the lanes of a wave that are at the same frame touch one line):
//   v, w     doubles, at the pool's start frame
//   len      uint16, the pool's length, at its start frame
//   start    uint16, the pool's start frame, at its end frame
// 20 bytes per frame and pixel.  The pool on top of a lane's stack is in registers while a launch runs; a launch ends by
// writing it to the planes, and the next one takes it up from there (start[k0 - 1] names it), so the frames may arrive in
// batches of any length.  What lies at frames that are no pool's start or end any more is stale and never read: the walk
// goes from a pool's start to its end by len, and from a pool's start to the pool below by start[t - 1].
#pragma once
#include "detrend_kernels.h"

#define EV_FMAX 65535                  // frames of a record: the planes len and start hold frame numbers in 16 bits
#define EV_PX_BYTES 20                 // bytes of the pool stack per frame and pixel
#define EV_BYTES_MAX (1ll << 34)       // hm_ctx_tune "rec_ev_bytes" at most

struct RecEvents {
    RecBox b;
    const uint8_t *const *chunks;      // the record: the source of kind 0
    const uint8_t *src;                // planes of kind 1..3 in the record's layout, frame ks first; NULL: the record
    int ks;
    int F;                             // frames of the record
    int seg0, nseg;                    // the pass: the 64-byte segments seg0 .. seg0 + nseg - 1 of the box frame
    double g, mu, lam;                 // mu = lam (1 - g)
    const double *pw, *pw2;            // g^l and its square, l = 0 .. F (formed on the host by repeated multiplication)
    double *v, *w;                     // the planes of the pool stack, F x 64 nseg each
    uint16_t *len, *start;
};

// a > 0 ? a : +0 (also for -0 and NaN)
__device__ __forceinline__ double d_ev_pos(double a) { return a > 0.0 ? a : 0.0; }

// Frames k0 .. k0 + m - 1 pushed onto the stacks of the pass: one wave per segment, a lane per box pixel.  Frame k's pool
// (y - mu, 1, k, 1) -- (y - lam) for the last frame of the record -- merges into the pool below it while
// v_b < pw[l_a] v_a; the first such pool is the old top in registers, further ones are loaded through start[t - 1].  The
// old top is written to the planes only when the new pool stays on top of it.  No LDS, no barrier, no atomics.
__global__ __launch_bounds__(64) void k_rec_ev_push(RecEvents e, int k0, int m)
{
    const int lane = threadIdx.x;
    const size_t P = (size_t)e.nseg * 64, pl = (size_t)blockIdx.x * 64 + lane;
    const size_t i = ((size_t)e.seg0 + blockIdx.x) * 64 + lane;           // the pixel's byte in a box frame
    const bool ok = i < (size_t)e.b.pitch * e.b.bh;                       // (the last segment may end beyond the frame)
    double vb = 0.0, wb = 0.0;                                            // the top pool; lb 0: none yet
    int tb = 0, lb = 0;
    if (k0 > 0) {
        tb = e.start[(size_t)(k0 - 1) * P + pl];
        const size_t o = (size_t)tb * P + pl;
        vb = e.v[o]; wb = e.w[o]; lb = e.len[o];
    }
    for (int k = k0; k < k0 + m; k++) {
        const uint8_t *f = e.src ? e.src + (size_t)(k - e.ks) * e.b.fs : d_rec_frame(e.b, e.chunks, k);
        const double y = ok ? (double)f[i] : 0.0;
        double vt = y - (k == e.F - 1 ? e.lam : e.mu), wt = 1.0;          // the new pool ...
        int tt = k, lt = 1;
        double va = vb, wa = wb;                                          // ... and the one below it (la 0: none)
        int ta = tb, la = lb;
        bool merged = false;
        while (la > 0) {
            const double pa = e.pw[la];
            if (!(vt < pa * va)) break;
            const double num = wa * va + (pa * wt) * vt, den = wa + e.pw2[la] * wt;
            vt = num / den; wt = den; tt = ta; lt += la;
            merged = true;
            la = 0;
            if (tt > 0) {
                ta = e.start[(size_t)(tt - 1) * P + pl];
                const size_t o = (size_t)ta * P + pl;
                va = e.v[o]; wa = e.w[o]; la = e.len[o];
            }
        }
        if (!merged && lb > 0) {                                          // the old top stays a pool of its own
            const size_t o = (size_t)tb * P + pl;
            e.v[o] = vb; e.w[o] = wb; e.len[o] = (uint16_t)lb;
            e.start[(size_t)(k - 1) * P + pl] = (uint16_t)tb;
        }
        vb = vt; wb = wt; tb = tt; lb = lt;
    }
    if (m > 0) {
        const size_t o = (size_t)tb * P + pl;
        e.v[o] = vb; e.w[o] = wb; e.len[o] = (uint16_t)lb;
        e.start[(size_t)(k0 + m - 1) * P + pl] = (uint16_t)tb;
    }
}

// The readout of the pass once all F frames are pushed: a lane walks its pools from frame 0 upwards.  s is not zero at the
// start of a pool i > 0 only: s = pos(pos(v_i) - g (pos(v_{i-1}) pw[l_{i-1} - 1])).  E (NULL: not wanted) holds the frames
// k0 .. k0 + n - 1 in the record's layout, zeroed before the launch: the lane stores the bytes that are not zero.  cnt and
// sum (either may be NULL) are indexed by the pixel's byte in a box frame; with s_min = 0 every frame counts.
__global__ __launch_bounds__(64) void k_rec_ev_read(RecEvents e, int k0, int n, uint8_t *E, double s_min, unsigned *cnt, double *sum)
{
    const int lane = threadIdx.x;
    const size_t P = (size_t)e.nseg * 64, pl = (size_t)blockIdx.x * 64 + lane;
    const size_t i = ((size_t)e.seg0 + blockIdx.x) * 64 + lane;
    if (i >= (size_t)e.b.pitch * e.b.bh) return;                          // (no barrier in this kernel)
    unsigned c = 0;
    double S = 0.0, tail = 0.0;                                           // pos(v) pw[l - 1] of the pool before
    for (int t = 0; t < e.F;) {
        const size_t o = (size_t)t * P + pl;
        const double vi = d_ev_pos(e.v[o]);
        const int l = e.len[o];
        if (l < 1) break;                                                 // (every pool has a frame: the walk cannot stand still)
        if (t > 0) {
            const double s = d_ev_pos(vi - e.g * tail);
            c += s >= s_min;
            S += s;
            if (E && t >= k0 && t < k0 + n) {
                const double r = floor(s + 0.5);
                const unsigned byte = r >= 255.0 ? 255u : (unsigned)r;
                if (byte) E[(size_t)(t - k0) * e.b.fs + i] = (uint8_t)byte;
            }
        }
        tail = vi * e.pw[l - 1];
        t += l;
    }
    if (cnt) cnt[i] = s_min == 0.0 ? (unsigned)e.F : c;
    if (sum) sum[i] = S;
}
