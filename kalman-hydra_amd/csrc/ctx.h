// The filter handle of libhydra_mi.so (hm_ctx) and the helpers every translation unit that works on one needs.  Private to
// the library: the filter's four files -- ekf.hip (handle, renders, measurement), update.hip (the dense update), mask.hip
// (pruning, outline, projection), predict_dev.hip (the prediction) -- and smooth.hip (the smoother), readout.hip (views,
// body-frame readout, statistics) and record.hip (the kept record) include it, all built by the one compiler command of the
// Makefile.  The filter's state is grouped by concern in structs, as the readout's is; each says which file writes it.  Everything defined here is
// static or a template; the hidden functions declared at the end are defined once, in the translation unit named there.
#pragma once
#include "hm_common.h"
#include "hm_types.h"
#include "host_block.h"
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// A persistent helper thread of a handle: it queues launches the calling thread does not have to wait for (the tail of
// hm_update_run: ~20 launches, ~80 us of host time at a frame boundary, where the caller's way to the NEXT frame's first
// launches is what the device ends up waiting for).  One job at a time; every entry point joins it first (ctx_join).
struct Helper {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool posted = false, busy = false, quit = false;
    int rc = HM_OK;
    char err[512] = "";
    void run()
    {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return quit || posted; });
            if (quit) return;
            posted = false;
            std::function<int()> f = std::move(job);
            lk.unlock();
            const int r = f();
            if (r != HM_OK) snprintf(err, sizeof err, "%s", hm_last_error());
            lk.lock();
            rc = r;
            busy = false;
            cv.notify_all();
        }
    }
    void post(std::function<int()> f)
    {
        std::unique_lock<std::mutex> lk(m);
        if (!th.joinable()) th = std::thread([this] { run(); });
        job = std::move(f);
        posted = busy = true;
        cv.notify_all();
    }
    // waits for the job in flight; its return code (reported once)
    int wait()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !busy; });
        const int r = rc;
        rc = HM_OK;
        return r;
    }
    void stop()
    {
        {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return !busy; });
            quit = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

// What hm_update_arm_newton / _arm_cov / _arm_mask arm, for the next hm_update_run only: that call takes the whole value out
// of the handle before anything can fail, so an error return never leaves a worker pointer or a mask address behind for a
// later call to start a job on.
struct Armed {
    bool newton = false;             // start the state prediction on `worker` when the state is final ...
    void *worker = nullptr;
    bool cov = false;                // ... and queue the covariance half of the next frame's prediction (with newton only)
    const uint8_t *mask = nullptr;   // queue this mask's outline when the state is final
};

// hm_view / hm_view_dev / hm_view_forces: targets of their own, allocated on first use -- a view touches nothing the
// filter reads (its render, triangle setups, state copy and wireframe counts are all here)
struct ViewState {
    Targets targets = {nullptr, nullptr, nullptr, nullptr};
    TriSetup *setup = nullptr;
    int *ids = nullptr, *lab = nullptr;
    unsigned *wire = nullptr, *mm = nullptr;
    double *X = nullptr, *force = nullptr;
    uint8_t *out = nullptr;
    hipEvent_t ev = nullptr;
    // hm_view_set_cells / hm_view_cells*: the cells in body coordinates (they stay until set again or cleared) ...
    int c_layers = 0, c_L = 0;       // layers 0: no cells set
    bool c_weighted = false;         // c_w holds weights (else 65535 everywhere)
    int *c_lab = nullptr;            // c_layers planes of W*H labels, -1: none
    uint16_t *c_w = nullptr;         // the same planes of weights
    uint8_t *c_col = nullptr;        // c_L x 3 colours, B G R
    uint8_t *c_outline = nullptr;    // W*H: the outline pixels of layer 0 (k_view_cell_outline)
    uint8_t *c_frame = nullptr;      // hm_view_cells' frame (W*H)
    // ... and what changes with every frame -- X (2N doubles) | points (2P doubles) | levels (c_L) | point colours (3P) --
    // copied into one of VIEW_CELL_SLOTS page-locked slots in turn and from there to c_in on the stream: the call returns
    // with the caller's arrays free, and waits only when the copy out of the slot it is about to fill is still to run
    uint8_t *c_in = nullptr;
    uint8_t *c_slot[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t c_slot_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool c_slot_used[4] = {false, false, false, false};
    int c_next = 0;
};
#define VIEW_CELL_SLOTS 4

// hm_body_*: the body-frame readout (body_kernels.h), buffers of its own allocated on first use -- it reads the state
// it is given and nothing else of the filter's
struct BodyState {
    bool ready = false;              // the body map and its counts are there
    TriSetup *setup = nullptr;
    double *uvX = nullptr, *X = nullptr;
    int *tri = nullptr;              // triangle per pixel (W*H), -1: none
    double2 *bary = nullptr;         // l1, l2 per pixel
    int4 *tidx = nullptr;            // vertex ids per triangle after the orientation swap
    unsigned *tcnt = nullptr;        // pixels per triangle
    std::vector<uint32_t> h_tcnt;
    std::vector<int> h_tri;          // the body map on the host (the record's box, and the pixel counts of discs and rings)
    int *lab = nullptr;              // the label image (W*H) of hm_body_set_labels; L labels, 0: none set
    int L = 0;
    unsigned *lcnt = nullptr;        // pixels per label
    uint8_t *frame = nullptr, *out = nullptr;           // hm_body_warp's frame and output (W*H, 3 W*H)
    unsigned long long *sum = nullptr;                  // hm_body_warp's sums: T per triangle, then L per label
    hipEvent_t ev = nullptr;         // recorded behind every queued warp (hm_body_warp_dev, hm_body_fence)
    // hm_body_stats_*: sums of the registered video over the warps queued between begin and end
    bool stats_on = false;
    int stats_frames = 0;            // frames added since hm_body_stats_begin
    int stats_cap = BODY_STATS_CAP;  // hm_ctx_tune "body_stats_cap" (tests lower it)
    // the registered plane (W*H) every warp writes while the statistics or the record are on.  Whichever of the two goes
    // last frees it: hm_body_stats_end unless rec.on, the record's end unless stats_on
    uint8_t *reg = nullptr;
    unsigned *stsum = nullptr;       // s1, s2, cross[4]: 6 planes of W*H, body_stats_stride values apart
    uint8_t *stmax = nullptr;        // W*H
    double *stimg = nullptr;         // mean, std, corr: 3 planes of W*H (hm_body_stats_images / _peaks)
    int *pkidx = nullptr, *pkcnt = nullptr;             // hm_body_stats_peaks: raster indices (W*H), their number
    double *pkscore = nullptr;
    // hm_deep_body_run (deep.hip, which borrows the map through body_map_view): the most entries of a column that one wave
    // of k_deep_cols walks; a longer column is cut into pieces of this many (hm_ctx_tune "deep_col_entries": same bytes
    // for every value)
    int deep_col_entries = 1024;
};

// hm_strain_*: the deformation readout (strain_kernels.h), buffers of its own, grown to the largest call so far
struct StrainState {
    double *X = nullptr;             // the states of a call (n_frames x 4N)
    double *v = nullptr;             // J, l1, l2, c2, s2, rc, rs per frame and triangle (n_frames x T x 7)
    int *off = nullptr, *ent_t = nullptr;            // cnt[s, t] of hm_strain_labels as compressed rows: L + 1 offsets, triangles,
    unsigned *ent_c = nullptr, *n_s = nullptr;       // their pixel counts; the map pixels per label (L)
    double *trace = nullptr;         // the traces per label (n_frames x L x 3)
};
#define STRAIN_MAX_GRID 2048         // workgroups of k_strain_tri / k_strain_label: they stride over what is beyond

// hm_body_rec_*: the registered video of the warps queued between begin and end, kept on the device (record.hip)
struct RecState {
    bool on = false;
    int frames = 0;                  // frames appended since hm_body_rec_begin
    int cap = 0;                     // frames the budget of hm_body_rec_begin holds
    int chunk = 0;                   // hm_ctx_tune "body_rec_chunk": frames per chunk (0: REC_CHUNK_BYTES worth; tests lower it)
    int tp_frames = 32;              // hm_ctx_tune "rec_tp_frames": frames per workgroup of hm_body_rec_trace_products
    int bl_frames = 256;             // hm_ctx_tune "rec_bl_frames": frames per run of k_rec_running (hm_body_rec_planes / _stats_add)
    int res_frames = 8;              // hm_ctx_tune "rec_res_frames": frames per run of k_rec_residual (hm_body_rec_residual_*)
    int map_frames = 64;             // hm_ctx_tune "rec_map_frames": frames per run of k_rec_trace_maps (hm_body_rec_trace_maps)
    int null_frames = 256;           // hm_ctx_tune "rec_null_frames": frames per run of k_rec_trace_null (hm_body_rec_trace_null)
    int tm_frames = 64;              // hm_ctx_tune "rec_tm_frames": frames per run of k_rec_tri_maps (hm_body_rec_tri_maps)
    int gram_bytes = 16384;          // hm_ctx_tune "rec_gram_bytes": bytes per run of k_rec_gram (hm_body_rec_gram)
    int wv_frames = 16;              // hm_ctx_tune "rec_wv_frames": events per launch of k_rec_wv_lat (hm_body_rec_waves)
    unsigned long long max = 0;      // the budget in bytes
    RecBox box = {0, 0, 0, 0, 0, 0, 0};
    std::vector<uint8_t *> chunks;
    uint8_t **tab = nullptr;         // the chunks' addresses for the reductions
    uint8_t *tmp = nullptr;          // their arguments and results
    size_t scr_bytes = (size_t)16 << 20;     // hm_ctx_tune "rec_scratch_bytes": the most scratch of a call (one frame at least; tests lower it)
    // a run of frames in the record's layout: as they were (hm_body_rec_shift / _warp), or the planes made of them
    // (hm_body_rec_planes / _stats_add / _residual_*); there while such a call runs, freed when it returns
    uint8_t *scr = nullptr;
    // hm_body_rec_event_*: the most bytes of the pool stack of a pass (hm_ctx_tune "rec_ev_bytes", one segment at least).
    // 16 GiB, the most the key admits: the kernels wait on dependent loads, so a pass is the faster the more waves it has
    // (the box of a 1024^2 frame with 2 000 frames, 18 GB of stack: 37.6 ms a call in two passes against 55 ms in five at
    // 4 GiB and 131 ms at 1 GiB).  The stack and the event bytes of the frames a call covers are
    // there while the call runs and freed when it returns.
    size_t ev_bytes = (size_t)16 << 30;
    uint8_t *ev = nullptr, *ev_out = nullptr;
    // hm_body_rec_waves: the map cut to the box, a launch's planes and results, the call's sums and, for kinds 1..3, a
    // window's planes; there while the call runs, freed when it returns
    uint8_t *wv = nullptr;
};

// ---- the filter's state, grouped as the readout's is.  Each struct says who writes it. ----------------------------------------

// The mask's pruning, its outline and projectmask (mask.hip; project_kernels.h), all allocated on first use (ready).  mask.hip
// writes it; ekf.hip marks outline_ready / prepared when the observation changes; hm_update_run takes the projection's block.
struct MaskState {
    int2 *d_outline = nullptr;       // outline pixels (W*H) ...
    int *d_outline_cnt = nullptr;    // ... and their counters
    uint8_t *d_mask = nullptr;       // a caller's host mask, uploaded (hm_project_mask, hm_prune_mask)
    uint8_t *d_flag = nullptr;       // border-pixel flags of the mask (W*H)
    uint8_t *d_pruned = nullptr;     // the mask after the reference's contour pruning (k_ccl_*): what the outline and the walk use
    Ccl ccl = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};     // its working arrays
    double *d_X = nullptr;           // hm_project_mask's copy of the state (second stream)
    double *pin = nullptr;           // page-locked: [X in (4N) | result block of 4N + 1 values: projected X, vertices moved] (k_project_mask_host)
    std::vector<double> v;           // the host's copy of that block
    int *d_done = nullptr;           // workgroups of k_project_mask_host that have finished
    long long ticket = 0;
    bool ready = false;              // project_buffers has built all of the above
    bool outline_ready = false;      // the outline of the resident mask (o_ym) has been queued on the second stream
    const uint8_t *prepared = nullptr;        // hm_prepare_mask: the outline in the buffers is that of this mask (device memory)
    hipEvent_t ev_outline = nullptr; // ... recorded behind every outline queued on the second stream
    hipEvent_t ev_pm = nullptr;      // the chained projection has run (hm_chain_project)
};

// hm_newton_dev_start / _finish: the state prediction's Newton loop as a four-wave kernel on a stream of its own
// (predict_dev.hip writes it; hm_update_run and hm_chain_project read the prediction in flight)
struct Newton4State {
    hipStream_t stream = nullptr;
    int *d_nbr = nullptr, *d_nbb = nullptr, *d_bars = nullptr;
    double *d_l0 = nullptr;
    int deg = 0;                     // padded degree of the table on the device (8 or 12), 0: this mesh does not fit the kernel
    std::vector<int32_t> bars;       // the springs the table was built for
    std::vector<double> l0;
    double *pin = nullptr;           // page-locked: [X in (4N) | result block of 4N + 2 values (host_block.h): X out, iterations, failed]
    double *d_X = nullptr;           // the same 4N + 2 values in device memory, for hm_chain_project
    std::vector<double> v;           // the host's copy of that block
    long long ticket = 0;
    bool pending = false;
    bool ready = false;              // hm_newton_dev_start's stream, blocks and event are there
    hipEvent_t ev = nullptr;         // the prediction's kernel has run
    int fail = 0;                    // test knob (hm_ctx_tune "newton_fail"): the next device predictions report a failed inner solve
};

// hm_ms_predict's own buffers (predict_dev.hip): the spring topology of k_ms_newton (bars, CSR of the bars of every vertex),
// its state and result words
struct NewtonState {
    int *d_bars = nullptr, *d_voff = nullptr, *d_vbar = nullptr, *d_info = nullptr;
    double *d_l0 = nullptr, *d_X = nullptr;
    bool ready = false;              // the fixed-size buffers are there and k_ms_newton may take its LDS
};

// hm_chain_project: projectmask of the prediction in flight queued behind it; the projected state (d_X0) is the
// prior mean of the next hm_update_run, which also collects what the two kernels report (update.hip writes the rest;
// pending is set by mask.hip and cleared by every call that starts or ends a prediction)
struct ChainState {
    bool pending = false;
    std::vector<double> pred, proj;  // ... the predicted / the projected state of the last chained update
    int its = 0, moved = 0;
};

// The spring topology of the covariance prediction on the device, kept between frames, and its host staging
// (predict_dev.hip: cov_predict_core, queue_predict_ahead)
struct SpringState {
    std::vector<int> h_off, h_bar, h_other;     // host staging of the topology: live until the copies ran
    std::vector<double> h_blk;
    std::vector<int32_t> bars_cached;           // the springs whose topology is on the device (d_off / d_bar / d_other)
    int *d_off = nullptr, *d_bar = nullptr, *d_other = nullptr;
    double *d_blk = nullptr;
    double *pin_blk = nullptr;       // page-locked staging of the spring blocks of the prediction queued ahead
};

// hm_update_arm_newton: the springs and parameters of the prediction the next hm_update_run starts (armed.newton);
// they stay: the tail on the helper thread reads them (update.hip)
struct ArmedPrediction {
    std::vector<int32_t> bars;
    std::vector<double> l0;
    double par[4] = {0, 0, 0, 0};    // kappa, M, dt, tol
    int maxiter = 0;
};

// hm_update_arm_cov: the covariance half of the next frame's prediction queued by hm_update_run itself ("pre-queued";
// predict_dev.hip writes it, every call that makes the prediction stale clears valid, hm_update_arm_cov sets eps_F)
struct QueuedPrediction {
    double eps_F = 0.0;
    bool valid = false;              // queued and not yet taken: d_Wprior / d_invW0 hold the prediction made from ...
    std::vector<double> X, l0;       // ... this state, these springs and parameters (kappa, a, s, eps_F)
    std::vector<int32_t> bars;
    double par[4] = {0, 0, 0, 0};
};

// The tail of hm_update_run -- covariance of the kept state, gains, their result block, and the covariance half of the
// NEXT frame's prediction (queue_predict_ahead) -- runs on a stream of its own: beside the measurement hm_update_run
// queued for an iteration that did not happen, and beside the next frame's reference render and measurement, which
// need none of its buffers.  on_stream4: it may still be running; `stream` waits for ev (on the device)
// before anything there touches the dense buffers (ctx_join; hm_update_run itself only before its first solve).
// (update.hip writes it; ctx_join clears on_stream4.)
struct TailState {
    int async = 1;                   // hm_ctx_tune "tail_async": the tail queued by the helper thread (same results)
    int split = 1;                   // hm_ctx_tune "tail_split": 0 keeps the tail on `stream` (same results either way)
    hipStream_t stream4 = nullptr;
    hipEvent_t ev = nullptr;
    bool on_stream4 = false;
    // the tail block of the last hm_update_run (Hz components, gains): taken by hm_update_tail, or by hm_update_run itself
    // when its caller wants them at once
    bool pending = false;
    // the tail block belongs to the last hm_update_run, which succeeded: false from the entry of every hm_update_run until it
    // has taken, queued or zero-filled the block (an update that fails leaves nothing for hm_update_tail to hand out)
    bool valid = false;
    long long ticket = 0;
    hipStream_t stream = nullptr;    // the stream that block's kernel is on
    std::vector<double> v;           // the host's copy of the block, taken when whole (hb_wait)
};

// hm_jz_multi / hm_j_multi (ekf.hip): id images of the reference and the two perturbed renders, the label palette (T),
// per-label boxes and sums; allocated on first use
struct MultiState {
    int *d_ids[3] = {nullptr, nullptr, nullptr};
    int *d_labels = nullptr;
    int4 *d_lbox = nullptr;
    double *d_lout = nullptr;
    std::vector<double> h_lout;
};

struct hm_ctx {
    int device = 0, W = 0, H = 0, N = 0, T = 0, E = 0, njobs = 0;
    HmOwner own{1};                  // every buffer, stream and event below (HYDRA_MI_POISON class 1)
    Helper helper;
    bool helper_used = false;
    double eps_Z = 0, eps_J = 0, eps_M = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the second stream (mask.hip's ensure_stream2): the mask's launches, hm_ms_predict's state prediction
    // mesh
    int *d_tri = nullptr, *d_star_off = nullptr, *d_star_tri = nullptr, *d_edges = nullptr;
    int *d_nb_off = nullptr, *d_nb_u = nullptr, *d_nb_e = nullptr;   // per vertex: neighbours (ascending) and their edge jobs (k_solve_prep)
    float *d_uv = nullptr;
    uint8_t *d_tex = nullptr;
    std::vector<int> edges;          // host copy, E*2
    std::vector<int> tri;            // host copy of the triangles (orientation test of hm_update_run)
    // observation
    uint8_t *d_yim = nullptr, *d_ym = nullptr;
    float *d_yfx = nullptr, *d_yfy = nullptr, *d_yfxm = nullptr, *d_yfym = nullptr;
    bool obs_owned = true;           // false when set_observation_dev aliases caller memory
    const uint8_t *o_yim = nullptr, *o_ym = nullptr;     // pointers in use (owned or caller's)
    const float *o_yfx = nullptr, *o_yfy = nullptr;
    bool have_tex = false, have_obs = false, have_ref = false;
    // renders and measurement
    Targets ref = {nullptr, nullptr, nullptr, nullptr}, P = {nullptr, nullptr, nullptr, nullptr}, Q = {nullptr, nullptr, nullptr, nullptr};
    TriSetup *d_setup = nullptr, *d_cfgs = nullptr;
    int4 *d_ubox = nullptr;
    int *d_tlist = nullptr, *d_tcount = nullptr;   // ... and the list / count of the tiles with a non-zero word
    unsigned *d_tmask = nullptr;     // per vertex and tile of its star region: the star triangles that can reach the tile (k_measure_vertex)
    double *d_X = nullptr, *d_out = nullptr, *d_partial = nullptr;
    uint8_t *d_im8 = nullptr, *d_m8 = nullptr;
    std::vector<double> X0;          // state of the reference render
    DPool pool = {};                 // parked difference images (see ekf_kernels.h)
    int *d_area = nullptr;
    std::vector<double> h_partial;
    int red_blocks = 512;
    double *d_tpart = nullptr;       // per-tile partial sums of Renderer.error from k_render_iter (tiles x 4)
    std::vector<double> h_tpart;
    int ntiles = 0;
    int render_rows = RI_H;          // strip height of k_render_iter (16 or 8)
    int vsplit = 5, esplit = 0;      // workgroups per vertex / per edge job of the measurement (hm_ctx_tune)
    // dense update on the device (n4 = 4N)
    double *d_HTH = nullptr;         // dense HTH of the last measurement: zero outside the J pattern (cleared once;
                                     // every pattern entry is rewritten by every measurement), used for nothing else
    double *d_H = nullptr, *d_Hz = nullptr, *d_Hzc = nullptr, *d_invW0 = nullptr, *d_Af[2] = {nullptr, nullptr}, *d_T[2] = {nullptr, nullptr},
           *d_step = nullptr, *d_Wtmp = nullptr, *d_X0 = nullptr, *d_Xn = nullptr, *d_Wprior = nullptr, *d_gain = nullptr, *d_Awork = nullptr,
           *d_Lt[2] = {nullptr, nullptr};
    std::vector<double> upd_X0;      // prior mean given to hm_update_begin
    int upd_last = -1, upd_prev = -1;   // which d_Af holds the factor of the last / previous step (-1: none)
    double *d_Wres = nullptr;        // the covariance resident on the device (the result of the last
                                     // hm_cov_predict / hm_update_cov / hm_update_run): d_Wtmp, d_H or
                                     // d_Wprior, or NULL when that buffer has been reused since
    double *pin = nullptr;           // page-locked, device-mapped: hm_update_run's result blocks (host_block.h) -- per iteration
                                     // [step (n4) | RES_HEAD values], then the tail block [Hzc (n4 x 4) | gains (3 x n4)], every value
                                     // a pair of words -- and two words of scratch (pin_scratch)
    size_t pin_n = 0;
    int *pin_scratch = nullptr;      // ... where hm_measure / hm_update_step have the pool's overflow flag copied to (with_pool_retry)
    std::vector<double> resv;        // the host's copy of an iteration's block, taken when whole (hb_wait)
    int result_delay = 0;            // test knob: the result kernels publish a block's last word first, the rest this many us later
    Armed armed;                     // hm_update_arm_*: taken whole by the next hm_update_run
    hipEvent_t ev_m0 = nullptr;      // the first measurement of an update has run (hm_update_arm_mask)
    bool upd_open = false;
    bool prefactored = false;        // d_invW0 is the inverse of the resident covariance d_Wprior (hm_update_prefactor)
    // Renderer.error of the state hm_update_run kept, against the raw flow, from the render of its last iteration
    // (hm_update_last_error): valid until the observation or anything else on the handle changes
    bool last_err_valid = false;
    double last_err[4] = {0, 0, 0, 0};
    std::vector<double> last_err_X;
    long long run_ticket = 0;        // sequence number of hm_update_run's per-iteration result blocks
    std::thread worker;              // hm_update_prefactor queues its launches from here while the caller predicts the state
    bool worker_active = false;
    int worker_rc = HM_OK;
    char worker_err[512] = "";
    // the factorisation as one persistent launch (chol_flow_kernels.h) / its workgroups.  (192 workgroups: 304.9 -> 306.9 us
    // per iteration with the filter alone, but 260.5 -> 264.2 and 318.6 -> 324.1 frames/s in the two benches -- the
    // workgroups that poll for blocks take issue slots from the flow's kernels on every compute unit they sit on; 160 and
    // 128 starve the chain: profiles/r04_ab_tunes.txt)
    int chol_flow = 1, flow_wgs = 192;
    int flow_stall = 0;              // test knob: FlowArgs.stall
    int speculate = 1;               // hm_update_run queues the next iteration's measurement before it knows that there is one
    double *d_flowP = nullptr;       // 3 x nb x 32 x 32 scratch of that launch
    unsigned *d_flowctl = nullptr;   // its task counter and time-out word
    // the filter's state by concern (the structs above)
    MaskState mask;
    Newton4State newton4;
    NewtonState newton;
    ChainState chain;
    SpringState sp;
    ArmedPrediction pn;
    QueuedPrediction pq;
    TailState tail;
    MultiState multi;
    // The readout: views, the body-frame readout with its statistics, the deformation readout, the kept record.  Each has buffers of its own, allocated
    // on first use through `own`, and touches nothing the filter reads (readout.hip and record.hip have the code and name no
    // other field of the handle than W, H, N, T, device, own, stream, d_tri, d_uv, d_tex and, for the overlay, have_tex,
    // have_obs, o_yim).
    ViewState view;
    BodyState body;
    StrainState strain;
    RecState rec;
};

static inline hipError_t alloc_targets(HmOwner &own, Targets &t, size_t n)
{
    hipError_t e = own.alloc(&t.acc, n * sizeof(int));
    if (e == hipSuccess) e = own.alloc(&t.fx, n * sizeof(float));
    if (e == hipSuccess) e = own.alloc(&t.fy, n * sizeof(float));
    if (e == hipSuccess) e = own.alloc(&t.cnt, n * sizeof(int));
    return e;
}

// the launches the helper thread is still queueing (the tail of the last update), and their failure, if any
static int helper_join(hm_ctx *h)
{
    if (h->helper_used) {
        const int rc = h->helper.wait();
        if (rc != HM_OK) { hm_set_error("%s", h->helper.err); return rc; }
    }
    return HM_OK;
}
// Every entry point waits for the launches hm_update_prefactor is still queueing (one handle = one
// stream = one thread at a time, as far as the device can tell) and reports their failure, if any.
static int ctx_join(hm_ctx *h, bool lazy = false)
{
    if (!h) return HM_OK;
    if (const int rc = helper_join(h)) return rc;
    if (!lazy && h->tail.on_stream4) {
        h->tail.on_stream4 = false;
        if (hipSetDevice(h->device) != hipSuccess || hipStreamWaitEvent(h->stream, h->tail.ev, 0) != hipSuccess) {
            hm_set_error("the handle's stream cannot wait for the tail of the last update");
            return HM_ERR_HIP;
        }
    }
    if (h->worker_active) {
        h->worker.join();
        h->worker_active = false;
        if (h->worker_rc != HM_OK) {
            const int rc = h->worker_rc;
            h->worker_rc = HM_OK;
            h->prefactored = false;
            hm_set_error("%s", h->worker_err);
            return rc;
        }
    }
    return HM_OK;
}
#define HM_JOIN(h) do { int _j = ctx_join(h); if (_j) return _j; } while (0)
// entry points of the frame loop that touch none of the tail's buffers (or wait for it themselves, where they do)
#define HM_JOIN_LAZY(h) do { int _j = ctx_join(h, true); if (_j) return _j; } while (0)

// Wait for the stream: poll it for a while (a few microseconds of latency) before falling back on
// hipStreamSynchronize, whose wake-up costs ~20 us -- three of those per frame on the compute() path.
// (A short pure spin, then the core is offered to other threads between polls: with several trackers
// per GPU plus their flow and prefactor helper threads on a CPU-quota'd host the pollers must not take
// the cores away from the threads that queue the launches.)
static inline hipError_t stream_wait(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    const auto t_yield = t0 + std::chrono::microseconds(50), t_give_up = t0 + std::chrono::milliseconds(20);
    bool polite = false;
    for (int spin = 0;; spin++) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (polite) std::this_thread::yield();
        else __builtin_ia32_pause();
        if ((spin & 15) == 15) {
            const auto now = std::chrono::steady_clock::now();
            if (now > t_give_up) return hipStreamSynchronize(s);
            polite = now > t_yield;
        }
    }
}

// Take values [first, first + n) of a result block in page-locked host memory (host_block.h) into `out` once every one of
// their pairs carries the launch's stamp.  The last pair is looked at first (one pair of loads per poll while nothing is
// there yet); a block of which some words are still missing is simply looked at again -- no order of arrival is assumed.
// A couple of microseconds against ~20 for waking up from a stream synchronisation, which remains as the fallback: after
// 20 ms the stream is waited for (everything queued behind the block's kernel included) and a block that is not whole
// then is an error.
static inline int hb_wait(hipStream_t st, const double *blk, size_t first, size_t n, unsigned long long stamp, double *out, const char *who)
{
    const volatile unsigned long long *canary = (const volatile unsigned long long *)blk + 2 * (first + n - 1);
    const auto t_start = std::chrono::steady_clock::now();
    const auto t_yield = t_start + std::chrono::microseconds(700), t_give_up = t_start + std::chrono::milliseconds(20);
    bool polite = false;
    for (int spin = 0;; spin++) {
        if ((canary[0] ^ canary[1]) == stamp && hb_take(blk, first, n, stamp, out)) return HM_OK;
        if (polite) std::this_thread::yield();
        else __builtin_ia32_pause();
        if ((spin & 255) == 255) {
            const auto now = std::chrono::steady_clock::now();
            if (now > t_give_up) break;
            polite = now > t_yield;
        }
    }
    HM_HIP(hipStreamSynchronize(st));
    if (hb_take(blk, first, n, stamp, out)) return HM_OK;
    hm_set_error("%s: a result block of the device is not whole although its stream has completed (stamp %016llx)", who, stamp);
    return HM_ERR_HIP;
}

// what an entry point of the filter needs to have been called before it
#define NEED_TEX(h, who) \
    if (!(h)->have_tex) { hm_set_error(who ": hm_set_texture has not been called"); return HM_ERR_STATE; }
#define NEED_OBS(h, who) \
    if (!(h)->have_obs) { hm_set_error(who ": hm_set_observation has not been called"); return HM_ERR_STATE; }
#define NEED_REF(h, who) \
    if (!(h)->have_ref) { hm_set_error(who ": hm_initjacobian has not been called"); return HM_ERR_STATE; }

template <typename T>
static int upload(HmOwner &own, T **dst, const T *src, size_t n)
{
    HM_HIP(own.alloc(dst, (n ? n : 1) * sizeof(T)));
    if (n) HM_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return HM_OK;
}

// n_layers planes of n labels each, every one within -1 .. L - 1.  n_layers 0: one plane, and the message names no layer.
static inline int hm_labels_ok(const char *who, int n_layers, const int32_t *labels, size_t n, int L)
{
    const size_t all = (size_t)(n_layers ? n_layers : 1) * n;
    for (size_t i = 0; i < all; i++) {
        if (labels[i] >= -1 && labels[i] < L) continue;
        if (n_layers) hm_set_error("%s: label %d at pixel %zu of layer %zu outside -1..%d", who, (int)labels[i], i % n, i / n, L - 1);
        else hm_set_error("%s: label %d at pixel %zu outside -1..%d", who, (int)labels[i], i, L - 1);
        return HM_ERR_ARG;
    }
    return HM_OK;
}

// The springs of every vertex (SpringTopo of k_fw_rows / k_pft_cols): off (N + 1) the CSR offsets, then per vertex its
// springs in the order of `bars` -- bar: the spring's id, other: the vertex at its other end.  Vertex ids are checked by
// the caller.  (Host arithmetic of the filter's prediction and of the smoother.)
static inline void spring_csr(int N, int n_bars, const int32_t *bars, std::vector<int> &off, std::vector<int> &bar,
                              std::vector<int> &other)
{
    off.assign(N + 1, 0);
    for (int i = 0; i < n_bars; i++) {
        off[bars[2 * i] + 1]++;
        off[bars[2 * i + 1] + 1]++;
    }
    for (int v = 0; v < N; v++) off[v + 1] += off[v];
    bar.resize(2 * (size_t)n_bars); other.resize(2 * (size_t)n_bars);
    std::vector<int> fill(off.begin(), off.end() - 1);
    for (int i = 0; i < n_bars; i++) {
        const int p = bars[2 * i], q = bars[2 * i + 1];
        bar[fill[p]] = i; other[fill[p]++] = q;
        bar[fill[q]] = i; other[fill[q]++] = p;
    }
}

// The per-spring blocks (Bxx, Bxy, Byy) of the force Jacobian at the vertices of X (kalman.py:892-901): bar i between
// a and b, d = y_a - y_b, l = |d|:  B = k I + c d d^T,  k = kappa (1 - l0/l),  c = kappa l0 / l^3.
static inline void spring_blocks(int n_bars, const int32_t *bars, const double *l0, double kappa, const double *X, double *blk)
{
    for (int i = 0; i < n_bars; i++) {
        const int a = bars[2 * i], b = bars[2 * i + 1];
        const double dx = X[2 * a] - X[2 * b], dy = X[2 * a + 1] - X[2 * b + 1];
        const double l = std::sqrt(dx * dx + dy * dy);
        const double k = kappa * (1.0 - l0[i] / l), c = kappa * l0[i] / (l * l * l);
        blk[3 * i] = k + c * dx * dx; blk[3 * i + 1] = c * dx * dy; blk[3 * i + 2] = k + c * dy * dy;
    }
}

// The filter's kernels that the readout launches (a view renders, the body map is a setup at X = uv).  Kernels are compiled
// by one translation unit each (ekf_kernels.h: ekf.hip), so readout.hip queues them through these, defined in ekf.hip:
// k_setup_all on T triangles of m at state X, and the full-frame render k_render<0> -- or k_render<1> with the label
// palette when ids is given -- on stream st.  Internal to the library: not in include/hydra_mi.h.
__attribute__((visibility("hidden"))) void ekf_queue_setup_all(hipStream_t st, const Mesh &m, const double *d_X, TriSetup *d_setup);
__attribute__((visibility("hidden"))) void ekf_queue_render(hipStream_t st, const Mesh &m, const double *d_X, const TriSetup *d_setup,
                                                            const Targets &out, const int *d_labels, int *d_ids);
// What crosses between the filter's own translation units, in the same way.  Defined in ekf.hip (the measurement):
// render_iter: the render of the device-resident state dX into t as one launch (k_render_iter), with the strips' partial sums
// of Renderer.error and, as extra workgroups, the star regions of the measurement at dX; render_strips: its strips;
// render_error_sums: those partial sums copied, waited for and added up into err (nothing stays in flight when it fails);
// measure_dev: the measurement at dX, whose render is in h->ref (ref_ready) or is put there -- scatter: the job sums also go
// to the dense HTH / Hz / Hzc; measure_on_device: the same at a host state, which becomes the state of the reference
// render; queue_star_regions: k_star_regions at dX alone; pool_grow: room for the star regions a measurement reported
// not to fit (the stream must be idle).
__attribute__((visibility("hidden"))) int render_iter(hm_ctx *h, const double *dX, Targets t, bool with_err, int masked, bool regions, double deltaX);
__attribute__((visibility("hidden"))) int render_strips(const hm_ctx *h);
__attribute__((visibility("hidden"))) int render_error_sums(hm_ctx *h, const char *who, double err[4]);
__attribute__((visibility("hidden"))) int measure_dev(hm_ctx *h, const double *dX, bool ref_ready, double deltaX, int masked,
                                                      bool regions_ready = false, bool scatter = true);
__attribute__((visibility("hidden"))) int measure_on_device(hm_ctx *h, const double *X, double deltaX, int masked, bool scatter = true);
__attribute__((visibility("hidden"))) int queue_star_regions(hm_ctx *h, const double *dX, double deltaX, int masked);
__attribute__((visibility("hidden"))) int pool_grow(hm_ctx *h, const char *who);
// Defined in update.hip (the dense update): the covariance half of hm_update_begin on stream st (NULL: the handle's) -- the
// prior (W_prior, or the resident covariance) into d_Wprior, its factor, inv(W) into d_invW0.
__attribute__((visibility("hidden"))) int prior_inverse(hm_ctx *h, const double *W_prior, hipStream_t st = nullptr);
#ifdef HM_STAMP
__attribute__((visibility("hidden"))) int update_debug_stamps(long long *dev_ptr);     // hm_debug_stamps: chol_flow_kernels.h' pointer
#endif
// Defined in mask.hip (pruning, outline, projection): the handle's second stream, made on first use; the pruning and the
// outline of a mask in device memory queued on it (the projection's buffers must be there: a non-NULL mask.d_outline says
// so); hm_prepare_mask behind its argument checks.
__attribute__((visibility("hidden"))) int ensure_stream2(hm_ctx *h);
__attribute__((visibility("hidden"))) int queue_outline(hm_ctx *h, const uint8_t *mask);
__attribute__((visibility("hidden"))) int prepare_mask(hm_ctx *h, const uint8_t *d_y_m);
// Defined in predict_dev.hip (the prediction): the covariance half of the NEXT frame's prediction from the state X that
// hm_update_run keeps, queued on st behind the covariance of that state (hm_update_arm_cov).
__attribute__((visibility("hidden"))) int queue_predict_ahead(hm_ctx *h, const double *X, int n_bars, const int32_t *bars, const double *l0,
                                                              double kappa, double M, double dt, double eps_F, hipStream_t st);

// A measurement whose star regions may not fit the pool of difference images: body() queues it and what hangs on it, the copy
// of the pool's overflow flag among them (pool_flag_queue), and returns with the stream idle.  When the flag is set the pool
// is grown and body() runs once more.  The flag lands in the handle's pinned block, not in a caller's frame: an error return
// must not leave a copy in flight towards a dead stack slot.
static inline int pool_flag_queue(hm_ctx *h)
{
    HM_HIP(hipMemcpyAsync(h->pin_scratch, h->pool.overflow, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return HM_OK;
}
template <typename Body>
static int with_pool_retry(hm_ctx *h, const char *who, Body body)
{
    for (int attempt = 0;; attempt++) {
        *h->pin_scratch = 0;
        HM_TRY(body());
        if (!*h->pin_scratch) return HM_OK;
        if (attempt) { hm_set_error("%s: the star regions do not fit the difference-image pool", who); return HM_ERR_STATE; }
        HM_TRY(pool_grow(h, who));
    }
}

// The filter's launch sequences that the smoother repeats (dense_kernels.h, chol_flow_kernels.h: update.hip), both defined in
// update.hip.  FP = F src by k_fw_rows, then dst = FP F^T + Weps by k_pft_cols, for the N vertices and springs tp.  The
// factorisation of a.A as one persistent launch, k_chol_flow on wgs workgroups, behind k_flow_fill unless the caller's
// own assembly pass has pre-filled its outputs (fill = false).
__attribute__((visibility("hidden"))) void ekf_queue_fpft(hipStream_t st, const double *src, double *FP, double *dst, int N,
                                                          const SpringTopo &tp, double a, double s, double eps_F);
__attribute__((visibility("hidden"))) void ekf_queue_chol_flow(hipStream_t st, const FlowArgs &a, int wgs, bool fill);

// What crosses between readout.hip (the warp, the statistics) and record.hip (the kept record), in the same way.  Defined in
// readout.hip: the body map, built once per handle; k_body_stats_add queued on the registered plane d_reg, and the frame
// counted.  Defined in record.hip: where the next frame of the record goes (allocates the chunk it starts; called before
// anything of a warp is queued, and may refuse: `who` names the caller in the error); k_rec_copy of the registered plane
// queued into that slot, and the frame counted.
__attribute__((visibility("hidden"))) int body_map_build(hm_ctx *h);
__attribute__((visibility("hidden"))) int body_stats_queue_add(hm_ctx *h, const uint8_t *d_reg);
__attribute__((visibility("hidden"))) int body_rec_slot(hm_ctx *h, const char *who, uint8_t **dst);
__attribute__((visibility("hidden"))) int body_rec_queue_copy(hm_ctx *h, uint8_t *dst);
