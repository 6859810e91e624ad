/*
 * hydra_mi.h -- C-ABI of libhydra_mi.so, the MI355X (gfx950) implementation of
 * HydraGL's per-frame hot loop: Brox optical flow followed by the EKF
 * measurement update of a textured triangle mesh.
 *
 * Every entry point is what the reference's binding for this path would call
 * through ctypes; the reference interface each one replaces is cited as
 * reference file:line.  Conventions:
 *   - plain pointers and sizes only; all host arrays are C-contiguous and owned
 *     by the caller, the library copies in/out; device buffers are owned by the
 *     handle and freed by *_destroy;
 *   - every call returns 0 on success and a negative code on error; the text of
 *     the last error of the calling thread is hm_last_error();
 *   - one handle <-> one HIP stream <-> one host thread; the host-pointer calls
 *     are synchronous at return (the reference synchronises after every launch,
 *     cuda_multi.py:793,804,1083); the *_dev calls enqueue on the handle's
 *     stream and return, hm_*_sync waits.
 */
#ifndef HYDRA_MI_H
#define HYDRA_MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_OK 0
#define HM_ERR_ARG (-1)     /* bad argument (reference: Python exception / assert) */
#define HM_ERR_HIP (-2)     /* HIP runtime failure, including "no GPU" */
#define HM_ERR_STATE (-3)   /* call sequence error, e.g. jz before initjacobian (cuda_multi.py:611) */
#define HM_ERR_NUMERIC (-4) /* the update system is not positive definite (non-finite input) */

const char *hm_last_error(void);
const char *hm_version(void);
/* number of visible HIP devices, or a negative error code */
int hm_device_count(void);

/* Device buffers for callers that keep frames / flow planes resident in HBM between calls (the
 * *_dev entry points below; the in-process flow -> EKF pipeline).  Counterpart of the reference's
 * cv::cuda::GpuMat uploads (src/optical_flow_ext.cpp:296-299) and gpuarray.to_gpu
 * (cuda_multi.py:760-790).  upload / download are synchronous. */
int hm_dev_alloc(int device, uint64_t bytes, void **out);
int hm_dev_free(int device, void *ptr);
int hm_dev_upload(int device, void *dst, const void *src, uint64_t bytes);
int hm_dev_download(int device, void *dst, const void *src, uint64_t bytes);
/* Streaming uploads (the frame loop of run_kalmanfilter.py:78-89 reads one frame per iteration): a copy
 * stream of the caller, page-locked host staging memory, and an asynchronous host -> device copy on that
 * stream; hm_copy_stream_sync waits for the copies queued so far. */
int hm_copy_stream_create(int device, void **stream_out);
int hm_copy_stream_destroy(int device, void *stream);
int hm_copy_stream_sync(int device, void *stream);
int hm_host_alloc(uint64_t bytes, void **out);
int hm_host_free(void *ptr);
int hm_dev_upload_async(int device, void *dst, const void *src, uint64_t bytes, void *stream);
/* ... and back: device -> page-locked host memory on the caller's copy stream (the video of the pipeline) */
int hm_dev_download_async(int device, void *dst, const void *src, uint64_t bytes, void *stream);
/* ... and device -> device on that stream (the frame ring's mirror slots when the frames are decoded on the device) */
int hm_dev_copy_async(int device, void *dst, const void *src, uint64_t bytes, void *stream);

/* ------------------------------------------------------------------------
 * Brox optical flow.  Replaces cv::cuda::BroxOpticalFlow as used by
 * processflow_gpu (src/optical_flow_ext.cpp:294-331).
 * ---------------------------------------------------------------------- */
typedef struct hm_brox *hm_brox_t;

/* cuda::BroxOpticalFlow::create(alpha, gamma, scale_factor, inner, outer, solver)
 * (src/optical_flow_ext.cpp:310; parameter meaning :300-308; defaults :453-488).
 * max_batch = number of frame pairs one calc_batch call may carry.
 * HM_ERR_ARG, before anything is allocated, when a pyramid level would be 1x1 px
 * (a 1x1 frame, or a scale_factor that shrinks a level to one pixel): its flow is undefined. */
int hm_brox_create(int device, int width, int height, int max_batch,
                   float alpha, float gamma, float scale_factor,
                   int inner_iterations, int outer_iterations, int solver_iterations,
                   hm_brox_t *out);
int hm_brox_destroy(hm_brox_t h);

/* brox->calc(frame0f, frame1f, flow) + split + download
 * (src/optical_flow_ext.cpp:314-328): two 8-bit gray frames in, flowx / flowy
 * (row-major f32, width*height each) out.  Host pointers. */
int hm_brox_calc(hm_brox_t h, const uint8_t *frame0, const uint8_t *frame1,
                 float *flowx, float *flowy);
/* n independent pairs, pair i at offset i*width*height in each array
 * (the loop of process(), src/optical_flow_ext.cpp:361-412, turned into a batch). */
int hm_brox_calc_batch(hm_brox_t h, int n, const uint8_t *frame0, const uint8_t *frame1,
                       float *flowx, float *flowy);
/* same, all four pointers in device memory; asynchronous on the handle's stream */
int hm_brox_calc_dev(hm_brox_t h, int n, const uint8_t *d_frame0, const uint8_t *d_frame1,
                     float *d_flowx, float *d_flowy);
int hm_brox_sync(hm_brox_t h);
/* the hipStream_t of the handle (so a caller can order its own work against it) */
void *hm_brox_stream(hm_brox_t h);
/* pyramid geometry: returns the number of levels, fills widths/heights (cap entries) */
int hm_brox_levels(hm_brox_t h, int *widths, int *heights, int cap);
/* SOR relaxation factor (default 1.99) */
int hm_brox_set_omega(hm_brox_t h, float omega);
/* launch tuning, never changes results: "sor_fuse" = red-black iterations fused
 * per SOR launch (0 = choose per level, else a divisor of solver_iterations, at most 10),
 * "sor_deep" = 1/0 (default 1): with sor_fuse 0, a level whose tiles would not fill the device even with the halo of
 * all solver_iterations takes them in one launch, "coarse_max" = 0, 32 (default) or 64: pyramid levels of at most
 * that many pixels per side run in one launch per pair (k_coarse) instead of one launch per operator,
 * "cu_reserve" = n (default 0): the handle gets a second stream with a compute-unit mask that leaves n CUs to
 * other streams and uses it from now on (call it before hm_brox_stream's value is kept anywhere; the pipeline sets 32),
 * "whole_chip" = 1/0: with a cu_reserve in force, the next calls go to the unmasked stream / back to the masked one
 * (the stream that is left is drained first; the pipeline gives the first series of a phase the whole chip),
 * "coarse_stagger" = 1/0: test knob, delays some workgroups of k_coarse between phases,
 * "sor_threads" = 256, 512 or 1024 threads per SOR workgroup (0, the default: 1024 for calls of one or two pairs,
 * 512 for larger ones), "warp_window" =
 * 1/0 the warp kernel stages its taps as an LDS window or reads them directly (default 0: measured
 * faster, see brox_kernels.h).  (Round 1 also had "graph": replaying a call's launch series as a captured
 * hipGraph.  Replays went wrong when the caller allocated device memory between calls, the cause was not
 * found, and with the series queued from a helper thread it bought nothing: removed.) */
int hm_brox_tune(hm_brox_t h, const char *key, int value);

/* HIP-event timing of the SOR launches of subsequent calc calls.
 * read: total milliseconds, launches, pixel-iterations (sum over launches of
 * pixels * red-black iterations) and pixels (sum over launches of pixels: every launch is one pass
 * over memory) since profiling was switched on or last read (switching it off stops the recording
 * and keeps the totals for `read`).  Any output pointer may be NULL. */
int hm_brox_profile(hm_brox_t h, int enable);
int hm_brox_profile_read(hm_brox_t h, double *sor_ms, long long *sor_launches,
                         double *sor_pixel_iterations, double *sor_pixels);
/* the same four totals per pyramid level (index 0 = the full frame) since profiling was switched on (not reset
 * by hm_brox_profile_read); fills at most cap entries of each array (any may be NULL), returns the number of levels */
int hm_brox_profile_levels(hm_brox_t h, int cap, double *sor_ms, long long *sor_launches,
                           double *sor_pixel_iterations, double *sor_pixels);

/* Single operators on host arrays, for parity tests against the oracle.
 * Each allocates scratch, runs the same kernel calc uses, and copies back. */
int hm_op_blur(const float *src, int w, int h, float scale_factor, float *dst);
int hm_op_resample(const float *src, int ws, int hs, float *dst, int wd, int hd, float mul);
int hm_op_deriv(const float *src, int w, int h, float *dx, float *dy);
/* the fused launches calc is made of (each gives the bits of the separate operators above applied in
 * turn): one pyramid level = blur + resample; all derivative images of a level (out: Ix0, Iy0 of I0;
 * I1x, I1y, I1xx, I1xy, I1yy of I1); u + du, v + dv prolonged to the next finer level with the flow
 * rescaled (wd = ws and hd = hs: the level-0 form, the sums themselves) */
int hm_op_pyr_down(const float *src, int ws, int hs, float scale_factor, float *dst, int wd, int hd);
int hm_op_deriv_all(const float *I0, const float *I1, int w, int h, float *const out[7]);
int hm_op_add_prolong(const float *u, const float *v, const float *du, const float *dv, int ws, int hs,
                      float *u2, float *v2, int wd, int hd);
/* in: I0,Ix0,Iy0,I1,I1x,I1y,I1xx,I1xy,I1yy,u,v   out: Iz,Ix,Iy,Ixz,Iyz,Ixx,Ixy,Iyy;
 * window: 1 = the LDS-window variant of the kernel (hm_brox_tune "warp_window"), 0 = direct reads */
int hm_op_warp(const float *const in[11], int w, int h, float *const out[8], int window);
/* in: u,v,du,dv + the 8 warped fields   out: nu,nv,a12,idu,idv,sx,sy */
int hm_op_prepare(const float *const in[12], int w, int h, float alpha, float gamma,
                  float *const out[7]);
/* du,dv updated in place; coef = nu,nv,a12,idu,idv,sx,sy; fuse = sor_fuse (+100 selects
 * 512-thread, +200 1024-thread workgroups) */
int hm_op_sor(float *du, float *dv, const float *const coef[7], int w, int h,
              int iterations, int fuse, float omega);

/* ------------------------------------------------------------------------
 * EKF measurement model.  Replaces Renderer (renderer.py:197-737, the OpenGL
 * rasteriser) and CUDAGL / CUDAGL_multi (cuda.py, cuda_multi.py: the reduction
 * kernels and their PBO plumbing).
 * ---------------------------------------------------------------------- */
typedef struct hm_ctx *hm_ctx_t;

/* Renderer.__init__ + loadMesh (renderer.py:199-295, 560-654) and the
 * CUDAGL_multi constructor (cuda_multi.py:24-71): mesh topology, texture
 * coordinates (= initial vertex positions in pixels, renderer.py:579) and the
 * measurement-noise scales that the reference bakes into its kernels
 * (cuda_multi.py:420).  tri: T*3 int32 vertex ids; uv: N*2 float pixels.
 * Refused (HM_ERR_ARG, the message names the limit): a frame outside
 * 1..4096 px either way, more than 4096 triangles (EKF_MAX_TRI), a vertex in
 * more than 24 triangles (EKF_MAX_STAR) or with more than 25 neighbours
 * (PREP_MAX_ENTRIES = 104 terms of a row of k_solve_prep).  A star region of
 * more than 1024 tiles of 8x8 px (TMASK_STRIDE) is measured without a tile
 * list: same numbers, more tiles walked. */
int hm_ctx_create(int device, int width, int height, int n_vertices, int n_triangles,
                  const int32_t *tri, const float *uv,
                  double eps_Z, double eps_J, double eps_M, hm_ctx_t *out);
int hm_ctx_destroy(hm_ctx_t h);
/* gloo.Texture2D(im1) bound as init_texture (renderer.py:222-223,232): W*H u8 */
int hm_set_texture(hm_ctx_t h, const uint8_t *tex);
/* the observed frame of compute()/initjacobian (kalman.py:676-700,
 * renderer.py:674-679): y_im u8, y_flow x/y f32, y_m u8 in {0,1} */
int hm_set_observation(hm_ctx_t h, const uint8_t *y_im, const float *y_fx,
                       const float *y_fy, const uint8_t *y_m);
/* device-resident variant (flow straight from hm_brox_calc_dev) */
int hm_set_observation_dev(hm_ctx_t h, const uint8_t *d_y_im, const float *d_y_fx,
                           const float *d_y_fy, const uint8_t *d_y_m);

/* Renderer.render() of state X (renderer.py:310-325 after update_vertex_buffer
 * :503-524).  X = 4N doubles [x0,y0,..,vx0,vy0,..] (kalman.py:178).  Any output
 * pointer may be NULL.  im u8, fx/fy f32, m u8 (255 where covered), all W*H. */
int hm_render(hm_ctx_t h, const double *X, uint8_t *im, float *fx, float *fy, uint8_t *m);

/* In the calls below `masked` selects which observed flow the residuals use:
 * 0 = the flow as given to hm_set_observation, 1 = that flow multiplied by y_m
 * (what compute() hands to update(), kalman.py:679-687; error() gets the raw
 * flow, :700). */

/* initjacobian (cuda.py:940-950): render X and keep it as the reference render */
int hm_initjacobian(hm_ctx_t h, const double *X, int masked);
/* jz (cuda.py:972-980): render Xp, return the sum and its 4 components
 * (image, flow x, flow y, mask) against the reference render */
int hm_jz(hm_ctx_t h, const double *Xp, int masked, double *jz, double jzc[4]);
/* j (cuda.py:982-1010): renders X + dX e_i and X + dX e_j and reduces the products
 * of their differences to the reference render */
int hm_j(hm_ctx_t h, const double *X, double deltaX, int i, int j, double *out);
/* The reference's multi-perturbation operators: several non-interacting perturbations in one render, the
 * sums separated by the label of the triangle a pixel belongs to.  labels: one per triangle (the palette
 * update_vertex_buffer selects, renderer.py:553-556, built at :610-614; -1 = none); a pixel takes the label
 * shown by the reference render where that covers it, else by the perturbed render(s) in turn
 * (cuda_multi.py:132-143, 215-235).  hm_initjacobian must have been called.
 *   jz_multi (cuda_multi.py:81-157, 721-845): Xp = the state with all its perturbations applied;
 *       hz[n_labels], hzc[n_labels x 4] (may be NULL): the sums of hm_jz per label;
 *   j_multi (cuda_multi.py:159-248, 979-1129): ee = n_pairs x 2 state indices; one render of X with every
 *       ee[k][0] raised by deltaX, one with every ee[k][1]; hsum, nz (pixels counted), hcomp[n_labels x 4]
 *       (may be NULL) per label.
 * The fused hm_measure does not need them (it evaluates every single perturbation inside its own star);
 * they are here so that KFState._jacobian_multi / _hessian_sparse_multi (kalman.py:452-489, 539-581) run
 * as in the reference. */
int hm_jz_multi(hm_ctx_t h, const double *Xp, int masked, const int32_t *labels, int n_labels,
                double *hz, double *hzc);
int hm_j_multi(hm_ctx_t h, const double *X, double deltaX, int n_pairs, const int32_t *ee,
               const int32_t *labels, int n_labels, double *hsum, double *nz, double *hcomp);
/* KalmanFilter.projectmask (kalman.py:724-742) on the device: every vertex whose signed distance fd to the object's
 * outline exceeds 1 px takes 10 steps p -= d g/|g|^2 (g: forward differences of 0.1 px; d and the set of vertices
 * are those before the first step) and its displacement is added to its velocity.  fd is the reference's
 * (findObjectThreshold(y_m, 0.5)[2], imgproc.py:175-248): the mask's contours pruned as there (:205-228: the largest
 * object and its holes of cv2.contourArea >= 40; areas from pixel counts by Pick's theorem), then the distance to the
 * polygon through the centres of the border pixels of what is left (-cv2.pointPolygonTest), negative inside.
 * y_m: W*H host mask (object where > 0), or NULL = the mask of the observation in place.  X (4N) is updated in
 * place; *moved (may be NULL) = number of vertices that were outside. */
int hm_project_mask(hm_ctx_t h, const uint8_t *y_m, double *X, int *moved);
/* the pruning step alone, for parity tests: out (W*H) = 1 where the pruned object is */
int hm_prune_mask(hm_ctx_t h, const uint8_t *y_m, uint8_t *out);
/* Renderer.error (renderer.py:485-501): SSE per channel of render(X) against the
 * observation, with the 8-bit wrap-around the reference's uint8 arithmetic has
 * for the image and mask terms.  err = e_im, e_fx, e_fy, e_m; fx/fy (may be NULL)
 * receive the rendered flow planes */
int hm_error(hm_ctx_t h, const double *X, int masked, double err[4], float *fx, float *fy);

/* KFState.update (kalman.py:437-449) in one call, single-perturbation
 * semantics (_jacobian :491-518, _hessian_sparse :583-606; deltaX = 2 there):
 * renders X once, then evaluates every +-deltaX perturbation only inside the
 * bounding box of the triangles it moves, one workgroup per vertex / per mesh
 * edge.  Hz[4N], Hzc[4N*4] (may be NULL), HTH[4N*4N] (dense, symmetric, zero
 * outside the J pattern kalman.py:202-205; _hessian :521-536 has the same
 * value because non-adjacent vertices have disjoint supports). */
int hm_measure(hm_ctx_t h, const double *X, double deltaX, int masked,
               double *Hz, double *Hzc, double *HTH);
/* The dense part of the update (kalman.py:753-755, 785-799) on the device, in information form:
 *   begin : factor the prior covariance W (4N x 4N, symmetric positive definite) and keep
 *           inv(W) and the prior mean X0 on the device;
 *   step  : hm_measure at X, then  step = (inv(W) + HTH)^-1 (Hz - HTH (X0 - X))  by a blocked
 *           Cholesky factorisation (the reference forms inv(inv(W) + HTH) explicitly and
 *           multiplies); the new iterate is X0 + step.  Hzc (4N x 4, may be NULL) as hm_measure;
 *           err (may be NULL) receives hm_error of the new iterate X0 + step (kalman.py:813);
 *   cov   : (inv(W) + HTH)^-1 of the last step (which = 0) or of the one before (which = 1,
 *           what the reference keeps as W_old for its mesh-inversion rollback, kalman.py:806-811);
 *           which = -1: the prior itself (no iterate was accepted).
 * A non-positive-definite system shows up as NaNs in `step`. */
int hm_update_begin(hm_ctx_t h, const double *W_prior, const double *X0);   /* W_prior NULL: the covariance
                                                                              resident on the device */
/* queue the covariance half of the next hm_update_begin / hm_update_run(h, NULL, ...) -- factoring and
 * inverting the covariance resident on the device -- and return; it does not need the predicted state,
 * so it can run while the host predicts the state (hm_ms_newton) */
int hm_update_prefactor(hm_ctx_t h);
int hm_update_step(hm_ctx_t h, const double *X, double deltaX, int masked, double *step, double *Hzc,
                   double err[4]);
int hm_update_cov(hm_ctx_t h, int which, double *W_out);                     /* W_out NULL: stays on the device */
/* The whole of IteratedKalmanFilter.update (kalman.py:774-831) in one call: begin, up to max_iter
 * steps with the reference's acceptance logic between them, cov of the state that is kept.
 *   X       in: the predicted state (prior mean); out: the state kept;
 *   info    iterations run, iterations accepted, reverted (a triangle flipped, :806-811), converged
 *           (|e_new - e_old| / e_new < reltol, :817-819);
 *   errs    max_iter x 4 (may be NULL): hm_error of every new iterate, one row per iteration run.  The row of an
 *           iteration whose iterate flipped a triangle is written as well -- the sums of the flipped iterate's render,
 *           which the reference never forms (it leaves the loop at :811, before error() at :813): only the first
 *           info[1] rows are the reference's; rows from info[0] on are not written;
 *   Hzc     4N x 4 (may be NULL) of the last measurement; gains 3 x 4N (may be NULL): W Hzc[:,0],
 *           W (Hzc[:,1] + Hzc[:,2]), W Hzc[:,3] with the covariance kept (:828-830);
 *   W_out   4N x 4N, or NULL to leave the covariance on the device (hm_cov_fetch / hm_cov_predict).
 * Between iterations the state stays on the device and the render that gave an iterate's error is
 * the reference render of the next measurement; the numbers are those of the step-by-step calls.
 * HM_ERR_NUMERIC: the system inv(W) + HTH was not positive definite. */
int hm_update_run(hm_ctx_t h, const double *W_prior, double *X, double deltaX, int masked, int max_iter,
                  double reltol, int info[4], double *errs, double *Hzc, double *gains, double *W_out);
/* the covariance resident on the device (result of the last hm_cov_predict, hm_update_cov or
 * hm_update_run) copied to W_out (4N x 4N) */
int hm_cov_fetch(hm_ctx_t h, double *W_out);
/* IteratedMSKalmanFilter._newton (kalman.py:923-960): the mass-spring state prediction, ceil(1/dt)
 * implicit-Euler sub-steps each solved by Newton's method.  Host code, no GPU involved.
 * bars: I*2 vertex ids (distmesh.bars), l0: rest lengths; X: 4N doubles, advanced in place. */
int hm_ms_newton(int n_vertices, int n_bars, const int32_t *bars, const double *l0, double kappa, double M,
                 double dt, int maxiter, double tol, double *X, int *newton_iterations);
/* The same, started ahead of time on a host thread: the state a frame ends with is the one the next frame's
 * prediction starts from (kalman.py:850-863 run at the top of the next compute()).  create: one persistent
 * thread; start: copies its arguments and returns (a job still running is waited for, its result dropped); finish:
 * waits, X (4N) receives the advanced state of the job started last.  One job at a time per worker. */
int hm_ms_worker_create(void **worker);
int hm_ms_worker_destroy(void *worker);
int hm_ms_newton_start(void *worker, int n_vertices, int n_bars, const int32_t *bars, const double *l0, double kappa,
                       double M, double dt, int maxiter, double tol, const double *X);
int hm_ms_newton_finish(void *worker, double *X, int *newton_iterations);
/* Jobs started on `worker` run as ONE launch on the device of the filter handle `ctx` (NULL: back to the worker's host
 * thread) when the mesh fits the kernel (k_ms_newton4, csrc/predict_kernels.h: at most 256 vertices and 12 springs per
 * vertex; four waves, a vertex per lane) -- the state goes in and out through page-locked memory, hm_ms_newton_finish
 * takes the kernel's result block when it is whole (csrc/host_block.h); larger meshes keep the host loop.  Host and device agree to rounding (sums over the vector are
 * added in another order).  The handle must outlive the worker's jobs. */
int hm_ms_worker_attach(void *worker, hm_ctx_t ctx);
/* what the attached worker calls; 1 = not for the device (mesh too large / inner solve gave up) */
int hm_newton_dev_start(hm_ctx_t h, int N, int n_bars, const int32_t *bars, const double *l0, double kappa, double M,
                        double dt, int maxiter, double tol, const double *X);
int hm_newton_dev_finish(hm_ctx_t h, double *X, int *newton_iterations);
/* one-shot: the next hm_update_run on h calls hm_ms_newton_start(worker, ..., X) with the state it ends with as soon
 * as that state is known -- before the covariance of the kept iterate is formed and fetched */
int hm_update_arm_newton(hm_ctx_t h, void *worker, int n_bars, const int32_t *bars, const double *l0, double kappa,
                         double M, double dt, int maxiter, double tol);
/* one-shot, with hm_update_arm_newton armed as well: the next hm_update_run also queues, right behind the covariance of
 * the state it keeps, the covariance half of the NEXT frame's prediction (reference kalman.py:856-863: F at that state,
 * W' = F W F^T + Weps -- hm_cov_predict with the spring blocks at that state) and the factorisation / inverse of W' the
 * next update starts with (hm_update_prefactor): both depend on the finished update only, and the device has them
 * done while the caller is still on its way back to predict().  hm_cov_fetch keeps returning the posterior;
 * hm_update_cov is not available after such a run. */
int hm_update_arm_cov(hm_ctx_t h, double eps_F);
/* Makes what hm_update_run queued ahead (hm_update_arm_cov) current, as if hm_cov_predict(h, NULL, n_bars, bars,
 * <blocks at X>, a, s, eps_F, NULL) and hm_update_prefactor(h) had just been called -- if it was made from exactly
 * these inputs (X: the 4N state before the step; compared bit for bit).  Returns 0 when taken, 1 when there is nothing
 * to take: the caller then makes the two calls itself (the posterior is still the resident covariance). */
int hm_predict_take(hm_ctx_t h, const double *X, int n_bars, const int32_t *bars, const double *l0, double kappa,
                    double a, double s, double eps_F);
/* Covariance prediction W' = F W F^T + Weps (kalman.py:717 and :863) on the device, with
 * F = [[I, a I], [s dfdy, I]], dfdy given as one symmetric 2x2 block (Bxx, Bxy, Byy) per spring
 * (kalman.py:865-902; n_bars = 0: the constant-velocity model), Weps = eps_F [[I/4, I/2], [I/2, I]]
 * (:182).  W_in NULL: propagate the covariance resident on the device.  The result is copied to
 * W_out (NULL: not copied) and kept on the device for hm_update_begin / hm_update_run(h, NULL, ...). */
int hm_cov_predict(hm_ctx_t h, const double *W_in, int n_bars, const int32_t *bars, const double *blocks,
                   double a, double s, double eps_F, double *W_out);
/* IteratedMSKalmanFilter.predict (kalman.py:850-863) in one call for the covariance resident on the device:
 * the spring Jacobian at X before the step gives F (:856, 904-912); X (4N, in place) is advanced by _newton
 * (:923-960) -- on the device, one workgroup on a second stream, for meshes whose problem fits its LDS (about 350
 * vertices), else by hm_ms_newton; W <- F W F^T + Weps (hm_cov_predict); prefactor != 0: also what
 * hm_update_prefactor does, queued by the calling thread while the state prediction runs. */
int hm_ms_predict(hm_ctx_t h, int n_bars, const int32_t *bars, const double *l0, double kappa, double M, double dt,
                  int maxiter, double tol, double eps_F, double *X, int *newton_iterations, int prefactor);
/* Renderer.error (renderer.py:485-501) of the state the last hm_update_run kept, against the observation as it was
 * given (raw flow), WITHOUT another render: when that state is the update's last iterate, the iterate's own render
 * produced these sums (KalmanFilter.compute ends with exactly this call, kalman.py:700).  X: the state asked about.
 * Returns 0 and fills err, or 1 when the sums are not at hand (another state, a reverted update, a new observation or
 * texture since): call hm_error then. */
int hm_update_last_error(hm_ctx_t h, const double *X, double err[4]);
/* KalmanFilter.compute's predict -> projectmask -> update (kalman.py:676-700) without a host round trip between the
 * three, for a state prediction started on the device (hm_ms_worker_attach + hm_update_arm_newton / hm_ms_newton_start)
 * and the new frame's observation in place: queues projectmask (kalman.py:724-742, mask of the resident observation) of
 * the prediction in flight behind its kernel; the projected state stays in device memory as the prior mean of the NEXT
 * hm_update_run on h, whose X argument is then output only (it must still point at 4N doubles).  Same numbers as
 * hm_ms_newton_finish + hm_project_mask(h, NULL, ...) + hm_update_run.  Returns 0 when queued, 1 when there is nothing
 * to chain (no device prediction in flight): the caller makes the three calls.  A chained hm_update_run returns 2 when
 * the prediction's inner solve gave up (never observed): the caller predicts on the host and calls it again. */
int hm_chain_project(hm_ctx_t h);
/* The contour pruning and outline of a mask in DEVICE memory queued ahead of the hm_set_observation_dev that will name it
 * as d_y_m (a streaming caller holds the next frame's mask a frame early): that call then finds the outline done instead
 * of queueing ~0.2 ms of kernels the projection waits for.  The mask must not change until then; any other observation
 * or a projection onto a host mask discards the preparation.  Only the address is compared: d_y_m = NULL discards the
 * preparation, for a caller about to put another mask at the prepared address (a reused frame slot, a new phase). */
int hm_prepare_mask(hm_ctx_t h, const uint8_t *d_y_m);
/* one-shot: the next hm_update_run on h calls hm_prepare_mask(h, d_y_m) the moment its state is final, so that the next
 * frame's outline is computed beside the state prediction and the update's tail.  That hm_update_run takes the arm out of
 * the handle whether or not it succeeds. */
int hm_update_arm_mask(hm_ctx_t h, const uint8_t *d_y_m);
/* Hz components (4N x 4) and gains (3 x 4N; kalman.py:826-828) of the last hm_update_run that was called with
 * Hzc = gains = NULL: such a call does not wait for the kernels that form them.  Either may be NULL.  Available until the
 * next hm_update_run on h; zeros for an update without iterations.  HM_ERR_STATE when the last hm_update_run on h failed
 * (or there was none): nothing of an earlier update is handed out. */
int hm_update_tail(hm_ctx_t h, double *Hzc, double *gains);
/* what the last chained hm_update_run started from: the predicted state, the projected state (its prior mean), the Newton
 * iterations of the prediction, the number of vertices projectmask moved; any pointer may be NULL */
int hm_chain_states(hm_ctx_t h, double *predicted, double *projected, int *newton_iterations, int *moved);
/* tuning knobs: "measure_split" = workgroups per vertex job of the measurement (1..16, default 5),
 * "edge_split" = workgroups per mesh-edge job (1..16, default 2); the sums change in their last
 * bits with them (another summation order); "chol_flow" = 1/0 the blocked Cholesky factorisations of the update as one
 * persistent launch whose block tasks hand their results over through memory, or one launch per 32-column block step
 * (same bits either way), "chol_flow_wgs" = workgroups of that launch (2..2048, default 256: the first becomes the chain of
 * the diagonal blocks, the others run the tasks it waits for), "chol_flow_stall" = n (test knob, default 0): that chain sleeps
 * ~4 us x n before every diagonal block, so that every wait for it takes the patient path; "result_delay" = n microseconds
 * (test knob, default 0): the kernels that hand result blocks to the host (csrc/host_block.h) publish a block's last word
 * first and the rest n us later -- same results; "tail_split" = 1/0 the tail of hm_update_run (covariance of the kept
 * state, gains, the next frame's covariance prediction) on a stream of its own or on the handle's (same results);
 * "newton_fail" = 1 (test knob): device state predictions report a failed inner solve */
int hm_ctx_tune(hm_ctx_t h, const char *key, int value);
/* the same with a value of 64 bits, for "rec_ev_bytes" (1..2^34); any other key takes what fits 32 bits, as hm_ctx_tune */
int hm_ctx_tune64(hm_ctx_t h, const char *key, int64_t value);
int hm_ctx_sync(hm_ctx_t h);
void *hm_ctx_stream(hm_ctx_t h);

/* ------------------------------------------------------------------------
 * Rauch-Tung-Striebel smoothing of a recorded track (offline; the reference has no smoother).
 * P_k, x_k: the posterior covariance and mean frame k's update kept; m_k: the prior mean that update started from,
 * after projectmask (the projection onto the mask is part of the prior the filter used, so the recursion takes m_k, not
 * the raw prediction F x_{k-1}); F_k = [[I, a I], [s dfdy(x_k), I]] with the spring blocks at x_k (hm_cov_predict),
 * Pp_{k+1} = F_k P_k F_k^T + Weps.  Backward, k = K-2 .. 0, from xs_{K-1} = x_{K-1}, Ps_{K-1} = P_{K-1}:
 *     G_k  = P_k F_k^T Pp_{k+1}^-1
 *     xs_k = x_k + G_k (xs_{k+1} - m_{k+1})
 *     Ps_k = P_k + G_k (Ps_{k+1} - Pp_{k+1}) G_k^T        (with covariances only)
 * A smoother belongs to one filter handle and is destroyed before it.
 *
 * create: a record of `capacity` (>= 2) frames -- capacity slots of 4N x 4N doubles plus 4 x 4N doubles per frame,
 *     and seven 4N x 4N work matrices -- and the model: springs bars (n_bars x 2 vertex ids), rest lengths l0, kappa,
 *     a, s, eps_F as hm_cov_predict takes them with the blocks of hm_ms_predict (a = dt, s = dt / M); n_bars = 0 with
 *     a = 1, s = 0: the constant-velocity model.  HM_ERR_ARG: capacity < 2, a NULL handle, a spring outside the mesh;
 *     HM_ERR_HIP: an allocation failed (the message names its size).
 * record: one call per frame, after that frame's update (hm_update_run, also after hm_update_arm_cov; hm_update_begin /
 *     _step / _cov; a chained run): queues on the filter's stream a device-to-device copy of the covariance the update
 *     kept (ordered behind the launches that form it and ahead of everything on the handle that overwrites it) and of
 *     the prior mean the update keeps on the device; X (4N): x_k, the state the update kept.  HM_ERR_STATE: the record
 *     is full, or no update has run on the handle -- the record is left as it was.
 * run: the backward pass over the K frames recorded, on the filter's stream.  Pp_{k+1} is recomputed by the kernels
 *     and from the inputs of the forward prediction (same bits) and factored by the update's factorisation, per step
 *     (Pp = L L^T, T = L^-1); G_k = (T F_k P_k)^T T is formed through the factor, inv(Pp) = T^T T never is;
 *     xs (K x 4N) always; want_cov != 0: var (K x 4N) = diag(Ps_k), and Ps_k replaces P_k in slot k (after such a run
 *     the record takes no more frames and cannot be run again).  want_cov = 0 needs matrix-vector products only and
 *     leaves the record as it is; its xs are bit-equal to those of a run with covariances.  HM_ERR_NUMERIC: some
 *     Pp_{k+1} is not positive definite or not finite; the message names frame k+1 (the latest such frame), xs and
 *     var hold no result.  After HM_ERR_NUMERIC with want_cov = 0 the record and the filter handle are as they were.
 *     With want_cov != 0 the record is consumed, as after a run that succeeded: its slots were being overwritten from
 *     the first step on, so record, run and prior return HM_ERR_STATE; fetch still gives x_k and m_k as recorded (and
 *     the last slot, which no step writes); the filter handle is as it was.
 * count: the frames recorded and the capacity (either pointer may be NULL).
 * fetch: slot k (4N x 4N: P_k, or Ps_k after a run with covariances), x_k and m_k (4N each); any may be NULL.
 * prior: Pp_k (k >= 1) recomputed from slot k-1 as the backward pass does; HM_ERR_STATE after a run with covariances.
 * hm_op_smooth_gemm: the backward step's products on host n x n row-major arrays on the f64 matrix cores, for tests:
 *     which 0: out = A^T B;  1: out = A (B - C) (E = G (Ps' - Pp));  2: out = C + A B^T formed for the lower triangle
 *     and mirrored (Ps = P + E G^T, exactly symmetric);  3: out = tril(A) B (Y = T (F P));  4: out = A^T tril(B)
 *     (G = Y^T T) -- tril: what lies right of the diagonal is not read.  C may be NULL except for 1 and 2. */
typedef struct hm_smooth *hm_smooth_t;
int hm_smooth_create(hm_ctx_t ctx, int capacity, int n_bars, const int32_t *bars, const double *l0, double kappa,
                     double a, double s, double eps_F, hm_smooth_t *out);
int hm_smooth_destroy(hm_smooth_t sm);
int hm_smooth_record(hm_smooth_t sm, const double *X);
int hm_smooth_run(hm_smooth_t sm, int want_cov, double *xs, double *var);
int hm_smooth_count(hm_smooth_t sm, int *frames, int *capacity);
int hm_smooth_fetch(hm_smooth_t sm, int k, double *P_out, double *x_out, double *m_out);
int hm_smooth_prior(hm_smooth_t sm, int k, double *Pp_out);
int hm_op_smooth_gemm(int device, int which, int n, const double *A, const double *B, const double *C, double *out);

/* ------------------------------------------------------------------------
 * Views of the tracker (reference renderer.py:436-475 screenshot, :595-628 draw,
 * :344-373 the wireframe; kalman.py:638-674 plotforces).  Every view is H x W x 3
 * uint8, B, G, R, rows top to bottom, rendered at the state X (4N doubles) on the
 * handle's stream with targets of its own: a view changes nothing a later
 * measurement, update or chained prediction reads.
 *   which  0 raw      the gray render in all three channels
 *          1 overlay  R = the observed frame in place (hm_set_observation*), G = the render,
 *                     B = the wireframe
 *          2 texture  raw plus the wireframe
 *          3 mask     R = 255 inside the mesh, G = label / 256, B = label % 256 of the palette
 *                     (`palette`: one label per triangle, -1 or NULL: 255, 255), plus the wireframe
 *          4 flowx, 5 flowy  the rendered flow plane, floor(255 (p - min) / (max - min)) in f64
 *                     (0 where max == min), in all three channels.  min and max are taken over the
 *                     finite pixels of the plane: a pixel that is NaN or +-inf (a diverged state: a
 *                     velocity beyond binary32) takes no part in them and shows 0; with no finite
 *                     pixel, or max == min (-0 equals +0), every pixel shows 0
 * The wireframe: the three edges of every triangle (interior edges twice), end points rint(vertex),
 * pixel i = 0..n, n = max(|dx|, |dy|): x0 + floor((2 i dx + n) / (2 n)); B = min(255, B + 128 count).
 * A triangle whose vertices round to one pixel counts three there.  Segments are clipped to the frame
 * pixel by pixel; one with an end point that is NaN, infinite or, after rounding, beyond +-2^20 px
 * (exactly 2^20 is drawn) is left out whole.  Where triangles overlap, G and B of the mask view are the
 * sums of their colours, each saturated at 255, as the mask render has them.
 * hm_view_dev writes into device memory d_bgr (W*H*3 bytes for any W*H, 4-byte aligned: HM_ERR_ARG
 * otherwise) and does not wait; `stream` (may be NULL) waits for the view on the device, so a copy
 * queued there reads it whole.  The observed frame is read when the view runs: keep it in place until
 * then.
 * hm_view_forces: the overlay with every channel halved, then the arrows of plotforces in four layers,
 * each over the one before: orig -> pred white, pred -> pred + 10 tv (255, 0, 0), + 10 fv (0, 255, 0),
 * + 10 mv (0, 0, 255) (B, G, R); orig, pred, tv, fv, mv: the 2N vertex coordinates.  End points are
 * truncated as C int() does; the head is two segments from the tip at +-45 degrees, 0.1 of the shaft:
 * tip + rint(K (dx - dy), K (dy + dx)) and tip + rint(K (dx + dy), K (dy - dx)), (dx, dy) = start - tip,
 * K = 0.1 sqrt(1/2).  An arrow with an end point (before truncation) that is NaN, infinite or beyond
 * +-2^20 is left out, heads included; one of length 0 is the pixel of its start; what falls off the
 * frame is clipped.  Not the reference's: no 2x upscale, thickness 1, no legend text. */
int hm_view(hm_ctx_t h, const double *X, int which, const int32_t *palette, uint8_t *bgr);
int hm_view_dev(hm_ctx_t h, const double *X, int which, const int32_t *palette, void *d_bgr, void *stream);
int hm_view_forces(hm_ctx_t h, const double *X, const double *orig, const double *pred, const double *tv,
                   const double *fv, const double *mv, uint8_t *bgr);

/* The cell view: what is known about the body -- ROIs, demixed shapes, their activity -- painted onto a frame of
 * the video at state X, on the animal as it moves (the reference paints its neurons onto every frame,
 * synth.py:268-279).  H x W x 3 uint8, B, G, R, rows top to bottom, like every view; it has buffers of its own
 * and changes nothing a measurement, update or prediction reads.  Per image pixel (row r, column c), in this order:
 *   base      B = G = R = frame[r, c], the gray frame passed (not the handle's observation).
 *   triangle  the lowest-indexed triangle that covers the pixel centre at X (the first 2N doubles of X, the
 *             positions), by the render's rule as hm_body_map applies it at X = uv: positions snapped to
 *             1/256 px, exact edge functions, top-left ties, orientation swap.  A triangle of area 0, or with a
 *             vertex that is not finite or beyond +-2^24 px, is skipped; without a covering triangle the pixel
 *             keeps the base.  l1 = e1 / area, l2 = e2 / area in binary64, vertex order i0, i1, i2 after the swap at X.
 *   body pixel  bx = (Ux[i0] + l1 (Ux[i1] - Ux[i0])) + l2 (Ux[i2] - Ux[i0]), the same for by, in binary64 without
 *             contraction, U the binary32 uv widened; the body pixel is column floor(bx), row floor(by); no
 *             cell where either is not finite or off the frame.
 *   layers    for j = 0 .. n_layers - 1 in order, s = labels[j][body pixel]; if s >= 0:
 *             a = weights[j][body pixel] levels[s] (uint16 times uint8), D = 65535 * 255, and every channel becomes
 *             (ch (D - a) + colour[s][ch] a + D / 2) / D in unsigned 64-bit integers.
 *   outline   (flags bit 0) a body pixel with layer-0 label s >= 0 is an outline pixel when one of its four
 *             neighbours has a different layer-0 label, a neighbour off the frame counting as different; an image
 *             pixel that lands on one takes colour[s] outright (a silent cell stays visible).
 *   wire      (flags bit 1) B = min(255, B + 128 count), the wireframe of hm_view.
 *   markers   last: P points, image coordinates (x, y) as doubles (what following a body point through the mesh
 *             gives), centre ((int)x, (int)y) truncated as C does, the filled disc dx^2 + dy^2 <= point_radius^2
 *             in integers in the point's own B G R colour; a later point wins over an earlier one; a point that
 *             is not finite or beyond +-2^20 px is skipped; pixels off the frame are not written.
 * hm_view_set_cells: labels: n_layers (1..4) planes of W*H int32 in body coordinates, -1 none, labels 0 .. L-1;
 * weights: the same planes as uint16, NULL: 65535 everywhere; colours: L x 3, B G R.  labels NULL clears the
 * cells.  A label >= L or an n_layers outside 1..4 is HM_ERR_ARG (hm_last_error has the numbers).  The cells stay
 * until they are set again or cleared.
 * hm_view_cells: host arrays; frame W*H gray; levels: L bytes, NULL: 255 everywhere; P = 0 or points NULL: no
 * markers; point_colours P x 3; bgr W*H*3.  Without cells and without points there is nothing to draw:
 * HM_ERR_STATE.  A negative point_radius is HM_ERR_ARG.
 * hm_view_cells_dev: d_frame and d_bgr (4-byte aligned) are device memory; queued on the handle's stream, it does
 * not wait: X, levels, points and their colours are copied before it returns (the caller may overwrite them at
 * once), the frame is read when the view runs; `stream` (may be NULL) waits for the view on the device, as in
 * hm_view_dev. */
int hm_view_set_cells(hm_ctx_t h, int n_layers, const int32_t *labels, const uint16_t *weights, int L, const uint8_t *colours);
int hm_view_cells(hm_ctx_t h, const double *X, const uint8_t *frame, const uint8_t *levels, int flags,
                  int P, const double *points, const uint8_t *point_colours, int point_radius, uint8_t *bgr);
int hm_view_cells_dev(hm_ctx_t h, const double *X, const void *d_frame, const uint8_t *levels, int flags,
                      int P, const double *points, const uint8_t *point_colours, int point_radius, void *d_bgr, void *stream);

/* The body-frame readout: frames pulled back through the tracked mesh into the coordinates of its texture
 * (the frame-0 pixel grid of the initial vertices uv), the neuron-tracking layer the reference leaves
 * unbuilt (test_neurontracking.py:15; its synthetic neurons move with the animal, synth.py:219-266).
 *   body map  every pixel (r, c) takes the lowest-indexed triangle that covers its centre at X = uv, by
 *             the render's rule (snapped positions, exact edge functions, top-left ties, orientation
 *             swap), or -1, and l1 = e1 / area, l2 = e2 / area (binary64, correctly rounded, the
 *             swapped vertex order i0, i1, i2).  Built once per handle, on first use.
 *   warp      x = (X[i0] + l1 (X[i1] - X[i0])) + l2 (X[i2] - X[i0]) in binary64, the same for y; the
 *             frame sampled bilinearly at (x - 0.5, y - 0.5), texels clamped to the frame, rint half to
 *             even; 0 outside the map and where x or y is not finite or beyond +-2^20 px.
 *   sums      uint64 sums of the registered values per triangle (T) and per label (L) of the label
 *             image, overwritten on every call; labels count only on pixels of the map.
 * hm_body_map: the triangle per pixel (W*H, may be NULL) and the pixels per triangle (T, may be NULL).
 * hm_body_set_labels: a W*H label image in body coordinates, -1 = none, labels 0..L-1 (NULL clears);
 * counts (L, may be NULL): the map pixels per label.
 * hm_body_warp: host arrays; frame W*H gray, out W*H (may be NULL), sums may be NULL; tri_sums holds T
 * values, label_sums the L of the last hm_body_set_labels (the caller keeps that count: there is no length here).
 * hm_body_warp_dev: device arrays queued on the handle's stream; out_channels 1 or 3 (B = G = R, the AVI's
 * layout), d_out 4-byte aligned or NULL, the sums 8-byte aligned (sizes as for hm_body_warp); `stream` (may be
 * NULL) waits for the warp on the device.
 * hm_body_fence: `stream` waits on the device for the last warp queued (before it overwrites its frame). */
int hm_body_map(hm_ctx_t h, int32_t *tri_of_pixel, uint32_t *tri_counts);
int hm_body_set_labels(hm_ctx_t h, const int32_t *labels, int L, uint32_t *counts);
int hm_body_warp(hm_ctx_t h, const double *X, const uint8_t *frame, uint8_t *out, uint64_t *tri_sums, uint64_t *label_sums);
int hm_body_warp_dev(hm_ctx_t h, const double *X, const void *d_frame, void *d_out, int out_channels,
                     void *d_tri_sums, void *d_label_sums, void *stream);
int hm_body_fence(hm_ctx_t h, void *stream);

/* The deformation readout: how the tracked mesh stretches the body, which is what the tracker estimates and the
 * reference never reports (it has the force arrows of plotforces alone).  The map body -> frame is affine on every
 * triangle; per frame k and triangle t, in binary64, every step one correctly rounded operation in the order written,
 * nothing contracted, + - * / sqrt fabs only (no hypot, atan2, log: angles are the caller's, on the host):
 *   vertices  i0, i1, i2 of the body map (hm_body_map: the triangle's order after the orientation swap at X = uv);
 *             U the binary32 uv widened; x the positions of frame k, x of vertex i at X[2 i], y at X[2 i + 1].
 *   p = U1 - U0, q = U2 - U0, a = x1 - x0, b = x2 - x0;  d0 = p.x q.y - p.y q.x
 *   F11 = (a.x q.y - b.x p.y) / d0    F12 = (b.x p.x - a.x q.x) / d0
 *   F21 = (a.y q.y - b.y p.y) / d0    F22 = (b.y p.x - a.y q.x) / d0        the deformation gradient
 *   J   = (a.x b.y - a.y b.x) / d0                                          the area ratio (< 0: the triangle is flipped)
 *   c11 = F11 F11 + F21 F21,  c12 = F11 F12 + F21 F22,  c22 = F12 F12 + F22 F22
 *   m = (c11 + c22) / 2,  d = (c11 - c22) / 2,  r = sqrt(d d + c12 c12)
 *   l1 = sqrt(m + r)  the larger principal stretch;  l2 = |J| / l1 the smaller (0 where l1 == 0)
 *   c2 = d / r, s2 = c12 / r  (1, 0 where r == 0): cosine and sine of TWICE the angle of the l1 axis in the body frame
 *   tr = F11 + F22, sk = F21 - F12, s = sqrt(tr tr + sk sk);  rc = tr / s, rs = sk / s  (1, 0 where s == 0): cosine
 *             and sine of the rotation of F's polar factor
 * Seven doubles per (frame, triangle): J, l1, l2, c2, s2, rc, rs.  Where d0 == 0 or one of the six position
 * coordinates is not finite all seven are NaN.
 * hm_strain_tri: X n_frames rows of 4N doubles (the states as recorded; the 2N positions of a row are read), out
 * n_frames x T x 7; one launch for all the frames.
 * hm_strain_labels: the mean of J, l1, l2 over the body-map pixels of every label -- the local deformation under a
 * cell.  labels: a W*H image in body coordinates as hm_body_set_labels takes it (-1 none, 0 .. L-1), or NULL: the
 * image of the last hm_body_set_labels, whose L must be passed (none set: HM_ERR_STATE).  cnt[s, t] = the map pixels
 * of label s in triangle t, n_s their sum over t:
 *   out[k, s, j] = (sum of (double)cnt[s, t] * v[k, t, j] over the t with cnt[s, t] > 0 in ascending order, added one
 *                  by one to 0.0) / (double)n_s,  j = J, l1, l2;
 * no atomics, one accumulator per (k, s, j).  n_s == 0: NaN; a NaN triangle under a label makes that label NaN in that
 * frame.  out n_frames x L x 3; counts (L, may be NULL): n_s.
 * hm_view_strain: one of the three painted onto a frame of the video at state X; H x W x 3 uint8, B, G, R, like every
 * view, with buffers of its own: it changes nothing a measurement, update or prediction reads.  Per image pixel:
 *   base      B = G = R = frame[r, c], the gray frame passed.
 *   triangle  the lowest-indexed triangle that covers the pixel centre at X, by the rule of hm_view_cells word for
 *             word (positions snapped to 1/256 px, exact edge functions, top-left ties, orientation swap; a triangle
 *             of area 0 or with a vertex not finite or beyond +-2^24 px is skipped); none: the pixel keeps the base.
 *   level     of that triangle, in binary64: 128 + rint(gain (value - 1)), rint half to even, clamped to 0 .. 255;
 *             value = J, l1 or l2 of the triangle at X as above for which = 0, 1, 2.  A level that is NaN (a NaN
 *             value) keeps the base -- also where a later triangle covers the pixel as well.
 *   colour    every channel becomes (ch (255 - alpha) + lut[level][ch] alpha + 127) / 255 in integers; lut 256 x 3
 *             bytes, B G R.
 *   wire      (flags bit 1, i.e. flags = 2) B = min(255, B + 128 count), the wireframe of hm_view.
 * n_frames <= 0, which outside 0..2, alpha outside 0..255, a NULL lut, flags other than 0 or 2, a label >= L are
 * HM_ERR_ARG (hm_last_error has the numbers); a failed allocation or launch is HM_ERR_HIP.
 * hm_view_strain_dev: d_frame and d_bgr (4-byte aligned) are device memory; queued on the handle's stream, it does not
 * wait (but for the body map, built by the first call that needs it): X and the lut are copied before it returns, the
 * frame is read when the view runs; `stream` (may be NULL) waits for the view on the device, as in hm_view_dev.
 * All buffers belong to the handle and are freed with it. */
int hm_strain_tri(hm_ctx_t h, int n_frames, const double *X, double *out);
int hm_strain_labels(hm_ctx_t h, int n_frames, const double *X, const int32_t *labels, int L, double *out, uint32_t *counts);
int hm_view_strain(hm_ctx_t h, const double *X, const uint8_t *frame, int which, double gain, int alpha,
                   const uint8_t *lut, int flags, uint8_t *bgr);
int hm_view_strain_dev(hm_ctx_t h, const double *X, const void *d_frame, int which, double gain, int alpha,
                       const uint8_t *lut, int flags, void *d_bgr, void *stream);

/* Statistics of the registered video, for finding cells in the body frame.  Between begin and end every
 * hm_body_warp and hm_body_warp_dev adds its registered frame (also one called without an output), right
 * behind the warp on the handle's stream.  Per pixel p of the map, v_k the registered value of frame k:
 *   s1 = sum v_k(p), s2 = sum v_k(p)^2, vmax = max v_k(p),
 *   cross[d] = sum v_k(p) v_k(p + d), d = 0..3 the neighbours right, down-right, down, down-left, where
 *              p + d is on the frame and in the map, else 0;
 * zeros outside the map.  Exact integers: at most 65536 frames per accumulation (65536 * 255^2 < 2^32);
 * the warp that would add one more fails with HM_ERR_STATE and adds nothing.
 * Images (binary64, F frames, every step one correctly rounded operation in this order):
 *   var = F s2 - s1 s1;  mean = s1 / F;  std = sqrt(var) / F;  max = vmax;
 *   rho(p, q) = (F cross(p, q) - s1(p) s1(q)) / sqrt(var(p) var(q)) over the eight neighbours q on the frame
 *   and in the map with var(p) > 0 and var(q) > 0;  corr = their sum in the order E, SE, S, SW, W, NW, N,
 *   NE divided by their number, 0 when there is none.  NaN (max: 0) outside the map.
 * Peaks of a score image (which: 0 corr, 1 std, 2 max - mean): the map pixels p with score(p) >= min_score
 * and no map pixel q != p within the (2 radius + 1)^2 window around p that has a greater score, or an equal
 * score and a lower raster index; 1 <= radius <= 16.  Sorted by score descending, raster index (row * W +
 * column) ascending; the first `cap` are written, *count is the number found.
 * begin allocates and zeroes (called again: starts over); end stops and frees (harmless when not begun);
 * fetch (cross: 4 planes of W*H), images and peaks wait for the warps queued so far and take NULL for what
 * is not wanted; HM_ERR_STATE before begin, images and peaks also while no frame has been added. */
int hm_body_stats_begin(hm_ctx_t h);
int hm_body_stats_end(hm_ctx_t h);
int hm_body_stats_count(hm_ctx_t h, int *frames);
int hm_body_stats_fetch(hm_ctx_t h, uint32_t *s1, uint32_t *s2, uint32_t *cross, uint8_t *vmax);
int hm_body_stats_images(hm_ctx_t h, double *mean, double *std, double *corr, uint8_t *vmax);
int hm_body_stats_peaks(hm_ctx_t h, int which, int radius, double min_score, int cap, int32_t *index,
                        double *score, int *count);

/* The registered video kept on the device, and exact integer reductions over it: what footprints, ROIs and
 * neuropil-corrected traces are built from (hydra_mi/roi.py).  Between begin and end every
 * hm_body_warp and hm_body_warp_dev appends its registered frame (also one called without an output), right
 * behind the warp on the handle's stream as the statistics are; statistics and record may be on together.
 * The record holds the bounding box of the body map, one byte per pixel (rows padded to 4 bytes), in chunks
 * allocated as it grows.  max_bytes is its budget: the warp that would pass it fails with HM_ERR_STATE, names
 * the numbers and appends nothing (nor adds to the statistics).  begin called again starts over; end stops
 * and frees (harmless when not begun); count gives the frames appended since begin.
 * The box may touch the frame's border on any side (the padding of a row then lies beyond the row, on the last row
 * beyond the plane: no call reads or writes a plane there).  A body map without a pixel (no pixel centre is covered by the
 * mesh at X = uv) is not an error: the box is the one pixel (0, 0), registered as 0, frames of 16 bytes.  Every call then
 * works as on any record and gives what the rules below give over no pixel: warps and fetches of zeros, sums, products,
 * counts and Gram matrices of zeros, n_core = 0 in the one patch of every grid, shifts, warps and gains that change
 * nothing (clipped = 0), statistics images NaN throughout and no peak, trace_null's tmax and tmin NaN; a call that takes
 * seeds refuses every seed, as it refuses any seed that is no pixel of the map.
 * fetch: frames k0 .. k0 + n - 1 as full W*H planes (0 outside the box), equal to what the warps returned.
 * The reductions run over all F recorded frames, wait for the warps queued so far and for their results, and
 * fail with HM_ERR_STATE before begin and while no frame is recorded.  v_k(p) is the registered value of
 * pixel p in frame k; only pixels of the map count (the others are registered as 0).
 *   label_sums     a W*H label image given now (-1: none, labels 0..L-1) -> out[k * L + l], the sums of
 *                  hm_body_warp's label_sums for every frame, without a second pass over the video.
 *   seed_sums      P seeds, (column, row) pairs of map pixels.  Per seed s and frame k, d2 the whole number
 *                  dx^2 + dy^2 from the seed, compared in binary64 with r * r:
 *                    T_k = sum v_k over the disc d2 <= r_disc^2 (n_T map pixels),
 *                    G_k = sum v_k over the ring r_in^2 <= d2 <= r_out^2 (n_G map pixels; 0 and G = 0 when empty),
 *                    U_k = n_G T_k - n_T G_k (int64): the disc trace minus the ring trace, as a whole number;
 *                  per pixel p of the (2R + 1)^2 window round the seed, R <= 16, index (dy + R)(2R + 1) + dx + R:
 *                    w1 = sum v_k(p), w2 = sum v_k(p)^2, c = sum v_k(p) U_k (0 off the frame, outside the map);
 *                  per seed u1 = sum U_k, u2 = sum U_k^2.  T, G, U hold F*P values (frame-major), w1, w2, c
 *                  P (2R + 1)^2, the others P; any output may be NULL.  Discs and rings of different seeds may
 *                  overlap; radii at most 32.  HM_ERR_ARG with the numbers when F (255 n_T n_G)^2 could pass 2^63
 *                  (every sum is exact in 64 bits below that), and for a seed that is no pixel of the map.
 *   weighted_sums  P windows of (2R + 1)^2 uint16 weights round the seeds, R <= 32 -> out[k * P + s] =
 *                  sum a_s(p) v_k(p): traces of ROIs that overlap or carry weights.
 *   trace_products P seeds and one int32 trace per seed, q[k * P + s] (any values, negative ones too), R <= 16 ->
 *                  out[s (2R + 1)^2 + p] = sum_k v_k(p) q[k * P + s] (int64; 0 off the frame, outside the map): the
 *                  product of every window pixel with a trace the host supplies, what the shape step of demixing
 *                  repeats every iteration (hydra_mi/demix.py).  Exact while
 *                  F x 255 x 2^31 < 2^63, HM_ERR_ARG with the numbers beyond that and for a seed that is no pixel
 *                  of the map.  The frames are split over the grid in runs of hm_ctx_tune "rec_tp_frames" (1..1024,
 *                  default 32) and the partial sums meet in 64-bit integer atomics: the same result in any order.
 *   trace_maps     L whole-number traces over all F recorded frames, q[k * L + s] (frame-major as in trace_products),
 *                  |q| <= 32767 and L is 1..1024 -> every trace against every pixel of the record (hydra_mi/network.py,
 *                  DESIGN.md section 17):
 *                    c[s * W*H + p] = sum_k v_k(p) q[k * L + s] (int64),
 *                    w1[p] = sum_k v_k(p),  w2[p] = sum_k v_k(p)^2 (uint64);
 *                  full W*H planes as fetch gives them: 0 outside the box and outside the map.  Any output may be NULL.
 *                  HM_ERR_ARG with the numbers for L out of range, for a |q| > 32767 (the first offender's frame and
 *                  trace are named) and when F x F x 255 x 32767 >= 2^63: below that every sum and the host's
 *                  F c - w1 u1 (u1 = sum_k q) are exact in 64 bits.  The traces are taken in groups of 8 and the frames
 *                  are split over the grid in runs of hm_ctx_tune "rec_map_frames" (1..256, default 64); the partial
 *                  sums of a run are 32-bit and meet in 64-bit integer atomics: the same result in any order and for
 *                  every value of the key.
 *   trace_null     a trace and its surrogates against every pixel, reduced to what a significance test needs
 *                  (hydra_mi/network.py map_null).  q as for trace_maps, L is 2..4096: column 0 is
 *                  the observed trace, columns 1 .. L - 1 its surrogates, however they were made.  vb[s] is the host's
 *                  F u2 - u1^2 of column s (u1 = sum_k q, u2 = sum_k q^2) rounded to binary64.  With c_s, w1, w2 as above:
 *                    num_s(p) = F c_s(p) - w1(p) u1_s,  a(p) = F w2(p) - w1(p)^2 (int64, exact under trace_maps' bound),
 *                    rho_s(p) = (double)num_s(p) / sqrt((double)a(p) * vb[s]): one conversion each, one product, one
 *                               square root, one division; 0.0 where a(p) = 0 or vb[s] = 0;
 *                    tmax[s], tmin[s] = the largest and smallest rho_s(p) over the pixels of the map (L doubles each;
 *                               NaN for a map without a pixel),
 *                    ge[p] = the number of s >= 1 with num_s(p) >= num_0(p), le[p] that with num_s(p) <= num_0(p)
 *                               (uint32, full W*H planes, 0 outside the map; whole numbers compared, a tie counts in both;
 *                               a constant pixel has L - 1 in both).
 *                  Any output may be NULL.  HM_ERR_ARG with the numbers for L out of range, for a |q| > 32767 (the first
 *                  offender's frame and trace are named), for a vb that is negative or not finite (its column is named)
 *                  and when F x F x 255 x 32767 >= 2^63.  vb is a whole number's rounding: one strictly between 0 and 1
 *                  may make a product that rounds to 0 and a rho that is not finite.  A workgroup walks all frames for
 *                  its pixels and 8 columns in runs of hm_ctx_tune "rec_null_frames" (1..256, default 256), 32-bit sums
 *                  widened in registers between runs: the same bytes for every value of the key.  The record is not
 *                  changed, and a refusal leaves it usable.
 *   gram           the Gram matrix of frames of the record (hydra_mi/pca.py; csrc/gram_kernels.h).
 *                  The call works on the frames f_i = k0 + i stride, i = 0 .. n - 1:
 *                    G[i * n + j] = sum_p v_fi(p) v_fj(p) (int64), the full symmetric n x n matrix,
 *                    s1[i] = sum_p v_fi(p) (uint64).
 *                  The sums run over the box; pixels off the map are registered as 0, so they are also the sums over the
 *                  map.  Either output may be NULL.  The record is not changed.  State errors and waiting are those of
 *                  hm_body_rec_seed_sums.  HM_ERR_ARG, with the numbers, for n < 1; for n > 8192 (REC_GRAM_MAX: G is
 *                  512 MiB there), refused on the number alone, before the frames are looked at; for stride < 1; for
 *                  k0 < 0; and for a last frame k0 + (n - 1) stride >= F.  No magnitude bound is needed: 255^2 x box bytes
 *                  is far below 2^63.  A refusal leaves the record usable.  The products are made by
 *                  v_mfma_i32_16x16x64_i8 on x = v - 128 and corrected exactly on the device; the bytes of a frame are
 *                  split over the grid in runs of hm_ctx_tune "rec_gram_bytes" (multiples of 64 in 64..131008, anything
 *                  else refused; default 16384), the sums of a run are 32-bit (128^2 x 131008 < 2^31) and meet in 64-bit
 *                  integer atomics: the same bytes in any order and for every value of the key. */
int hm_body_rec_begin(hm_ctx_t h, uint64_t max_bytes);
int hm_body_rec_end(hm_ctx_t h);
int hm_body_rec_count(hm_ctx_t h, int *frames);
int hm_body_rec_fetch(hm_ctx_t h, int k0, int n, uint8_t *out);
int hm_body_rec_label_sums(hm_ctx_t h, const int32_t *labels, int L, uint64_t *out);
int hm_body_rec_seed_sums(hm_ctx_t h, int P, const int32_t *seeds, double r_disc, double r_in, double r_out, int R,
                          uint32_t *n_T, uint32_t *n_G, uint64_t *T, uint64_t *G, int64_t *U, uint64_t *w1,
                          uint64_t *w2, int64_t *c, int64_t *u1, int64_t *u2);
int hm_body_rec_weighted_sums(hm_ctx_t h, int P, const int32_t *seeds, int R, const uint16_t *weights, uint64_t *out);
int hm_body_rec_trace_products(hm_ctx_t h, int P, const int32_t *seeds, int R, const int32_t *q, int64_t *out);
int hm_body_rec_trace_maps(hm_ctx_t h, int L, const int32_t *q, int64_t *c, uint64_t *w1, uint64_t *w2);
int hm_body_rec_trace_null(hm_ctx_t h, int L, const int32_t *q, const double *vb, double *tmax, double *tmin,
                           uint32_t *ge, uint32_t *le);
int hm_body_rec_gram(hm_ctx_t h, int k0, int n, int stride, int64_t *G, uint64_t *s1);

/* The record against the deformation of its own tissue, and the deformation's brightness taken out of it in place
 * (hydra_mi/deform.py; csrc/deform_kernels.h; tests/deform_ref.py restates both calls in NumPy).
 * Exact integers throughout.  Notation as above: F recorded frames, v_k(p) the record's byte.  t(p) = tri_of_pixel[p], the
 * body map's triangle of pixel p: the index hm_body_map returns, the same t as in hm_strain_tri, -1 off the map.  T must be
 * the handle's number of triangles: otherwise HM_ERR_ARG with both numbers.  Waiting and state errors are those of
 * hm_body_rec_seed_sums; a refusal leaves the record usable.
 *   tri_maps    every pixel against the trace of its own triangle.  q[k * T + t] are whole numbers, |q| <= 32767:
 *                 c[p]  = sum_k v_k(p) q[k * T + t(p)]  (int64),
 *                 w1[p] = sum_k v_k(p),  w2[p] = sum_k v_k(p)^2  (uint64);
 *               one full W*H plane each, 0 outside the map and the box.  Any output may be NULL.  The record is not changed.
 *               HM_ERR_ARG with the numbers for a |q| > 32767 (the first offender's frame and triangle are named) and when
 *               F x F x 255 x 32767 >= 2^63, the bound of trace_maps: below it every sum and the host's F c - w1 u1_t
 *               (u1_t = sum_k q[k * T + t]) are exact in 64 bits.  The frames are split over the grid in runs of
 *               hm_ctx_tune "rec_tm_frames" (1..256, default 64); the partial sums of a run are 32-bit and meet in 64-bit
 *               integer atomics: the same result in any order and for every value of the key.  (trace_maps with L = T
 *               traces would do T times the work and return T planes, of which a pixel needs one.)
 *   tri_gain    m[k * T + t] is uint16, 0..65535.  The record is rewritten in place: for every frame k and map pixel p
 *                 v_k(p) <- min(255, (v_k(p) m[k * T + t(p)] + 2048) >> 12)   in unsigned 32-bit integers,
 *               a gain of m / 4096: 0 to just under 16, m = 4096 the identity (the rule returns v exactly).  Pixels off the
 *               map and the padding stay 0.  *clipped (may be NULL) is the number of (frame, pixel) values whose unclamped
 *               result exceeded 255.  The rule is pointwise: the frames are rewritten where they lie, no scratch.  Every
 *               hm_body_rec_* call afterwards, fetch included, sees the rewritten frames.  NOT reversible, as
 *               hm_body_rec_shift is not (what the rounding and the clamp merge stays merged).  Nothing else on the handle
 *               changes. */
int hm_body_rec_tri_maps(hm_ctx_t h, int T, const int32_t *q, int64_t *c, uint64_t *w1, uint64_t *w2);
int hm_body_rec_tri_gain(hm_ctx_t h, int T, const uint16_t *m, uint64_t *clipped);

/* Residual motion of the kept registered video: the shift of every patch of every frame found against a template
 * and taken out of the record in place (hydra_mi/stabilize.py).  Waiting, errors and state are
 * those of hm_body_rec_seed_sums: the calls wait for the warps queued so far and for their results, fail with
 * HM_ERR_STATE before begin and while no frame is recorded, and with HM_ERR_ARG and the offending numbers in
 * hm_last_error for an argument out of range.
 * The patch grid: B is 4..64 and S is 0..8.  Patches of B x B body pixels tile the record's box (the bounding box of
 * the body map) from its top-left corner; the last column and row of patches may be narrower; patches are indexed
 * row-major.  The core of a patch is its pixels p for which every p + d, |dx| <= S and |dy| <= S, is on the frame and
 * in the map: every shift therefore sums over the same n pixels.  n may be 0; then all of that patch's sums are 0.
 *   match       `template` is W*H bytes in body coordinates.  Outputs are uint32, indexed
 *               [frame - k0][patch][(dy + S)(2S + 1) + dx + S], over frames k0 .. k0 + n_frames - 1:
 *                 A  = sum over the core of v_k(p + d) t(p),
 *                 V1 = sum over the core of v_k(p + d),
 *                 V2 = sum over the core of v_k(p + d)^2;
 *               n_core is per patch.  Any output may be NULL.  All sums are exact: 255^2 64^2 < 2^32.  The frames
 *               are split over the grid in runs of hm_ctx_tune "rec_tp_frames"; one slot per (frame, patch, shift),
 *               no atomics: the result does not depend on order.
 *   frame_sums  out[p] = sum over the frames k0 .. k0 + n_frames - 1 of v_k(p + d_k,patch(p)) as uint32, W*H values.
 *               Off the map the value is 0.  A source pixel off the box or the map counts 0.  `shifts` are int8, laid
 *               out [frame - k0][patch][2] as (dx, dy), each within +-16.  NULL means no shift, and B is then unused.
 *               Refused with HM_ERR_ARG when n_frames 255 could pass 2^32.
 *   shift       `shifts` covers all F frames.  The record is rewritten in place: v'_k(p) = v_k(p + d_k,patch(p)) where
 *               p and p + d are both in the box and in the map, else 0; the result is as if every frame were gathered
 *               from its own unshifted self (a scratch buffer of at most one chunk holds the frames as they were,
 *               freed when the call returns, with an error too).  Every hm_body_rec_* call afterwards, fetch
 *               included, sees the shifted frames.  Calling it again shifts what is there: NOT reversible (what a
 *               shift moves off the box or the map is lost).  Nothing else on the handle changes. */
int hm_body_rec_match(hm_ctx_t h, int k0, int n_frames, int B, int S, const uint8_t *tmpl, uint32_t *n_core, uint32_t *A,
                      uint32_t *V1, uint32_t *V2);
int hm_body_rec_frame_sums(hm_ctx_t h, int k0, int n_frames, int B, const int8_t *shifts, uint32_t *out);
int hm_body_rec_shift(hm_ctx_t h, int B, const int8_t *shifts);

/* The same residual motion taken out as a smooth sub-pixel shift field instead of one whole-pixel vector per patch
 * (hydra_mi/stabilize.py mode="field"; tests/stabfield_ref.py restates it).  Exact integers
 * throughout.  Waiting, state errors and argument errors are those of hm_body_rec_shift and hm_body_rec_frame_sums, with
 * the offending numbers in hm_last_error: a patch size outside 4..64, a q outside +-256 (naming component, patch and
 * frame), frames outside the record, a call before begin, a call on an empty record.
 *   Sub-pixel estimate (host arithmetic on the match sums, in stabilize.py).  Per (frame, patch) and per axis, take s0,
 *               the winning score, and s-, s+, the scores at the two neighbouring shifts along that axis.  The refinement
 *               applies only when all of these hold: the winning shift is strictly inside the search on that axis
 *               (|d| < S); both neighbours are valid; den = s- - 2 s0 + s+ < 0.  When it applies,
 *               off = (s- - s+) / (2 den), clipped to +-0.5.  Otherwise off is 0.
 *               q = 16 d + floor(16 off + 0.5) as int16, in 1/16 px.  A fallback patch has q = 0 and valid = 0.  Every
 *               step is one binary64 operation in this order.
 *   Field       Patch centres are where the patches measured.  For a box pixel at column x, per axis: u = 2x + 1 - B,
 *               i = clamp(floor(u / 2B), 0, max(npx - 2, 0)), w1 = clamp(u - 2B i, 0, 2B), w0 = 2B - w1,
 *               i1 = min(i + 1, npx - 1).  Rows are formed alike with npy.  The pixel sees the four patches
 *               (iy|iy1, ix|ix1), each with weight wy wx valid(frame, patch).  Per component, num = sum w q and
 *               den = sum w.  The shift is d(p) = floor((2 num + den) / (2 den)), floor division also for negative
 *               numbers, and 0 when den = 0.  Inside the first and last half patch the field is constant.  An invalid
 *               patch does not pull the field to zero: its neighbours fill it.  Magnitudes: w <= 4 B^2 = 16384,
 *               |q| <= 256, four terms.  int32 is enough.
 *   Sample      X = 16x + d_x(p), x0 = X >> 4 (arithmetic shift), fx = X & 15.  The y components are formed alike.
 *               v'(p) = ((16 - fx)(16 - fy) v(x0, y0) + fx (16 - fy) v(x0 + 1, y0) + (16 - fx) fy v(x0, y0 + 1)
 *                        + fx fy v(x0 + 1, y0 + 1) + 128) >> 8.
 *               A source off the box counts 0.  Off the map the record already holds 0.  v' is written only where p is in
 *               the map, and is 0 elsewhere, padding included.  With every q a multiple of 16 and every valid 1 inside
 *               one patch, the sample reduces to the whole-pixel gather.
 *   warp        `q` is int16 [frame][patch][2] as (dx, dy), each within +-256, for all F frames.  `valid` is uint8
 *               [frame][patch].  The record is rewritten in place, every frame gathered from its own unwarped self (the
 *               scratch buffer is hm_body_rec_shift's: at most 16 MiB, never more than a chunk, freed on every return
 *               including errors).  Afterwards every hm_body_rec_* call, fetch included, sees the warped frames.  NOT
 *               reversible.  Nothing else on the handle changes.  A refused warp changes nothing.
 *   field_sums  out[p] = sum over the frames k0 .. k0 + n_frames - 1 of v'_k(p) at the field of each frame as uint32, W*H
 *               values; `q` and `valid` are laid out [frame - k0][patch].  The template of pass p > 1 in field mode.
 *               Refused with HM_ERR_ARG when n_frames 255 could pass 2^32. */
int hm_body_rec_warp(hm_ctx_t h, int B, const int16_t *q, const uint8_t *valid);
int hm_body_rec_field_sums(hm_ctx_t h, int k0, int n_frames, int B, const int16_t *q, const uint8_t *valid, uint32_t *out);

/* A running baseline per pixel of the record, and the planes made from it (hydra_mi/detrend.py, DESIGN.md section 14;
 * csrc/detrend_kernels.h; tests/detrend_ref.py restates the rule in NumPy).  Exact integers throughout.
 *   Notation: F is the number of recorded frames and v_k(p) is the record's value.  half is 0..1024.  q is an integer
 *   0..100.  floor is 1..255.  gain is 1..65535.  For frame k and box pixel p:
 *   Window      frames a = max(0, k - half) .. b = min(F - 1, k + half).  It is clipped at the ends, as roi.baseline
 *               clips.  n = b - a + 1.
 *   Baseline    B_k(p) is the value at 0-based rank floor(q (n - 1) / 100) of the window's n values sorted ascending.
 *               The rank is formed in integers.  This is np.percentile(..., method="lower"), not the linear rule: it
 *               stays a uint8 and needs no rounding.
 *   Excess      E_k(p) = max(v_k(p) - B_k(p), 0).
 *   dF/F byte   D_k(p) = min(255, (gain E_k(p)) / max(B_k(p), floor)), computed by unsigned integer division.
 *   Off the map and in the padding: v = 0, so B = E = D = 0 without a look at the map.
 *   Four kinds of plane, `what`: 0 as recorded, 1 baseline, 2 excess, 3 dF/F byte.
 *   planes      writes the frames k0 .. k0 + n_frames - 1 as full W x H planes into `out`, laid out as hm_body_rec_fetch
 *               lays them out; what = 0 equals that call.  The windows reach outside [k0, k0 + n_frames) into the whole
 *               record.
 *   stats_add   adds every recorded frame's plane of that kind to the statistics of hm_body_stats_*, exactly as if it
 *               had just been warped, in frame order: the sums and the count are the same, and images / peaks / fetch
 *               work afterwards unchanged.  It needs the statistics begun (HM_ERR_STATE otherwise).  If count + F would
 *               pass the capacity it fails with HM_ERR_STATE naming the numbers and adds nothing.
 *   Both: waiting and state errors are those of hm_body_rec_seed_sums; an argument out of range is HM_ERR_ARG with the
 *   numbers in hm_last_error.  The record, the map and the tracker do not change by a bit (the registered plane of the
 *   last warp, which only the next warp reads again after rewriting it, is stats_add's work plane).  The frames are split
 *   over the grid in runs of hm_ctx_tune "rec_bl_frames" (1..2^24, default 256: same results for every value); the scratch
 *   follows hm_body_rec_shift's: at most 16 MiB (one frame at least), freed on every return including errors.  (Tests set
 *   that size with hm_ctx_tune "rec_scratch_bytes", 1..2^30, for every call that uses the scratch: same results for
 *   every value.) */
int hm_body_rec_planes(hm_ctx_t h, int k0, int n_frames, int what, int half, int q, int floor, int gain, uint8_t *out);
int hm_body_rec_stats_add(hm_ctx_t h, int what, int half, int q, int floor, int gain);

/* Events per pixel of the record: AR(1) deconvolution of every box pixel's planes of a kind (hydra_mi/events.py, DESIGN.md
 * section 19; csrc/events_kernels.h; tests/events_ref.py restates the rule in Python floats).
 *   All arithmetic is binary64, in exactly this order; the library is built with -ffp-contract=off, a lane works through
 *   its pixel sequentially, and multiplication, addition and division are correctly rounded, so the device reproduces a
 *   plain Python-float restatement bit for bit.  pos(a) below is a where a > 0 and +0 otherwise.
 *   Input       The F recorded frames.  y_k(p) is the pixel's value in the plane of kind `what` (0 raw, 1 baseline, 2 excess,
 *               3 dF/F byte) of frame k; half, q, floor, gain are exactly those of hm_body_rec_planes.  y_k(p) is an
 *               integer 0..255 converted to double.  g (0 < g < 1), lam >= 0, s_min >= 0.
 *   Powers      Formed on the host: pw[0] = 1, pw[l] = pw[l-1] g for l <= F; pw2[l] = pw[l] pw[l].  No pow anywhere.
 *   Pool stack  AR(1) OASIS for min 1/2 sum (c_k - y_k)^2 + lam sum s_k with s_k = c_k - g c_{k-1} >= 0, on a stack of pools
 *               (v, w, t, l).  For k = 0 .. F-1 push (y_k - lam (1 - g), 1, k, 1); the last frame pushes y_k - lam instead.
 *               While there are two pools a (below) and b (top) with v_b < pw[l_a] v_a, merge b into a:
 *                 num = w_a v_a + (pw[l_a] w_b) v_b,  den = w_a + pw2[l_a] w_b,
 *                 v_a = num / den, w_a = den, l_a += l_b, then pop b.
 *   Readout     For a pool i, c_{t_i + j} = pos(v_i) pw[j].  At the start of a pool i > 0:
 *               s_{t_i} = pos(pos(v_i) - g (pos(v_{i-1}) pw[l_{i-1} - 1])).  s_k = 0 everywhere else, and s_0 = 0.
 *   Results     Event byte E_k(p) = min(255, floor(s_k + 0.5)).  Event count n(p) = #{k : s_k >= s_min} as uint32 (with
 *               s_min = 0 every frame of every box pixel counts: n = F).  Event sum S(p) = sum_k s_k, added in ascending
 *               k, as double.  Off the map and in the padding y = 0 and so everything is 0; outside the box all is 0.
 *   event_planes     writes the full W x H byte planes of E of the frames k0 .. k0 + n_frames - 1 into `out`, laid out as
 *               hm_body_rec_planes lays them out.  The solution is that of the whole record whatever the window.
 *   event_stats_add  adds every recorded frame's E plane to the statistics of hm_body_stats_*, exactly as
 *               hm_body_rec_stats_add adds its planes (same state errors, same capacity rule).
 *   event_sums       writes W x H planes of n (uint32) and S (double); either may be NULL.
 *   All three: HM_ERR_ARG with the numbers in hm_last_error for detrend parameters that hm_body_rec_planes refuses, for g,
 *   lam or s_min outside their range or not finite, for a frame range outside the record, and for a record of more than
 *   65535 frames (the stack keeps frame numbers in 16 bits).  Waiting and state errors are those of hm_body_rec_planes.
 *   The record, the map and the tracker do not change by a bit.  The pool stack takes 20 bytes per frame and pixel
 *   (v, w: doubles at a pool's start; its length, 16 bits, at its start; its start, 16 bits, at its end) in a device work
 *   buffer; the box is worked through in passes over as many 64-byte segments of the box frame as fit into hm_ctx_tune
 *   "rec_ev_bytes" (hm_ctx_tune64: 1..2^34, default 2^34, one segment at least: same results for every value).  Beside it
 *   the call holds the E bytes of the frames it covers (a twentieth of what their stack would take) and, for kinds 1..3,
 *   the scratch of hm_body_rec_planes; all three are freed on every return including errors. */
int hm_body_rec_event_planes(hm_ctx_t h, int k0, int n_frames, int what, int half, int q, int floor, int gain, double g,
                             double lam, uint8_t *out);
int hm_body_rec_event_stats_add(hm_ctx_t h, int what, int half, int q, int floor, int gain, double g, double lam);
int hm_body_rec_event_sums(hm_ctx_t h, int what, int half, int q, int floor, int gain, double g, double lam, double s_min,
                           uint32_t *count, double *sum);

/* The residual of the record: every recorded frame minus the light a model of the cells puts there (hydra_mi/residual.py,
 * DESIGN.md section 15; csrc/residual_kernels.h; tests/residual_ref.py restates the rule in NumPy).  Exact integers.
 *   labels, weights   n_layers (1..4) planes of W*H in body coordinates, exactly what hm_view_set_cells takes: int32 labels,
 *               -1 none, 0 .. L-1 (L is 1..65536); uint16 weights, NULL: 65535 everywhere.
 *   traces      F x L int32, row k for recorded frame k; F is the record's frame count, also for `planes`.
 *   blank       W*H bytes, NULL: none.  offset is 0..255.
 *   Rule        For recorded frame k and map pixel p, with record value v_k(p):
 *               acc = sum_j weights[j][p] * traces[k][labels[j][p]], over the layers j with a label >= 0, in int64.  Since
 *               4 * 65535 * 2^31 < 2^50, no order matters.
 *               m = (acc + 2^23) >> 24, an arithmetic shift (floor): half a grey level goes up, -0.5 -> 0 and +0.5 -> 1.
 *               A weight of 65535 with a trace of rint(l * 2^24 / 65535) takes off l grey levels.
 *               r = offset + v_k(p) - m, and R_k(p) = min(255, max(0, r)).
 *               R_k(p) = 0 where blank[p] != 0, outside the map, and in the padding.  A blanked pixel is constant: by the
 *               rule of hm_body_stats_images it gets corr 0 and drops out of its neighbours' averages.
 *               *clipped (may be NULL) is the number of (frame, map pixel, not blanked) with r outside 0..255, over the
 *               frames the call covers.
 *   planes      writes the frames k0 .. k0 + n_frames - 1 as full W x H planes into `out`, laid out as hm_body_rec_planes
 *               lays them out.
 *   stats_add   adds every recorded frame's residual plane to the statistics of hm_body_stats_*, exactly as
 *               hm_body_rec_stats_add adds its planes: in frame order, the statistics begun (HM_ERR_STATE otherwise), and
 *               if count + F would pass the capacity it fails with HM_ERR_STATE naming the numbers and adds nothing.
 *   Both: HM_ERR_ARG with the numbers in hm_last_error for n_layers outside 1..4, L outside 1..65536, offset outside
 *   0..255, NULL labels or traces (all four before the handle is looked at), a frame range outside the record, F L >= 2^30,
 *   and a label outside -1..L-1 anywhere in the planes (checked on the host while the box is packed: nothing has run).
 *   HM_ERR_STATE without a record or without a recorded frame.  The record, the map and the tracker do not change by a bit.
 *   The frames are split over the grid in runs of hm_ctx_tune "rec_res_frames" (1..2^24, default 8: same results for
 *   every value); the scratch follows hm_body_rec_planes': at most 16 MiB (one frame at least), freed on every return
 *   including errors. */
int hm_body_rec_residual_planes(hm_ctx_t h, int k0, int n_frames, int n_layers, const int32_t *labels, const uint16_t *weights,
                                int L, const int32_t *traces, const uint8_t *blank, int offset, uint8_t *out, uint64_t *clipped);
int hm_body_rec_residual_stats_add(hm_ctx_t h, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                                   const int32_t *traces, const uint8_t *blank, int offset, uint64_t *clipped);

/* Activity waves: per event a latency map of the kept video, its sums over the events, and the sums of a local plane fit
 * (hydra_mi/waves.py; csrc/waves_kernels.h; tests/waves_ref.py restates the rule in NumPy and Python
 * integers).  Exact integers throughout.
 *   Notation    F is the number of recorded frames.  y_k(p) is the byte of the plane of kind `what` (0 raw, 1 baseline,
 *               2 excess, 3 dF/F) of frame k at box pixel p, exactly as hm_body_rec_planes defines it.  half, q, floor,
 *               gain are the same arguments with the same ranges.
 *   Binning     b is 0..8.  For a map pixel p:
 *               Y_k(p) = sum of y_k(q) over the q of the (2b+1)^2 window round p that are on the frame, in the box and
 *               in the map.  n(p) = the number of such q.  It is >= 1.  Y <= 255 * 289 < 2^17.
 *   Windows     pre is 1..64, lead is 0..64, post is 1..256.  Event e has trigger frame t_e (int32).  E is 1..65536.
 *               Baseline frames: t_e - lead - pre .. t_e - lead - 1.
 *               Search frames: k_b = t_e - lead .. k_c = t_e + post.
 *               A trigger with t_e - lead - pre < 0 or t_e + post > F - 1 is HM_ERR_ARG.  The error names the event, the
 *               trigger and F.  Nothing has run at that point.
 *   Per (e, p)  Every product below stays under 2^33: pre * M and S <= 64 * 73695 < 2^23; 2 * pre * Y and theta < 2^24;
 *               256 * d0 <= 256 * theta < 2^32; Lat^2 <= (256 * 257)^2 < 2^33.
 *               S = sum of Y over the baseline frames.
 *               M = max of Y over the search frames.
 *               k_M = the first frame that attains M.
 *               R = pre * M - S (int32; may be <= 0).
 *               theta = S + pre * M.
 *               k_x = the first search frame with 2 * pre * Y_k >= theta.
 *   Sub-frame step, when k_x > k_b:
 *               d0 = theta - 2 * pre * Y_{k_x - 1}.
 *               d1 = 2 * pre * (Y_{k_x} - Y_{k_x - 1}).  Then d1 >= d0 > 0.
 *               frac = floor(256 * d0 / d1), in 0..256.
 *               Latency Lat = 256 * (k_x - 1 - t_e) + frac, int32, in 1/256 frame relative to the trigger.
 *   Code `why`, uint8.  The first rule that applies wins:
 *               255   p off the map                                              off the map
 *               2     R < pre * n(p) * min_rise (min_rise 1..255 grey levels)    rise too small
 *               3     k_x == k_b                                                 already at half height when the search starts
 *               1     k_M == k_c                                                 valid, still rising at the window's end
 *               0     otherwise                                                  valid
 *               Lat = INT32_MIN wherever why >= 2.  (R < 0 leaves no crossing: it is code 2.)  `rise` is R on the map
 *               whatever the code, and 0 off it.
 *   Across the events of one call.  Per pixel, over the events with why <= 1:
 *               cnt (uint32).  sum_lat = sum of Lat (int64).  sum_lat2 = sum of Lat^2 (int64).  This is exact:
 *               Lat^2 < 2^33, E <= 2^16.
 *   Local fit per event.  step is 1..64, Rf is 1..16.
 *               Node (i, j) sits at box column c0 + i * step, row r0 + j * step.  i < ceil(bw / step), j < ceil(bh / step).
 *               Nodes are row-major.  The sums run over the pixels q = node + (dx, dy) with |dx|, |dy| <= Rf that are on
 *               the frame, in the map and valid in this event.  Nine int64 sums per node: n, sum dx, sum dy, sum dx^2,
 *               sum dx * dy, sum dy^2, sum Lat, sum dx * Lat, sum dy * Lat.  A node off the map is only a position; it
 *               still sums its valid neighbours.  No validity test is made on the node itself.
 *   waves       One call, any output may be NULL.  n_bin: W*H, n(p), 0 off the map.  lat, rise, why: E planes of W*H
 *               each; outside the box as off the map (why 255, Lat INT32_MIN, rise 0).  cnt, sum_lat, sum_lat2: W*H, 0
 *               off the map.  fit: E x nodes x 9.
 *   wave_nodes  The grid of `step`: nx = ceil(bw / step), ny = ceil(bh / step), and the box's corner c0, r0 (any may be
 *               NULL).  It needs the record begun (HM_ERR_STATE otherwise), not a frame in it.
 *   Waiting, state errors and the empty-map case are those of hm_body_rec_seed_sums.  A map without a pixel gives why 255
 *   everywhere (so Lat INT32_MIN) and zeros elsewhere.  It is not an error.  Every argument out of range is HM_ERR_ARG
 *   with the numbers in hm_last_error: the detrend parameters that hm_body_rec_planes refuses, E, NULL triggers, b, pre,
 *   lead, post, min_rise, step and Rf before the handle is looked at, the triggers against F after it.  The record, the
 *   map, the statistics and the tracker do not change by a bit.  A refusal leaves the record usable.
 *   One launch of the latency kernel takes hm_ctx_tune "rec_wv_frames" events (1..65535, default 16), and no more than
 *   keep its planes of lat, rise and why and, where `fit` is asked for, its sums of the fit (72 bytes per node and event)
 *   below 1 GiB together (one event at least); of kinds 1..3 a launch takes consecutive
 *   events only as long as their windows together span no more than pre + lead + post + 1 frames, whose planes
 *   (k_rec_running) go into a work buffer of the call's own in the record's layout.  That buffer, the launch's planes and
 *   the call's sums are one allocation that is freed on every return including errors; it does not count against
 *   "rec_scratch_bytes".  The bytes of every output are the same for every value of both keys. */
int hm_body_rec_waves(hm_ctx_t h, int E, const int32_t *triggers, int what, int half, int q, int floor, int gain,
                      int b, int pre, int lead, int post, int min_rise, int step, int Rf,
                      uint16_t *n_bin,            /* W*H, n(p), 0 off the map */
                      int32_t *lat, int32_t *rise, uint8_t *why,   /* E planes of W*H each; outside the box as off the map */
                      uint32_t *cnt, int64_t *sum_lat, int64_t *sum_lat2,   /* W*H */
                      int64_t *fit);              /* E x nodes x 9 */
int hm_body_rec_wave_nodes(hm_ctx_t h, int step, int *nx, int *ny, int *c0, int *r0);

/* The flow tool's preview (reference src/optical_flow_ext.cpp:172-281 colour code, :336-389 the
 * blend into <prefix>.avi): n frames (channels 1: gray, 3: B G R) and their flow planes fx, fy
 * (n x H x W f32 each) -> out n x H x W x 3, round((2 frame + 3 wheel) / 5) per channel.  wheel: the
 * 55-entry Middlebury colour code at flow / 15 px, interpolated in f32, saturation rad (x 0.75 past
 * 15 px), truncated to uint8; 0 for a non-finite flow.  on_device 0: host arrays, synchronous;
 * 1: device arrays, queued on `stream`. */
int hm_flow_preview(int device, int n, int W, int H, int channels, const uint8_t *frames, const float *fx,
                    const float *fy, uint8_t *out, int on_device, void *stream);

/* The video container (reference src/optical_flow_ext.cpp:351-358 cv::VideoWriter at 20 frames/s;
 * run_kalmanfilter.py:43-44 the output video): uncompressed 24-bit AVI, one 'DIB ' stream, rows
 * bottom-up padded to 4 bytes, 'idx1' for the first RIFF; past riff_limit bytes (0: 1 GiB) the file
 * goes on in OpenDML 'AVIX' RIFFs, every RIFF indexed by an 'ix00' chunk named in the 'indx' super
 * index, the total frame count in 'odml'/'dmlh'.  Frames are H x W x 3 B G R, rows top to bottom.
 * Host only; close writes the indices and frees the handle. */
typedef struct hm_avi *hm_avi_t;
int hm_avi_open(const char *path, int W, int H, int fps, uint64_t riff_limit, hm_avi_t *out);
int hm_avi_write(hm_avi_t avi, const uint8_t *bgr);
int hm_avi_close(hm_avi_t avi);

/* The same container around compressed frames.  codec HM_AVI_RAW: exactly hm_avi_open (frames through hm_avi_write).
 * codec HM_AVI_MJPG: Motion-JPEG, one complete JPEG file per frame through hm_avi_write_chunk(data, n), n in 1..2^31-1.
 * The stream's fccHandler and biCompression are 'MJPG' (biBitCount 24, biSizeImage that of the raw frame), dwSampleSize is 0,
 * the chunks are '00dc', written as they come and followed by one zero byte when n is odd; 'idx1' (first RIFF, every
 * entry with AVIIF_KEYFRAME) and 'ix00' hold each chunk's own n, 'indx' names '00dc'.  dwSuggestedBufferSize (avih and
 * strh: the largest n + 8) and dwMaxBytesPerSec (the largest n x fps) are patched at close.  A chunk that would take the
 * RIFF past riff_limit (0: 1 GiB; at least 16384), counted with its padding and the indexes as hm_avi_write counts, opens
 * the next 'AVIX' RIFF; a single chunk larger than the limit gets a RIFF to itself.  hm_avi_write refuses a file opened
 * for MJPG and hm_avi_write_chunk one opened raw (HM_ERR_ARG); any other codec is refused with its number. */
#define HM_AVI_RAW 0
#define HM_AVI_MJPG 1
int hm_avi_open_codec(const char *path, int W, int H, int fps, uint64_t riff_limit, int codec, hm_avi_t *out);
int hm_avi_write_chunk(hm_avi_t avi, const uint8_t *data, uint64_t n);

/* Motion-JPEG: a baseline sequential JPEG encoder (ITU-T T.81) on the device, for the frames the views leave there.
 * Integers only; tests/mjpeg_ref.py restates every rule below and the device gives the same bytes.
 *
 *   Frame       H x W x channels bytes, rows top to bottom; channels 1 (grey, one component) or 3 (B G R in memory, coded
 *               as Y Cb Cr, every component at full resolution: 4:4:4).
 *   Colour      Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *               Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *               Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16        (>>: arithmetic; all in 0..255)
 *               With one channel the sample is the byte.  128 is taken off every sample: s in -128..127.
 *   Blocks      bw = ceil(W / 8) by bh = ceil(H / 8) blocks of 8 x 8; pixels past the frame repeat its last column and row.
 *   DCT         T[u][x] = rint(2^13 (c(u) / 2) cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2, c(u > 0) = 1.
 *               rows:    r[y][u]  = (sum_x T[u][x] s[y][x] + 2^10) >> 11      (two fractional bits are kept)
 *               columns: c8[v][u] = (sum_y T[v][y] r[y][u] + 2^11) >> 12      (v: vertical frequency)
 *               c8 is the coefficient in eighths, c = c8 / 8: the quantiser sees three fractional bits, as libjpeg's does.
 *               32-bit sums; DESIGN section 21 shows that none overflows and bounds |c - exact| by E = 0.66.
 *   Tables      Quantisation: Annex K tables K.1 (Y, grey) and K.2 (Cb, Cr) scaled as libjpeg does: s = 5000 / quality
 *               (integer division) below quality 50, else 200 - 2 quality; q = min(255, max(1, (v s + 50) / 100)).
 *               Huffman: the typical tables K.3 - K.6, table 0 for Y / grey and table 1 for Cb and Cr.
 *   Quantise    k = sign(c) floor((2 |c| + q) / (2 q)), in integers sign(c8) ((2 |c8| + 8 q) / (16 q)) with integer
 *               division; then zigzag order.
 *   Coding      Per block: the DC difference to the previous block of the same component in the restart interval (0 for
 *               the first) as its category's code and the category's low bits (of diff - 1 when negative); the AC
 *               coefficients as (run, size) codes with the value's low bits likewise, ZRL (F0) for every 16 zeros of a
 *               run before a non-zero coefficient, EOB (00) if and only if the block ends in a zero.  With three
 *               components the blocks of a position follow each other: Y, Cb, Cr.  Bits fill bytes from the most
 *               significant end.
 *   Intervals   A restart interval is restart_rows rows of blocks (the last may have fewer): ri = bw min(restart_rows, bh)
 *               positions.  It ends padded to a byte with 1-bits; every FF byte of it (the padded one included) is
 *               followed by 00; RSTm (FF D0+m, m = the interval's index mod 8) follows every interval but the last,
 *               EOI (FF D9) the last.  The DC prediction starts again at 0.
 *   Header      SOI; APP0 JFIF 1.01, no units, 1:1; DQT table 0 (and 1 with three components), 8-bit, zigzag order;
 *               SOF0 (8 bits, H, W, components 1.. with sampling 1x1 and tables 0, 1, 1); DHT DC 0, AC 0 (then DC 1, AC 1
 *               with three components), one segment each; DRI ri; SOS (components with tables 00, 11, 11; 0, 63, 0).
 *   Stream      what follows the header: the intervals with their markers, EOI included, dense.
 *
 * hm_mjpeg_create   builds the tables and the header on the host; nothing runs on the device before the first encode,
 *               which allocates the handle's buffers there (128 bytes of coefficients and 208 of bit buffer per block).
 *               HM_ERR_ARG with the numbers in hm_last_error for W or H outside 1..32767, channels not 1 or 3, quality
 *               outside 1..100, restart_rows < 1, ri > 65535 (DRI is a 16-bit field), and a frame whose stream could
 *               reach 2^31 bytes.
 * hm_mjpeg_header   copies the header (SOI through SOS) and gives its length in *n; buf NULL: the length alone; a cap
 *               below it is refused.
 * hm_mjpeg_max_bytes  the largest file a frame can code to: the header, 416 bytes per block (64 coefficients of at most
 *               26 bits, every byte stuffed) and a marker per interval.
 * hm_mjpeg_encode_dev  queues the encode of the frame at device address d_frame on `stream` and returns.  The stream
 *               (no header) goes to `out`, device or page-locked host memory of `cap` bytes; its size to *size_word,
 *               device or page-locked host memory, written by the last launch.  The size is known on the device before a
 *               byte is written: a stream larger than cap is not written at all and the size word (> cap) says so.  The
 *               handle's bit buffer is all zero between frames (the launch that reads it clears it), so no frame sees
 *               another's bits.  One encode of a handle at a time: queue them on one stream, or order them yourself.
 * hm_mjpeg_encode   host frame in, whole JPEG file (header + stream) out, synchronous, on a stream of the handle's own.
 *               *n is the file's size also when it does not fit: then HM_ERR_ARG names both numbers and `out` is untouched.
 * Plain HIP: vector stores and ordinary atomics (atomicOr into the bit buffer, one LDS atomicAdd). */
typedef struct hm_mjpeg *hm_mjpeg_t;
int hm_mjpeg_create(int device, int W, int H, int channels, int quality, int restart_rows, hm_mjpeg_t *out);
int hm_mjpeg_destroy(hm_mjpeg_t enc);
int hm_mjpeg_header(hm_mjpeg_t enc, uint8_t *buf, uint64_t cap, uint64_t *n);
uint64_t hm_mjpeg_max_bytes(hm_mjpeg_t enc);
int hm_mjpeg_encode_dev(hm_mjpeg_t enc, const void *d_frame, void *out, uint64_t cap, uint32_t *size_word, void *stream);
int hm_mjpeg_encode(hm_mjpeg_t enc, const uint8_t *frame, uint8_t *out, uint64_t cap, uint64_t *n);

/* Motion-JPEG, decoding: a baseline JPEG decoder on the device for the frames of an MJPG video, bit-equal to libjpeg's
 * default ("islow") decoder.  tests/mjpeg_dec_ref.py restates every rule below; DESIGN section 23.
 *
 *   Accepted    Baseline sequential DCT (SOF0), 8 bits; one component, or three (Y Cb Cr) in one interleaved scan with luma
 *               sampling factors 1 or 2 each way and chroma 1 x 1 (4:4:4, 4:2:2 either way, 4:2:0); up to four 8-bit
 *               quantisation tables; Huffman tables from DHT segments anywhere before SOS, and for a table the scan names
 *               but no DHT defined the Annex K table of its class and index (K.3 - K.6; index 0 or 1); DRI of any value or
 *               none; APPn, COM and other segments with a length are skipped; FF fill bytes before a marker are allowed.
 *               With one component the sampling factors mean nothing: an MCU is one block.
 *   Refused     on the host, HM_ERR_ARG with the marker or field in hm_last_error: SOF1 and above, DAC, a precision other
 *               than 8, a 16-bit DQT, two or four components, a scan that does not hold every component (several scans), a
 *               second SOS, other sampling factors, a scan that is not 0..63 / 0, any marker but RSTn and EOI inside the
 *               scan, and (by the decoder) a frame size other than the handle's.
 *   Output      the one component, or of three the luma plane (what libjpeg gives for grey output, PIL's
 *               draft("L", size)); chroma blocks are Huffman-decoded to step over them and never transformed.  On in-gamut
 *               colours this is within rounding of rint(0.114 B + 0.587 G + 0.299 R) of the decoded colours; where the
 *               colour conversion clamps R, G or B it is not (up to 16 grey levels on saturated noise).
 *   Intervals   The host scans the entropy-coded segment once for markers (FF followed by neither 00 nor FF).  With DRI = Ri
 *               the RSTn found must number ceil(MCUs / Ri) - 1 and run 0..7 in turn, else the frame is refused; interval i
 *               is the bytes between the markers, [start, end), and begins at MCU i Ri.  Without DRI the frame is one
 *               interval.  EOI ends the last; a file cut before EOI ends it with the file.
 *   Entropy     Per interval, DC predictions from 0.  A block: the DC category t (Huffman) and t bits (EXTEND), added to the
 *               component's prediction in 32-bit wrap, the coefficient being the low 16 bits; then (run, size) symbols:
 *               size 0 with run 15 moves 16 places (ZRL), size 0 otherwise ends the block, else run places are skipped and
 *               size bits give the coefficient.  An MCU is hs x vs luma blocks, rows first, then one Cb and one Cr block.
 *               Bytes: FF 00 is the data byte FF; an FF that no 00 follows ends the interval's data.
 *   Bad         An interval is bad from the block in which a code is of no table, a DC category is above 11 or an AC size
 *               above 10, a run or ZRL leaves index 63, or a bit is needed after the data ended.  That block and the rest
 *               of the interval are all-zero coefficients (grey 128); the frame's status word counts its bad intervals.
 *   Transform   coefficient x table entry, then libjpeg's jidctint.c: columns first, CONST_BITS 13, PASS1_BITS 2, descale
 *               by 11 (pass 1) and 18 (pass 2) with rounding, the result through x & 1023 into the range-limit table
 *               centred on 128.  All sums in 32-bit two's-complement wrap (uint32_t).  Equal to libjpeg for every stream
 *               whose dequantised coefficients fit 16 bits (every stream an encoder writes); beyond, this is the rule.
 *   Planes      the grey frame and, when their addresses are given, mask = frame > threshold (0 or 1) and shown =
 *               mask x frame; every plane W x H at the caller's row pitch, frames of a run frame_stride bytes apart.
 *
 * hm_mjpeg_probe    host only: what the headers and the marker scan say.  hm_mjpeg_intervals: the interval table, three
 *               words (start, end, first MCU) per interval.
 * hm_mjpeg_dec_create  W, H in 1..32767, max_run (frames per hm_mjpeg_decode_run_dev) in 1..64; nothing runs on the device
 *               before the first decode, which allocates the handle's buffers (128 bytes of coefficients per luma block
 *               and frame of a run).  One owner for buffers, streams and events, released by hm_mjpeg_dec_destroy.
 * hm_mjpeg_dec_tune    "entropy": HM_MJPEG_ENTROPY_AUTO / _HOST / _DEVICE: where the intervals are Huffman-decoded; both
 *               give the same coefficients.  "auto_intervals": the intervals per frame from which AUTO takes the device
 *               path, default 512 (measured at 1024^2: DESIGN section 23); 0: the device path exactly when the frame has a
 *               DRI.  "pool": threads of the host path, 1..16, default 4, a frame at a time each; they are started by the
 *               first run that needs them and sleep between runs.  On the host path the CPU does the Huffman decoding and
 *               the coefficients are uploaded (hm_mjpeg_dec_uploaded).
 * hm_mjpeg_dec_entropy_host  host only: the coefficients of every luma block in scan order (MCU by MCU), 64 each in zigzag
 *               order, and the number of bad intervals.  coef: cap values, 8-byte aligned.
 * hm_mjpeg_decode_run_dev  parses the frames (refusing before anything is queued), queues copies and two launches on
 *               `stream` and returns: the planes of frame i at d_frame / d_mask / d_shown + i frame_stride (mask and shown
 *               may be NULL), status_words[i] (device or page-locked memory, may be NULL) the frame's bad intervals.  No
 *               state is carried between frames.  Staging is page-locked and used in turns of two; after the first decode
 *               nothing is allocated unless a run has more bytes or intervals than any before.
 * hm_mjpeg_dec_uploaded  the bytes that hm_mjpeg_decode_run_dev queued from host to device, in the last run and in all
 *               runs of the handle (either pointer may be NULL).  Per frame of a run that is a descriptor of
 *               HM_MJPEG_DESC_BYTES (scan, quantisation table, decode tables) and then, on the device entropy path, the
 *               file's bytes rounded up to a multiple of 16 and 12 bytes per interval; on the host entropy path the Huffman
 *               decoding has run on the CPU and the coefficients cross instead, 128 bytes per luma block of the scan,
 *               which is 2 bytes per pixel of the padded frame and more than the file.
 * hm_mjpeg_decode   one frame to host memory (W x H bytes), synchronous, on a stream of the handle's own; *bad (may be
 *               NULL) the bad intervals; with strict != 0 a frame with bad intervals is HM_ERR_ARG (out is still written).
 * Plain HIP: vector stores (32-bit words where base, stride and pitch are multiples of 4, else bytes), one atomicAdd. */
typedef struct hm_mjpeg_info {
    int32_t W, H, components, hs, vs, ri;       /* hs, vs: luma blocks of an MCU; ri: the DRI value, 0 without */
    uint32_t intervals, mcus;
} hm_mjpeg_info;
#define HM_MJPEG_DESC_BYTES 5608
#define HM_MJPEG_ENTROPY_AUTO 0
#define HM_MJPEG_ENTROPY_HOST 1
#define HM_MJPEG_ENTROPY_DEVICE 2
typedef struct hm_mjpeg_dec *hm_mjpeg_dec_t;
int hm_mjpeg_probe(const uint8_t *file, uint64_t n, hm_mjpeg_info *info);
int hm_mjpeg_intervals(const uint8_t *file, uint64_t n, uint32_t *table, uint64_t cap);
int hm_mjpeg_dec_create(int device, int W, int H, int max_run, hm_mjpeg_dec_t *out);
int hm_mjpeg_dec_destroy(hm_mjpeg_dec_t dec);
int hm_mjpeg_dec_tune(hm_mjpeg_dec_t dec, const char *name, int value);
int hm_mjpeg_dec_entropy_host(hm_mjpeg_dec_t dec, const uint8_t *file, uint64_t n, int16_t *coef, uint64_t cap, uint32_t *bad);
int hm_mjpeg_decode_run_dev(hm_mjpeg_dec_t dec, int nframes, const uint8_t *const *files, const uint64_t *sizes, void *d_frame,
                            void *d_mask, void *d_shown, uint64_t frame_stride, uint64_t pitch, int threshold,
                            uint32_t *status_words, void *stream);
int hm_mjpeg_dec_uploaded(hm_mjpeg_dec_t dec, uint64_t *last_run, uint64_t *total);
int hm_mjpeg_decode(hm_mjpeg_dec_t dec, const uint8_t *file, uint64_t n, uint8_t *out, int strict, uint32_t *bad);

/* 16-bit input: frames of unsigned 16-bit pixels mapped to the 8 bits everything downstream works in, through one window
 * for the whole recording chosen from its histogram.  tests/deep_ref.py restates every rule below; DESIGN section 24.
 *
 *   Histogram   h[v], v = 0..65535, counts the pixels of the frames given.  The counts are exact 64-bit integers.  It is
 *               additive over calls until reset.
 *   Window      Inputs are lo_ppm and hi_ppm, whole parts per million in 0..1 000 000.  N = sum h, and cum(v) = sum of
 *               h[u] over u <= v.  lo is the least v with cum(v) > N lo_ppm // 10^6 (with lo_ppm = 10^6 there is none: then
 *               lo = 65535, and the repair below applies).  hi is the least v with
 *               cum(v) >= max(1, (N hi_ppm + 10^6 - 1) // 10^6).  If hi <= lo, then hi = lo + 1, capped at 65535 with
 *               lo = 65534.  No floating point is used.  Defaults: lo_ppm = 1000 and hi_ppm = 999 990; these are policy,
 *               not measurements, and every interface exposes them.  (The window is computed on the host, from
 *               hm_deep_hist_get: hydra_mi.deepio.window.)
 *   Table       lut[v] for all 65536 v, with t = min(max(v, lo), hi) - lo and D = hi - lo.  With gamma = 1 (the default),
 *               lut[v] = (510 t + D) // (2 D): this rounds half up.  Otherwise lut[v] = floor(255 (t / D)^gamma + 0.5) in
 *               binary64.  The host makes the table once (hydra_mi.deepio.make_lut); the device only applies it, so host
 *               and device agree by construction.
 *   Mapping     raw = lut[v], mask = raw > threshold, shown = mask ? raw : 0.  threshold is on the 8-bit scale, as the
 *               tracker's -t is everywhere else.  swap = 1 exchanges the two bytes of v first, for big-endian files.  Per
 *               frame there are two 32-bit counts: pixels with v < lo and pixels with v > hi.
 *
 * hm_deep_create  W, H in 1..32767, max_run (frames per hm_deep_map_run_dev) in 1..64; nothing runs on the device before
 *               the first call that needs it, which allocates the handle's buffers: max_run frames of 16-bit pixels on
 *               the device and twice that page-locked, the table, 65536 64-bit counts.  One owner for buffers, streams
 *               and events, released by hm_deep_destroy.
 * hm_deep_hist_reset / _add / _get  the histogram of the handle.  add takes nframes >= 1 dense frames of W x H uint16 in
 *               host memory, works through them max_run frames at a time on a stream of the handle's own and returns when
 *               they are counted.  get: hist[65536] and (samples may be NULL) the pixels counted, the sum of hist.
 * hm_deep_set_lut  the table (65536 bytes, copied) and the window it was made for, 0 <= lo < hi <= 65535; lo >= hi is
 *               HM_ERR_ARG with both numbers.  The device reads lut[min(max(v, lo), hi)], so only lut[lo .. hi] matters.
 * hm_deep_map_run_dev  queues, on `stream`, the copy of nframes (1..max_run) dense host frames and one launch, and returns:
 *               the planes of frame i at d_frame / d_mask / d_shown + i stride (stride >= W H bytes; mask and shown may be
 *               NULL), rows dense, nothing outside W H bytes of each frame's plane written; d_status (device or page-locked
 *               memory, may be NULL): 2 nframes words, frame i's pixels below lo and above hi.  Refused with the numbers in
 *               hm_last_error: nframes outside 1..max_run, a threshold outside 0..255 (HM_ERR_ARG), no table set
 *               (HM_ERR_STATE).  Staging is page-locked and used in turns of two; the host frames may be reused on return.
 *               One map of a handle at a time: queue them on one stream, or order them yourself.
 * hm_deep_map     one frame to host memory (W x H bytes, threshold 0, no mask), synchronous, on the handle's stream;
 *               clipped (may be NULL): the two counts.
 * hm_deep_uploaded  the bytes hm_deep_map_run_dev queued from host to device, in the last run and in all runs (either
 *               pointer may be NULL): 2 W H per frame.
 * Plain HIP, integers only: vector stores (8 bytes where the addresses allow, else bytes), LDS and global atomicAdd. */
typedef struct hm_deep *hm_deep_t;
int hm_deep_create(int device, int W, int H, int max_run, hm_deep_t *out);
int hm_deep_destroy(hm_deep_t deep);
int hm_deep_hist_reset(hm_deep_t deep);
int hm_deep_hist_add(hm_deep_t deep, int64_t nframes, const uint16_t *host_frames, int swap);
int hm_deep_hist_get(hm_deep_t deep, uint64_t *hist, uint64_t *samples);
int hm_deep_set_lut(hm_deep_t deep, const uint8_t *lut, int lo, int hi);
int hm_deep_map_run_dev(hm_deep_t deep, int nframes, const uint16_t *host_frames, int swap, void *d_frame, void *d_mask,
                        void *d_shown, uint64_t stride, int threshold, uint32_t *d_status, void *stream);
int hm_deep_map(hm_deep_t deep, const uint16_t *host_frame, int swap, uint8_t *out, uint32_t *clipped);
int hm_deep_uploaded(hm_deep_t deep, uint64_t *last_run, uint64_t *total);

/* Full-depth traces: a second pass over the 16-bit frames once the track and the cells are known.  The frames are uploaded
 * run by run as above; only the body pixels that belong to some column (an ROI, a ring, a shape) are pulled back through
 * the tracked mesh, by the body warp's own rule, and summed at full depth in exact integers.  Where the cells are stays
 * the 8-bit pipeline's decision; only how bright they are is read again, from the camera's numbers.
 * tests/deeptrace_ref.py restates every rule below; DESIGN section 25.
 *
 *   Value       For a body pixel p (raster index in body coordinates) and frame k, the full-depth registered value
 *               v16_k(p) follows k_body_warp's rule (csrc/body_kernels.h, d_body_px).  It uses the same body map, the same
 *               barycentrics and the same binary64 position, computed without contraction.  It takes the same bilinear
 *               sample at (x - 0.5, y - 0.5), with texels clamped to the frame.  It rounds with the same rint, half to even.
 *               The texels are the frame's unsigned 16-bit pixels.  With swap = 1 their two bytes are exchanged first, at
 *               the gather, with no extra pass over the frame.  It is 0 off the map, and 0 where x or y is not finite or
 *               lies beyond +-2^20 px.  The result lies in 0..65535.
 *   Columns     A readout is C columns, 1 <= C <= 4096, in compressed-column form: col_ptr[C + 1] is int64, ascending,
 *               with col_ptr[0] = 0; pix[M] is int32, each entry a raster index in 0..W H - 1; wt[M] is uint16
 *               (M = col_ptr[C], at most 2^30).  A column may be empty, and a pixel may appear in any number of columns.
 *               The sums are
 *                   sums[k C + s] = sum over e in column s of wt[e] v16_k(pix[e])   (uint64).
 *               An entry whose pixel is off the map adds 0.  No magnitude bound is needed: 2^30 entries x 65535^2 < 2^63.
 *   Planes      Optionally, each frame's whole registered plane is returned: W H uint16 values, 0 off the map -- the
 *               16-bit twin of hm_body_warp's out.
 *
 * Both calls take the deep handle and the filter handle.  The deep handle owns the upload path (its device copies of a
 * run, its two page-locked staging blocks used in turn, an upload stream) and the columns, states, sums and planes on the
 * device, all released by hm_deep_destroy; the filter handle owns the body map, built on first use as ever.  Both must be
 * on one device and have one W x H: otherwise HM_ERR_ARG with both sizes.
 * hm_deep_body_set_columns  copies the columns to the device; they stay until they are set again or cleared (pix NULL).
 *               HM_ERR_ARG, with the numbers: C outside 1..4096; a col_ptr that does not start at 0 or is not ascending
 *               (the column is named); more than 2^30 entries; a pix outside the frame (the entry is named).
 * hm_deep_body_run  nframes >= 1 dense host frames of W x H uint16 (of any number: they are worked through max_run at a time)
 *               and X, one state per frame, dense, 4N doubles each, of which the first 2N are read as hm_body_warp reads
 *               them.  sums: nframes C values; planes: nframes W H values; either may be NULL, not both (HM_ERR_ARG).
 *               Sums without columns set: HM_ERR_STATE.  Runs alternate between two device copies, so that the upload
 *               of run i + 1 (from page-locked blocks, on the upload stream, queued before run i's downloads) is free to go
 *               beside the kernels of run i (on the handle's stream): that is the intent, and whether the two overlap is
 *               the runtime's to decide (DESIGN section 25 could not measure it).  Returns when everything
 *               has been computed and downloaded; waits for the filter handle's helper, and for its stream only while the
 *               map is built; changes nothing on the filter handle.  One call on a pair of handles at a time.
 *               k_deep_cols (the sums): a wave takes one column of one frame and strides through its entries; a column of
 *               more than hm_ctx_tune "deep_col_entries" (64..2^30, default 1024) entries is cut into pieces of that many
 *               whose 64-bit partial sums meet in integer atomics: the same bytes for every value of the key.  A pixel in
 *               several columns is warped once per column.  k_body_warp16 (the planes): 4 pixels a thread. */
int hm_deep_body_set_columns(hm_deep_t deep, hm_ctx_t ctx, int C, const int64_t *col_ptr, const int32_t *pix, const uint16_t *wt);
int hm_deep_body_run(hm_deep_t deep, hm_ctx_t ctx, int64_t nframes, const uint16_t *host_frames, int swap, const double *X,
                     uint64_t *sums, uint16_t *planes);

#ifdef __cplusplus
}
#endif
#endif /* HYDRA_MI_H */
