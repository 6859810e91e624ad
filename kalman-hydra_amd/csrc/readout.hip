// The readout of a filter handle: views (hm_view*), the body-frame readout and its statistics (hm_body_*, hm_body_stats_*),
// the registered video kept on the device with its reductions (hm_body_rec_*), and the flow tool's preview.  Host
// orchestration and C-ABI (include/hydra_mi.h); the kernels are in view_kernels.h, body_kernels.h, roi_kernels.h,
// stab_kernels.h and detrend_kernels.h, which this translation unit alone compiles.  Of the handle (ctx.h) it uses its own three members -- view, body, rec -- and reads
// W, H, N, T, device, own, stream, the mesh (d_tri, d_uv, d_tex) and, for the overlay view, have_tex, have_obs and o_yim.
#include "ctx.h"
#include "view_kernels.h"
#include "body_kernels.h"
#include "roi_kernels.h"
#include "stab_kernels.h"
#include "detrend_kernels.h"
#include "residual_kernels.h"
#include <algorithm>
#include <cstring>

// ---- views of a context (reference renderer.py:436-475 screenshot, :595-628 draw; kalman.py:638-674 plotforces) ------
static int view_buffers(hm_ctx *h)
{
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(alloc_targets(h->own, h->view.targets, n));
    HM_HIP(h->own.alloc(&h->view.setup, (size_t)h->T * sizeof(TriSetup)));
    HM_HIP(h->own.alloc(&h->view.ids, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->view.lab, (size_t)h->T * sizeof(int)));
    HM_HIP(h->own.alloc(&h->view.wire, n * sizeof(unsigned)));
    HM_HIP(h->own.alloc(&h->view.mm, 2 * sizeof(unsigned)));
    HM_HIP(h->own.alloc(&h->view.force, (size_t)10 * h->N * sizeof(double)));
    HM_HIP(h->own.alloc(&h->view.out, 3 * n));
    HM_HIP(h->own.event(&h->view.ev));
    HM_HIP(h->own.alloc(&h->view.X, (size_t)4 * h->N * sizeof(double)));
    return HM_OK;
}

// Queue view `which` (VIEW_*) of state X (host) into d_out (device, W*H*3) on the handle's stream.  palette: the mask
// view's label per triangle (NULL: -1, i.e. (255, 255, 255)).  forces (VIEW_FORCES_BASE): orig | pred | tv | fv | mv,
// 2N doubles each, host.
static int view_queue(hm_ctx *h, const double *X, int which, const int32_t *palette, const double *const forces[5],
                      uint8_t *d_out, const char *who)
{
    HM_ARG(h && X && d_out, "%s: NULL argument", who);
    HM_ARG(which >= VIEW_RAW && which <= VIEW_FORCES_BASE, "%s: view %d outside 0..%d", who, which, VIEW_FLOWY);
    HM_JOIN_LAZY(h);
    if (!h->have_tex) { hm_set_error("%s: hm_set_texture has not been called", who); return HM_ERR_STATE; }
    if ((which == VIEW_OVERLAY || which == VIEW_FORCES_BASE) && !h->have_obs) {
        hm_set_error("%s: the overlay shows the observed frame, and hm_set_observation has not been called", who);
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    int rc = view_buffers(h);
    if (rc) return rc;
    const int n = h->W * h->H;
    HM_HIP(hipMemcpyAsync(h->view.X, X, (size_t)4 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    Mesh m = {h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    ekf_queue_setup_all(h->stream, m, h->view.X, h->view.setup);
    if (which == VIEW_MASK) {
        if (palette) HM_HIP(hipMemcpyAsync(h->view.lab, palette, (size_t)h->T * sizeof(int), hipMemcpyHostToDevice, h->stream));
        else HM_HIP(hipMemsetAsync(h->view.lab, 0xFF, (size_t)h->T * sizeof(int), h->stream));
        ekf_queue_render(h->stream, m, h->view.X, h->view.setup, h->view.targets, h->view.lab, h->view.ids);
    } else {
        ekf_queue_render(h->stream, m, h->view.X, h->view.setup, h->view.targets, nullptr, nullptr);
    }
    const bool wire = which == VIEW_TEXTURE || which == VIEW_OVERLAY || which == VIEW_MASK || which == VIEW_FORCES_BASE;
    if (wire) {
        HM_HIP(hipMemsetAsync(h->view.wire, 0, (size_t)n * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_view_wire, dim3(hm_cdiv(3 * h->T, 256 / VIEW_SEG_WAVE)), dim3(256), 0, h->stream,
                           (const int *)h->d_tri, h->T, (const double *)h->view.X, h->W, h->H, h->view.wire);
    }
    ViewArgs a;
    a.n = n; a.which = which;
    a.acc = h->view.targets.acc; a.cnt = h->view.targets.cnt; a.ids = h->view.ids;
    a.flow = which == VIEW_FLOWY ? h->view.targets.fy : h->view.targets.fx;
    a.mm = h->view.mm;
    a.wire = wire ? h->view.wire : nullptr;
    a.obs = h->o_yim;
    a.out = d_out;
    if (which == VIEW_FLOWX || which == VIEW_FLOWY) {
        HM_HIP(hipMemsetAsync(h->view.mm, 0xFF, sizeof(unsigned), h->stream));
        HM_HIP(hipMemsetAsync(h->view.mm + 1, 0, sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_view_minmax, dim3(std::min(hm_cdiv(n, 256), 256)), dim3(256), 0, h->stream, a.flow, n, h->view.mm);
    }
    hipLaunchKernelGGL(k_view_compose, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, a);
    if (which == VIEW_FORCES_BASE) {
        const size_t n2 = (size_t)2 * h->N;
        for (int k = 0; k < 5; k++)
            HM_HIP(hipMemcpyAsync(h->view.force + k * n2, forces[k], n2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const double *o = h->view.force, *p = o + n2;
        const dim3 ag(hm_cdiv(3 * h->N, 256 / VIEW_SEG_WAVE));
        // reference kalman.py:654-661, in its order: prediction (white), template (blue), flow (green), mask (red) force
        hipLaunchKernelGGL(k_view_arrows, ag, dim3(256), 0, h->stream, o, p, (const double *)nullptr, 0.0, h->N, h->W, h->H,
                           make_uchar3(255, 255, 255), d_out);
        hipLaunchKernelGGL(k_view_arrows, ag, dim3(256), 0, h->stream, p, (const double *)nullptr, (const double *)(p + n2), 10.0,
                           h->N, h->W, h->H, make_uchar3(255, 0, 0), d_out);
        hipLaunchKernelGGL(k_view_arrows, ag, dim3(256), 0, h->stream, p, (const double *)nullptr, (const double *)(p + 2 * n2),
                           10.0, h->N, h->W, h->H, make_uchar3(0, 255, 0), d_out);
        hipLaunchKernelGGL(k_view_arrows, ag, dim3(256), 0, h->stream, p, (const double *)nullptr, (const double *)(p + 3 * n2),
                           10.0, h->N, h->W, h->H, make_uchar3(0, 0, 255), d_out);
    }
    HM_HIP(hipGetLastError());
    return HM_OK;
}

static int view_download(hm_ctx *h, uint8_t *bgr)
{
    HM_HIP(hipMemcpyAsync(bgr, h->view.out, (size_t)3 * h->W * h->H, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_view(hm_ctx_t h, const double *X, int which, const int32_t *palette, uint8_t *bgr)
{
    HM_ARG(h && bgr, "hm_view: NULL argument");
    HM_ARG(which >= VIEW_RAW && which <= VIEW_FLOWY, "hm_view: view %d outside 0..%d", which, VIEW_FLOWY);
    HM_JOIN_LAZY(h);                             // (view_buffers may create resources: the helper must not be queueing)
    HM_HIP(hipSetDevice(h->device));
    int rc = view_buffers(h);
    if (rc) return rc;
    rc = view_queue(h, X, which, palette, nullptr, h->view.out, "hm_view");
    if (rc) return rc;
    return view_download(h, bgr);
}

extern "C" int hm_view_dev(hm_ctx_t h, const double *X, int which, const int32_t *palette, void *d_bgr, void *stream)
{
    HM_ARG(h && d_bgr, "hm_view_dev: NULL argument");
    HM_ARG(which >= VIEW_RAW && which <= VIEW_FLOWY, "hm_view_dev: view %d outside 0..%d", which, VIEW_FLOWY);
    int rc = view_queue(h, X, which, palette, nullptr, (uint8_t *)d_bgr, "hm_view_dev");
    if (rc) return rc;
    if (stream) {
        HM_HIP(hipEventRecord(h->view.ev, h->stream));
        HM_HIP(hipStreamWaitEvent((hipStream_t)stream, h->view.ev, 0));
    }
    return HM_OK;
}

extern "C" int hm_view_forces(hm_ctx_t h, const double *X, const double *orig, const double *pred, const double *tv,
                              const double *fv, const double *mv, uint8_t *bgr)
{
    HM_ARG(h && bgr && orig && pred && tv && fv && mv, "hm_view_forces: NULL argument");
    HM_JOIN_LAZY(h);                             // (view_buffers may create resources: the helper must not be queueing)
    HM_HIP(hipSetDevice(h->device));
    int rc = view_buffers(h);
    if (rc) return rc;
    const double *f[5] = {orig, pred, tv, fv, mv};
    rc = view_queue(h, X, VIEW_FORCES_BASE, nullptr, f, h->view.out, "hm_view_forces");
    if (rc) return rc;
    return view_download(h, bgr);
}

// ---- the cell overlay (view_kernels.h: k_view_cells) ----------------------------------------------------------------
extern "C" int hm_view_set_cells(hm_ctx_t h, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                                 const uint8_t *colours)
{
    HM_ARG(h != nullptr, "hm_view_set_cells: NULL handle");
    if (labels) {
        HM_ARG(n_layers >= 1 && n_layers <= CV_MAX_LAYERS, "hm_view_set_cells: n_layers %d outside 1..%d", n_layers, CV_MAX_LAYERS);
        HM_ARG(L >= 1 && colours, "hm_view_set_cells: %d labels (need at least 1) or no colours", L);
        const size_t nl = (size_t)n_layers * h->W * h->H;
        for (size_t p = 0; p < nl; p++)
            HM_ARG(labels[p] >= -1 && labels[p] < L, "hm_view_set_cells: label %d at pixel %zu of layer %zu outside -1..%d",
                   (int)labels[p], p % ((size_t)h->W * h->H), p / ((size_t)h->W * h->H), L - 1);
    }
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipStreamSynchronize(h->stream));          // (a view in flight reads the cells in place)
    ViewState &v = h->view;
    v.c_layers = 0;
    if (!labels) return HM_OK;
    const size_t n = (size_t)h->W * h->H, nl = (size_t)n_layers * n;
    HM_HIP(h->own.grow(&v.c_lab, nl * sizeof(int)));
    if (weights) HM_HIP(h->own.grow(&v.c_w, nl * sizeof(uint16_t)));
    HM_HIP(h->own.grow(&v.c_col, (size_t)3 * L));
    HM_HIP(h->own.alloc(&v.c_outline, n));
    HM_HIP(hipMemcpyAsync(v.c_lab, labels, nl * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (weights) HM_HIP(hipMemcpyAsync(v.c_w, weights, nl * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(v.c_col, colours, (size_t)3 * L, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_view_cell_outline, dim3(hm_cdiv((int)n, 256)), dim3(256), 0, h->stream, (const int *)v.c_lab, h->W, h->H,
                       v.c_outline);
    HM_HIP(hipGetLastError());
    HM_HIP(hipStreamSynchronize(h->stream));
    v.c_weighted = weights != nullptr;
    v.c_L = L;
    v.c_layers = n_layers;
    return HM_OK;
}

// Queue the cell view of frame d_frame (device) at state X (host) into d_out (device, W*H*3) on the handle's stream.
static int view_cells_queue(hm_ctx *h, const double *X, const uint8_t *d_frame, const uint8_t *levels, int flags, int P,
                            const double *points, const uint8_t *point_colours, int radius, uint8_t *d_out, const char *who)
{
    ViewState &v = h->view;
    if (!points) P = 0;
    HM_ARG(X && d_frame && d_out, "%s: NULL state, frame or output", who);
    HM_ARG(((uintptr_t)d_out & 3) == 0, "%s: the output is not 4-byte aligned", who);
    HM_ARG(flags >= 0 && flags <= (CV_OUTLINE | CV_WIRE), "%s: flags %d outside 0..%d", who, flags, CV_OUTLINE | CV_WIRE);
    HM_ARG(P >= 0 && (P == 0 || point_colours), "%s: %d points without colours", who, P);
    HM_ARG(radius >= 0, "%s: point radius %d is negative", who, radius);
    if (v.c_layers == 0 && P == 0) {
        hm_set_error("%s: nothing to draw: hm_view_set_cells has set no cells and there are no points", who);
        return HM_ERR_STATE;
    }
    HM_HIP(hipSetDevice(h->device));
    const int n = h->W * h->H;
    const bool cells = v.c_layers > 0, wire = (flags & CV_WIRE) != 0;
    const int L = cells ? v.c_L : 0;
    // the frame's block: X | points | levels | point colours
    const size_t oX = 0, oP = (size_t)2 * h->N * sizeof(double), oL = oP + (size_t)2 * P * sizeof(double), oC = oL + (levels ? L : 0);
    const size_t bytes = oC + (size_t)3 * P;
    HM_HIP(h->own.event(&v.ev));
    if (wire) HM_HIP(h->own.alloc(&v.wire, (size_t)n * sizeof(unsigned)));
    const int s = v.c_next;
    HM_HIP(h->own.event(&v.c_slot_ev[s]));
    if (v.c_slot_used[s]) HM_HIP(hipEventSynchronize(v.c_slot_ev[s]));      // (the copy out of this slot has run)
    v.c_slot_used[s] = false;
    HM_HIP(h->own.host_grow(&v.c_slot[s], bytes, hipHostMallocDefault));
    {
        const auto it = h->own.mem.find(v.c_in);
        if (!v.c_in || it == h->own.mem.end() || it->second.bytes < bytes) {
            HM_HIP(hipStreamSynchronize(h->stream));      // (a view in flight reads the block that grows)
            HM_HIP(h->own.grow(&v.c_in, bytes));
        }
    }
    uint8_t *slot = v.c_slot[s];
    memcpy(slot + oX, X, oP);
    if (P) memcpy(slot + oP, points, (size_t)2 * P * sizeof(double));
    if (levels && L) memcpy(slot + oL, levels, (size_t)L);
    if (P) memcpy(slot + oC, point_colours, (size_t)3 * P);
    HM_HIP(hipMemcpyAsync(v.c_in, slot, bytes, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipEventRecord(v.c_slot_ev[s], h->stream));
    v.c_slot_used[s] = true;
    v.c_next = (s + 1) % VIEW_CELL_SLOTS;
    const double *dX = (const double *)(v.c_in + oX);
    if (wire) {
        HM_HIP(hipMemsetAsync(v.wire, 0, (size_t)n * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_view_wire, dim3(hm_cdiv(3 * h->T, 256 / VIEW_SEG_WAVE)), dim3(256), 0, h->stream,
                           (const int *)h->d_tri, h->T, dX, h->W, h->H, v.wire);
    }
    CellViewArgs a;
    a.W = h->W; a.H = h->H; a.T = cells ? h->T : 0; a.n_layers = v.c_layers; a.flags = flags;
    a.tiles_x = hm_cdiv(h->W, CV_W);
    a.tri = h->d_tri; a.uv = h->d_uv; a.X = dX; a.frame = d_frame;
    a.labels = v.c_lab; a.weights = v.c_weighted ? v.c_w : nullptr; a.colours = v.c_col;
    a.levels = levels ? v.c_in + oL : nullptr;
    a.outline = v.c_outline; a.wire = v.wire; a.out = d_out;
    hipLaunchKernelGGL(k_view_cells, dim3(a.tiles_x * hm_cdiv(h->H, CV_H)), dim3(256), 0, h->stream, a);
    if (P)
        hipLaunchKernelGGL(k_view_cell_marks, dim3(hm_cdiv(P, 256 / VIEW_SEG_WAVE)), dim3(256), 0, h->stream, h->W, h->H, P, radius,
                           (const double *)(v.c_in + oP), (const uint8_t *)(v.c_in + oC), d_out);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_view_cells(hm_ctx_t h, const double *X, const uint8_t *frame, const uint8_t *levels, int flags, int P,
                             const double *points, const uint8_t *point_colours, int point_radius, uint8_t *bgr)
{
    HM_ARG(h && frame && bgr, "hm_view_cells: NULL argument");
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->view.c_frame, n));
    HM_HIP(h->own.alloc(&h->view.out, 3 * n));
    HM_HIP(hipMemcpyAsync(h->view.c_frame, frame, n, hipMemcpyHostToDevice, h->stream));
    const int rc = view_cells_queue(h, X, h->view.c_frame, levels, flags, P, points, point_colours, point_radius, h->view.out,
                                    "hm_view_cells");
    if (rc) return rc;
    return view_download(h, bgr);
}

extern "C" int hm_view_cells_dev(hm_ctx_t h, const double *X, const void *d_frame, const uint8_t *levels, int flags, int P,
                                 const double *points, const uint8_t *point_colours, int point_radius, void *d_bgr, void *stream)
{
    HM_ARG(h != nullptr, "hm_view_cells_dev: NULL handle");
    HM_JOIN_LAZY(h);
    const int rc = view_cells_queue(h, X, (const uint8_t *)d_frame, levels, flags, P, points, point_colours, point_radius,
                                    (uint8_t *)d_bgr, "hm_view_cells_dev");
    if (rc) return rc;
    if (stream) {
        HM_HIP(hipEventRecord(h->view.ev, h->stream));
        HM_HIP(hipStreamWaitEvent((hipStream_t)stream, h->view.ev, 0));
    }
    return HM_OK;
}

// ---- the body-frame readout (body_kernels.h) --------------------------------------------------------------------
// The body map at X = uv (k_setup_all, then k_body_map), the pixels per triangle on the host.  Once per handle.
static int body_map_build(hm_ctx *h)
{
    HM_HIP(hipSetDevice(h->device));
    if (h->body.ready) return HM_OK;
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->body.setup, (size_t)h->T * sizeof(TriSetup)));
    HM_HIP(h->own.alloc(&h->body.uvX, (size_t)4 * h->N * sizeof(double)));
    HM_HIP(h->own.alloc(&h->body.X, (size_t)2 * h->N * sizeof(double)));
    HM_HIP(h->own.alloc(&h->body.tri, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->body.bary, n * sizeof(double2)));
    HM_HIP(h->own.alloc(&h->body.tidx, (size_t)h->T * sizeof(int4)));
    HM_HIP(h->own.alloc(&h->body.tcnt, (size_t)h->T * sizeof(unsigned)));
    HM_HIP(h->own.alloc(&h->body.sum, (size_t)(h->T + h->body.L) * sizeof(unsigned long long)));
    HM_HIP(h->own.event(&h->body.ev));
    Mesh m = {h->W, h->H, h->N, h->T, h->d_tri, h->d_uv, h->d_tex};
    hipLaunchKernelGGL(k_body_uvX, dim3(hm_cdiv(4 * h->N, 256)), dim3(256), 0, h->stream, (const float *)h->d_uv, h->N, h->body.uvX);
    ekf_queue_setup_all(h->stream, m, h->body.uvX, h->body.setup);
    HM_HIP(hipMemsetAsync(h->body.tcnt, 0, (size_t)h->T * sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(k_body_map, dim3(hm_cdiv(h->W, EKF_TILE), hm_cdiv(h->H, EKF_TILE)), dim3(EKF_TILE, EKF_TILE), 0, h->stream,
                       h->W, h->H, h->T, (const TriSetup *)h->body.setup, h->body.tri, h->body.bary, h->body.tidx, h->body.tcnt);
    HM_HIP(hipGetLastError());
    h->body.h_tcnt.resize(h->T);
    HM_HIP(hipMemcpyAsync(h->body.h_tcnt.data(), h->body.tcnt, (size_t)h->T * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    h->body.ready = true;
    return HM_OK;
}

extern "C" int hm_body_map(hm_ctx_t h, int32_t *tri_of_pixel, uint32_t *tri_counts)
{
    HM_ARG(h != nullptr, "hm_body_map: NULL handle");
    HM_JOIN_LAZY(h);                             // (body_map_build creates resources: the helper must not be queueing)
    int rc = body_map_build(h);
    if (rc) return rc;
    if (tri_of_pixel) {
        HM_HIP(hipMemcpyAsync(tri_of_pixel, h->body.tri, (size_t)h->W * h->H * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipStreamSynchronize(h->stream));
    }
    if (tri_counts) memcpy(tri_counts, h->body.h_tcnt.data(), (size_t)h->T * sizeof(uint32_t));
    return HM_OK;
}

extern "C" int hm_body_set_labels(hm_ctx_t h, const int32_t *labels, int L, uint32_t *counts)
{
    HM_ARG(labels == nullptr || L >= 1, "hm_body_set_labels: %d labels (need at least 1 with a label image)", L);
    HM_ARG(h != nullptr, "hm_body_set_labels: NULL handle");
    const size_t n = (size_t)h->W * h->H;
    if (labels) {
        for (size_t p = 0; p < n; p++)
            HM_ARG(labels[p] >= -1 && labels[p] < L, "hm_body_set_labels: label %d at pixel %zu outside -1..%d", (int)labels[p],
                   p, L - 1);
    }
    HM_JOIN_LAZY(h);
    int rc = body_map_build(h);
    if (rc) return rc;
    if (!labels) { h->body.L = 0; return HM_OK; }
    HM_HIP(h->own.alloc(&h->body.lab, n * sizeof(int)));
    HM_HIP(h->own.grow(&h->body.lcnt, (size_t)L * sizeof(unsigned)));
    HM_HIP(h->own.grow(&h->body.sum, (size_t)(h->T + L) * sizeof(unsigned long long)));
    h->body.L = 0;                               // (until the label image and its counts are in place)
    HM_HIP(hipMemcpyAsync(h->body.lab, labels, n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(h->body.lcnt, 0, (size_t)L * sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(k_body_label_count, dim3(hm_cdiv((int)n, 256)), dim3(256), 0, h->stream, (const int *)h->body.tri,
                       (const int *)h->body.lab, (int)n, h->body.lcnt);
    HM_HIP(hipGetLastError());
    if (counts) HM_HIP(hipMemcpyAsync(counts, h->body.lcnt, (size_t)L * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    h->body.L = L;
    return HM_OK;
}

// the planes of the sums start 16 bytes aligned (k_body_stats_add moves four values at a time)
static size_t body_stats_stride(const hm_ctx *h) { return ((size_t)h->W * h->H + 3) & ~(size_t)3; }
static BodyStats body_stats_planes(const hm_ctx *h)
{
    const size_t ns = body_stats_stride(h);
    return BodyStats{h->body.stsum, h->body.stsum + ns, h->body.stsum + 2 * ns, ns, h->body.stmax};
}

static int body_rec_slot(hm_ctx *h, const char *who, uint8_t **dst);

// Queue the warp of frame d_frame (device) at state X (host, the first 2N values are read) on the handle's stream.
static int body_queue(hm_ctx *h, const double *X, const uint8_t *d_frame, uint8_t *d_out, int ch, unsigned long long *d_tsum,
                      unsigned long long *d_lsum, const char *who)
{
    if (d_lsum && h->body.L == 0) { hm_set_error("%s: label sums asked for, and hm_body_set_labels has set no labels", who); return HM_ERR_STATE; }
    if (h->body.stats_on && h->body.stats_frames >= h->body.stats_cap) {
        hm_set_error("%s: the statistics hold %d frames, their capacity is %d (sums of 32 bits are exact up to %d frames): "
                     "nothing added", who, h->body.stats_frames, h->body.stats_cap, BODY_STATS_CAP);
        return HM_ERR_STATE;
    }
    uint8_t *rec_dst = nullptr;
    if (h->rec.on) {                 // (before anything is queued: a refused warp leaves statistics and record as they were)
        const int rc = body_rec_slot(h, who, &rec_dst);
        if (rc) return rc;
    }
    const int n = h->W * h->H;
    HM_HIP(hipMemcpyAsync(h->body.X, X, (size_t)2 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (d_tsum) HM_HIP(hipMemsetAsync(d_tsum, 0, (size_t)h->T * sizeof(unsigned long long), h->stream));
    if (d_lsum) HM_HIP(hipMemsetAsync(d_lsum, 0, (size_t)h->body.L * sizeof(unsigned long long), h->stream));
    BodyWarpArgs a;
    a.n = n; a.W = h->W; a.H = h->H; a.ch = ch;
    a.tri_of = h->body.tri; a.bary = h->body.bary; a.tidx = h->body.tidx;
    a.X = h->body.X; a.frame = d_frame; a.labels = h->body.lab;
    a.out = d_out; a.tsum = d_tsum; a.lsum = d_lsum;
    a.reg = h->body.stats_on || h->rec.on ? h->body.reg : nullptr;
    hipLaunchKernelGGL(k_body_warp, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    HM_HIP(hipEventRecord(h->body.ev, h->stream));
    if (h->body.stats_on) {               // (behind the event: whoever waits for the warp's output does not wait for this)
        const BodyStats st = body_stats_planes(h);
        hipLaunchKernelGGL(k_body_stats_add, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W,
                           (const int *)h->body.tri, (const uint8_t *)h->body.reg, st);
        HM_HIP(hipGetLastError());
        h->body.stats_frames++;
    }
    if (h->rec.on) {                 // (behind the event as well)
        const RecBox &b = h->rec.box;
        hipLaunchKernelGGL(k_rec_copy, dim3(hm_cdiv((b.pitch >> 2) * b.bh, 256)), dim3(256), 0, h->stream, h->W, b,
                           (const uint8_t *)h->body.reg, rec_dst);
        HM_HIP(hipGetLastError());
        h->rec.frames++;
    }
    return HM_OK;
}

extern "C" int hm_body_warp(hm_ctx_t h, const double *X, const uint8_t *frame, uint8_t *out, uint64_t *tri_sums,
                            uint64_t *label_sums)
{
    HM_ARG(X && frame, "hm_body_warp: NULL state or frame");
    HM_ARG(h != nullptr, "hm_body_warp: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_map_build(h);
    if (rc) return rc;
    if (label_sums && h->body.L == 0) { hm_set_error("hm_body_warp: label sums asked for, and hm_body_set_labels has set no labels"); return HM_ERR_STATE; }
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->body.frame, n));
    HM_HIP(h->own.alloc(&h->body.out, 3 * n));
    HM_HIP(hipMemcpyAsync(h->body.frame, frame, n, hipMemcpyHostToDevice, h->stream));
    unsigned long long *ts = h->body.sum, *ls = h->body.sum + h->T;
    rc = body_queue(h, X, h->body.frame, out ? h->body.out : nullptr, 1, tri_sums ? ts : nullptr, label_sums ? ls : nullptr,
                    "hm_body_warp");
    if (rc) return rc;
    if (out) HM_HIP(hipMemcpyAsync(out, h->body.out, n, hipMemcpyDeviceToHost, h->stream));
    if (tri_sums) HM_HIP(hipMemcpyAsync(tri_sums, ts, (size_t)h->T * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (label_sums) HM_HIP(hipMemcpyAsync(label_sums, ls, (size_t)h->body.L * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_warp_dev(hm_ctx_t h, const double *X, const void *d_frame, void *d_out, int out_channels,
                                void *d_tri_sums, void *d_label_sums, void *stream)
{
    HM_ARG(out_channels == 1 || out_channels == 3, "hm_body_warp_dev: out_channels %d (1 or 3)", out_channels);
    HM_ARG(X && d_frame, "hm_body_warp_dev: NULL state or frame");
    HM_ARG(((uintptr_t)d_out & 3) == 0, "hm_body_warp_dev: d_out is not 4-byte aligned");
    HM_ARG(((uintptr_t)d_tri_sums & 7) == 0 && ((uintptr_t)d_label_sums & 7) == 0,
           "hm_body_warp_dev: the sums are not 8-byte aligned");
    HM_ARG(h != nullptr, "hm_body_warp_dev: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_map_build(h);
    if (rc) return rc;
    rc = body_queue(h, X, (const uint8_t *)d_frame, (uint8_t *)d_out, out_channels, (unsigned long long *)d_tri_sums,
                    (unsigned long long *)d_label_sums, "hm_body_warp_dev");
    if (rc) return rc;
    if (stream) HM_HIP(hipStreamWaitEvent((hipStream_t)stream, h->body.ev, 0));
    return HM_OK;
}

extern "C" int hm_body_fence(hm_ctx_t h, void *stream)
{
    HM_ARG(h && stream, "hm_body_fence: NULL argument");
    if (h->body.ev) {
        HM_HIP(hipSetDevice(h->device));
        HM_HIP(hipStreamWaitEvent((hipStream_t)stream, h->body.ev, 0));
    }
    return HM_OK;
}

// ---- statistics of the registered video: sums per pixel, summary images, peaks (body_kernels.h) -------------------
extern "C" int hm_body_stats_begin(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_body_stats_begin: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_map_build(h);
    if (rc) return rc;
    const size_t n = (size_t)h->W * h->H;
    h->body.stats_on = false;                         // (until every buffer is there and zeroed)
    HM_HIP(h->own.alloc(&h->body.reg, n));
    const size_t ns = body_stats_stride(h);
    HM_HIP(h->own.alloc(&h->body.stsum, 6 * ns * sizeof(unsigned)));
    HM_HIP(h->own.alloc(&h->body.stmax, n));
    HM_HIP(hipMemsetAsync(h->body.stsum, 0, 6 * ns * sizeof(unsigned), h->stream));
    HM_HIP(hipMemsetAsync(h->body.stmax, 0, n, h->stream));
    h->body.stats_frames = 0;
    h->body.stats_on = true;
    return HM_OK;
}

extern "C" int hm_body_stats_end(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_body_stats_end: NULL handle");
    HM_JOIN_LAZY(h);
    h->body.stats_on = false;
    h->body.stats_frames = 0;
    if (!h->body.stsum) return HM_OK;
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipStreamSynchronize(h->stream));
    hipError_t e = h->rec.on ? hipSuccess : h->own.free(&h->body.reg);     // (the record's copy reads the same plane)
    if (e == hipSuccess) e = h->own.free(&h->body.stsum);
    if (e == hipSuccess) e = h->own.free(&h->body.stmax);
    if (e == hipSuccess) e = h->own.free(&h->body.stimg);
    if (e == hipSuccess) e = h->own.free(&h->body.pkidx);
    if (e == hipSuccess) e = h->own.free(&h->body.pkscore);
    if (e == hipSuccess) e = h->own.free(&h->body.pkcnt);
    HM_HIP(e);
    return HM_OK;
}

extern "C" int hm_body_stats_count(hm_ctx_t h, int *frames)
{
    HM_ARG(h && frames, "hm_body_stats_count: NULL argument");
    HM_JOIN_LAZY(h);
    *frames = h->body.stats_on ? h->body.stats_frames : 0;
    return HM_OK;
}

static int body_stats_begun(hm_ctx *h, bool need_frames, const char *who)
{
    if (!h->body.stats_on) { hm_set_error("%s: no statistics (hm_body_stats_begin first)", who); return HM_ERR_STATE; }
    if (need_frames && h->body.stats_frames < 1) { hm_set_error("%s: no frame added since hm_body_stats_begin", who); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    return HM_OK;
}

extern "C" int hm_body_stats_fetch(hm_ctx_t h, uint32_t *s1, uint32_t *s2, uint32_t *cross, uint8_t *vmax)
{
    HM_ARG(h != nullptr, "hm_body_stats_fetch: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_stats_begun(h, false, "hm_body_stats_fetch");
    if (rc) return rc;
    const size_t n = (size_t)h->W * h->H, b = n * sizeof(uint32_t);
    const BodyStats st = body_stats_planes(h);
    if (s1) HM_HIP(hipMemcpyAsync(s1, st.s1, b, hipMemcpyDeviceToHost, h->stream));
    if (s2) HM_HIP(hipMemcpyAsync(s2, st.s2, b, hipMemcpyDeviceToHost, h->stream));
    for (int d = 0; cross && d < 4; d++)
        HM_HIP(hipMemcpyAsync(cross + d * n, st.cross + d * st.stride, b, hipMemcpyDeviceToHost, h->stream));
    if (vmax) HM_HIP(hipMemcpyAsync(vmax, h->body.stmax, n, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// the three summary images of the sums so far into body.stimg, queued on the handle's stream
static int body_stats_images_queue(hm_ctx *h)
{
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->body.stimg, 3 * n * sizeof(double)));
    BodyImages g;
    g.n = (int)n; g.W = h->W; g.H = h->H; g.F = (double)h->body.stats_frames;
    g.tri_of = h->body.tri;
    g.st = body_stats_planes(h);
    g.mean = h->body.stimg; g.sd = h->body.stimg + n; g.corr = h->body.stimg + 2 * n;
    hipLaunchKernelGGL(k_body_stats_images, dim3(hm_cdiv((int)n, 256)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_body_stats_images(hm_ctx_t h, double *mean, double *std, double *corr, uint8_t *vmax)
{
    HM_ARG(h != nullptr, "hm_body_stats_images: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_stats_begun(h, true, "hm_body_stats_images");
    if (rc) return rc;
    rc = body_stats_images_queue(h);
    if (rc) return rc;
    const size_t n = (size_t)h->W * h->H, b = n * sizeof(double);
    if (mean) HM_HIP(hipMemcpyAsync(mean, h->body.stimg, b, hipMemcpyDeviceToHost, h->stream));
    if (std) HM_HIP(hipMemcpyAsync(std, h->body.stimg + n, b, hipMemcpyDeviceToHost, h->stream));
    if (corr) HM_HIP(hipMemcpyAsync(corr, h->body.stimg + 2 * n, b, hipMemcpyDeviceToHost, h->stream));
    if (vmax) HM_HIP(hipMemcpyAsync(vmax, h->body.stmax, n, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_stats_peaks(hm_ctx_t h, int which, int radius, double min_score, int cap, int32_t *index,
                                   double *score, int *count)
{
    HM_ARG(which >= 0 && which <= 2, "hm_body_stats_peaks: score %d (0 corr, 1 std, 2 max - mean)", which);
    HM_ARG(radius >= 1 && radius <= BODY_PEAK_RMAX, "hm_body_stats_peaks: radius %d outside 1..%d", radius, BODY_PEAK_RMAX);
    HM_ARG(!(min_score != min_score), "hm_body_stats_peaks: min_score is NaN");
    HM_ARG(cap >= 0 && (cap == 0 || (index && score)), "hm_body_stats_peaks: cap %d without arrays to fill", cap);
    HM_ARG(h && count, "hm_body_stats_peaks: NULL argument");
    HM_JOIN_LAZY(h);
    int rc = body_stats_begun(h, true, "hm_body_stats_peaks");
    if (rc) return rc;
    rc = body_stats_images_queue(h);
    if (rc) return rc;
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->body.pkidx, n * sizeof(int)));
    HM_HIP(h->own.alloc(&h->body.pkscore, n * sizeof(double)));
    HM_HIP(h->own.alloc(&h->body.pkcnt, sizeof(int)));
    HM_HIP(hipMemsetAsync(h->body.pkcnt, 0, sizeof(int), h->stream));
    BodyPeaks g;
    g.W = h->W; g.H = h->H; g.which = which; g.radius = radius; g.cap = (int)n; g.min_score = min_score;
    g.tri_of = h->body.tri;
    g.mean = h->body.stimg; g.sd = h->body.stimg + n; g.corr = h->body.stimg + 2 * n; g.vmax = h->body.stmax;
    g.count = h->body.pkcnt; g.index = h->body.pkidx; g.score = h->body.pkscore;
    hipLaunchKernelGGL(k_body_peaks, dim3(hm_cdiv(h->W, BODY_PEAK_TILE), hm_cdiv(h->H, BODY_PEAK_TILE)),
                       dim3(BODY_PEAK_TILE, BODY_PEAK_TILE), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    int found = 0;
    HM_HIP(hipMemcpyAsync(&found, h->body.pkcnt, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    if (found < 0 || (size_t)found > n) { hm_set_error("hm_body_stats_peaks: %d peaks reported for %zu pixels", found, n); return HM_ERR_HIP; }
    std::vector<int> idx(found);
    std::vector<double> sc(found);
    if (found) {
        HM_HIP(hipMemcpyAsync(idx.data(), h->body.pkidx, (size_t)found * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipMemcpyAsync(sc.data(), h->body.pkscore, (size_t)found * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipStreamSynchronize(h->stream));
    }
    // the waves arrive in any order: score descending, raster index ascending
    std::vector<int> order(found);
    for (int i = 0; i < found; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return sc[a] != sc[b] ? sc[a] > sc[b] : idx[a] < idx[b]; });
    for (int i = 0; i < found && i < cap; i++) {
        index[i] = idx[order[i]];
        score[i] = sc[order[i]];
    }
    *count = found;
    return HM_OK;
}

// ---- the registered video kept on the device, and the reductions over it (roi_kernels.h) ---------------------------
#define REC_CHUNK_BYTES ((size_t)64 << 20)
#define REC_MAX_FRAMES (1 << 24)

// stop recording and free the record (the caller has checked that there is one)
static int body_rec_drop(hm_ctx *h)
{
    h->rec.on = false;
    h->rec.frames = 0;
    HM_HIP(hipSetDevice(h->device));
    HM_HIP(hipStreamSynchronize(h->stream));
    hipError_t e = hipSuccess;
    for (uint8_t *&c : h->rec.chunks) {
        const hipError_t e1 = h->own.free(&c);
        if (e == hipSuccess) e = e1;
    }
    h->rec.chunks.clear();
    if (e == hipSuccess) e = h->own.free(&h->rec.tab);
    if (e == hipSuccess) e = h->own.free(&h->rec.tmp);
    if (e == hipSuccess) e = h->own.free(&h->rec.scr);
    if (e == hipSuccess && !h->body.stats_on) e = h->own.free(&h->body.reg);
    HM_HIP(e);
    return HM_OK;
}

extern "C" int hm_body_rec_begin(hm_ctx_t h, uint64_t max_bytes)
{
    HM_ARG(h != nullptr, "hm_body_rec_begin: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_map_build(h);
    if (rc) return rc;
    if (h->rec.on) {
        rc = body_rec_drop(h);
        if (rc) return rc;
    }
    const size_t n = (size_t)h->W * h->H;
    if (h->body.h_tri.empty()) {
        h->body.h_tri.resize(n);
        HM_HIP(hipMemcpyAsync(h->body.h_tri.data(), h->body.tri, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HM_HIP(hipStreamSynchronize(h->stream));
    }
    int c0 = h->W, c1 = -1, r0 = h->H, r1 = -1;
    for (int r = 0; r < h->H; r++)
        for (int c = 0; c < h->W; c++)
            if (h->body.h_tri[(size_t)r * h->W + c] >= 0) {
                c0 = std::min(c0, c); c1 = std::max(c1, c);
                r0 = std::min(r0, r); r1 = std::max(r1, r);
            }
    if (c1 < 0) c0 = c1 = r0 = r1 = 0;          // (an empty map: one pixel, registered as 0)
    RecBox &b = h->rec.box;
    b.c0 = c0; b.r0 = r0; b.bw = c1 - c0 + 1; b.bh = r1 - r0 + 1;
    b.pitch = (b.bw + 3) & ~3;
    b.fs = ((size_t)b.pitch * b.bh + 15) & ~(size_t)15;
    b.fpc = h->rec.chunk > 0 ? h->rec.chunk : (int)std::max<size_t>(1, REC_CHUNK_BYTES / b.fs);
    h->rec.max = max_bytes;
    h->rec.cap = (int)std::min<unsigned long long>(max_bytes / b.fs, REC_MAX_FRAMES);
    HM_HIP(h->own.alloc(&h->body.reg, n));
    h->rec.frames = 0;
    h->rec.on = true;
    return HM_OK;
}

extern "C" int hm_body_rec_end(hm_ctx_t h)
{
    HM_ARG(h != nullptr, "hm_body_rec_end: NULL handle");
    HM_JOIN_LAZY(h);
    if (!h->rec.on) return HM_OK;
    return body_rec_drop(h);
}

extern "C" int hm_body_rec_count(hm_ctx_t h, int *frames)
{
    HM_ARG(h && frames, "hm_body_rec_count: NULL argument");
    HM_JOIN_LAZY(h);
    *frames = h->rec.on ? h->rec.frames : 0;
    return HM_OK;
}

// where the next frame of the record goes; allocates the chunk it starts
static int body_rec_slot(hm_ctx *h, const char *who, uint8_t **dst)
{
    const RecBox &b = h->rec.box;
    if (h->rec.frames >= h->rec.cap) {
        hm_set_error("%s: the record holds %d frames of %zu bytes (a box of %d x %d pixels) and its budget of %llu bytes holds "
                     "%d: nothing appended", who, h->rec.frames, b.fs, b.bw, b.bh, h->rec.max, h->rec.cap);
        return HM_ERR_STATE;
    }
    const int ch = h->rec.frames / b.fpc;
    if (ch == (int)h->rec.chunks.size()) {
        const int frames = std::min(b.fpc, h->rec.cap - ch * b.fpc);
        uint8_t *p = nullptr;
        HM_HIP(h->own.alloc(&p, (size_t)frames * b.fs));
        h->rec.chunks.push_back(p);
    }
    *dst = h->rec.chunks[ch] + (size_t)(h->rec.frames - ch * b.fpc) * b.fs;
    return HM_OK;
}

static int body_rec_begun(hm_ctx *h, const char *who)
{
    if (!h->rec.on) { hm_set_error("%s: no record (hm_body_rec_begin first)", who); return HM_ERR_STATE; }
    HM_HIP(hipSetDevice(h->device));
    return HM_OK;
}

extern "C" int hm_body_rec_fetch(hm_ctx_t h, int k0, int n, uint8_t *out)
{
    HM_ARG(h != nullptr, "hm_body_rec_fetch: NULL handle");
    HM_JOIN_LAZY(h);
    int rc = body_rec_begun(h, "hm_body_rec_fetch");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n >= 0 && k0 <= h->rec.frames && n <= h->rec.frames - k0,
           "hm_body_rec_fetch: frames %d .. %d of a record of %d", k0, k0 + n - 1, h->rec.frames);
    HM_ARG(out || n == 0, "hm_body_rec_fetch: NULL output");
    HM_HIP(hipStreamSynchronize(h->stream));
    const RecBox &b = h->rec.box;
    const size_t px = (size_t)h->W * h->H;
    for (int k = 0; k < n; k++) {
        uint8_t *o = out + (size_t)k * px;
        memset(o, 0, px);
        const int ch = (k0 + k) / b.fpc;
        const uint8_t *src = h->rec.chunks[ch] + (size_t)(k0 + k - ch * b.fpc) * b.fs;
        HM_HIP(hipMemcpy2D(o + (size_t)b.r0 * h->W + b.c0, (size_t)h->W, src, (size_t)b.pitch, (size_t)b.bw, (size_t)b.bh,
                           hipMemcpyDeviceToHost));
    }
    return HM_OK;
}

// a reduction may start: there are frames, and the chunks' addresses are on the device
static int body_rec_ready(hm_ctx *h, const char *who)
{
    const int rc = body_rec_begun(h, who);
    if (rc) return rc;
    if (h->rec.frames < 1) { hm_set_error("%s: no frame recorded since hm_body_rec_begin", who); return HM_ERR_STATE; }
    const size_t bytes = h->rec.chunks.size() * sizeof(uint8_t *);
    HM_HIP(h->own.grow(&h->rec.tab, bytes));       // (every reduction waits for its results: nothing in flight reads it)
    HM_HIP(hipMemcpyAsync(h->rec.tab, h->rec.chunks.data(), bytes, hipMemcpyHostToDevice, h->stream));
    return HM_OK;
}

// the reductions' buffers, carved from one allocation (16-byte aligned pieces)
struct RecCarve {
    uint8_t *base;
    size_t off;
    template <typename T> T *take(size_t count)
    {
        off = (off + 15) & ~(size_t)15;
        T *p = (T *)(base + off);
        off += count * sizeof(T);
        return p;
    }
};
// Lay a reduction's buffers out in rec.tmp: `lay` takes its pieces from the RecCarve it is given, first to measure them,
// then, once the allocation holds them all, for their addresses.
template <typename Lay>
static int body_rec_carve(hm_ctx *h, Lay lay)
{
    RecCarve cv = {nullptr, 0};
    lay(cv);
    HM_HIP(h->own.grow(&h->rec.tmp, cv.off));
    cv = {h->rec.tmp, 0};
    lay(cv);
    return HM_OK;
}

extern "C" int hm_body_rec_label_sums(hm_ctx_t h, const int32_t *labels, int L, uint64_t *out)
{
    HM_ARG(labels && out && L >= 1, "hm_body_rec_label_sums: NULL argument or %d labels", L);
    HM_ARG(h != nullptr, "hm_body_rec_label_sums: NULL handle");
    const size_t n = (size_t)h->W * h->H;
    for (size_t p = 0; p < n; p++)
        HM_ARG(labels[p] >= -1 && labels[p] < L, "hm_body_rec_label_sums: label %d at pixel %zu outside -1..%d", (int)labels[p],
               p, L - 1);
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_label_sums");
    if (rc) return rc;
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames, nb = b.pitch * b.bh;
    int *d_img = nullptr, *d_lab = nullptr;
    unsigned long long *d_sum = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_img = cv.take<int>(n);
        d_lab = cv.take<int>(nb);
        d_sum = cv.take<unsigned long long>((size_t)F * L);
    });
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(d_img, labels, n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(d_sum, 0, (size_t)F * L * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_rec_box_labels, dim3(hm_cdiv(nb, 256)), dim3(256), 0, h->stream, h->W, b, (const int *)h->body.tri,
                       (const int *)d_img, d_lab);
    hipLaunchKernelGGL(k_rec_label_sums, dim3(hm_cdiv(nb >> 2, 256), std::min(F, 1024)), dim3(256), 0, h->stream, b,
                       (const uint8_t *const *)h->rec.tab, F, (const int *)d_lab, L, d_sum);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, d_sum, (size_t)F * L * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// What the reductions over seeds open with, in this order: the helper joined, a record with frames whose chunk table is on
// the device (body_rec_ready), every seed a pixel of the map, and F P below 2^30 (the kernels index frame x seed in an int).
static int body_rec_seeded(hm_ctx *h, int P, const int32_t *seeds, const char *who)
{
    HM_JOIN_LAZY(h);
    const int rc = body_rec_ready(h, who);
    if (rc) return rc;
    for (int s = 0; s < P; s++) {
        const int c = seeds[2 * s], r = seeds[2 * s + 1];
        if (!(c >= 0 && c < h->W && r >= 0 && r < h->H && h->body.h_tri[(size_t)r * h->W + c] >= 0)) {
            hm_set_error("%s: seed %d (column %d, row %d) is not a pixel of the body map", who, s, c, r);
            return HM_ERR_ARG;
        }
    }
    HM_ARG((long long)h->rec.frames * P < (1ll << 30), "%s: %d frames x %d seeds", who, h->rec.frames, P);
    return HM_OK;
}

extern "C" int hm_body_rec_seed_sums(hm_ctx_t h, int P, const int32_t *seeds, double r_disc, double r_in, double r_out, int R,
                                     uint32_t *n_T, uint32_t *n_G, uint64_t *T, uint64_t *G, int64_t *U, uint64_t *w1,
                                     uint64_t *w2, int64_t *c, int64_t *u1, int64_t *u2)
{
    HM_ARG(P >= 1 && seeds, "hm_body_rec_seed_sums: %d seeds", P);
    HM_ARG(r_disc >= 0.0 && r_disc <= REC_RMAX && r_in >= 0.0 && r_in <= r_out && r_out <= REC_RMAX,
           "hm_body_rec_seed_sums: radii %g, %g, %g (need 0 <= r_disc <= %d and 0 <= r_in <= r_out <= %d)", r_disc, r_in, r_out,
           REC_RMAX, REC_RMAX);
    HM_ARG(R >= 0 && R <= REC_WIN_RMAX, "hm_body_rec_seed_sums: window radius %d outside 0..%d", R, REC_WIN_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_seed_sums: NULL handle");
    int rc = body_rec_seeded(h, P, seeds, "hm_body_rec_seed_sums");
    if (rc) return rc;
    const int F = h->rec.frames;
    // the pixels of every disc and ring, and the bound that keeps sum U^2 exact: |U| <= 255 n_T n_G
    const double rd2 = r_disc * r_disc, ri2 = r_in * r_in, ro2 = r_out * r_out;
    const int Rg = (int)std::max(r_disc, r_out);
    std::vector<unsigned> cnt(2 * (size_t)P, 0);
    for (int s = 0; s < P; s++) {
        for (int dy = -Rg; dy <= Rg; dy++)
            for (int dx = -Rg; dx <= Rg; dx++) {
                const int x = seeds[2 * s] + dx, y = seeds[2 * s + 1] + dy;
                if (x < 0 || x >= h->W || y < 0 || y >= h->H || h->body.h_tri[(size_t)y * h->W + x] < 0) continue;
                const double d2 = (double)(dx * dx + dy * dy);
                if (d2 <= rd2) cnt[s]++;
                if (d2 >= ri2 && d2 <= ro2) cnt[P + s]++;
            }
        const unsigned __int128 m = (unsigned __int128)255 * cnt[s] * cnt[P + s];
        HM_ARG(m * m * (unsigned __int128)F < ((unsigned __int128)1 << 63),
               "hm_body_rec_seed_sums: seed %d: F (255 n_T n_G)^2 = %d (255 x %u x %u)^2 could pass 2^63", s, F, cnt[s], cnt[P + s]);
    }
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    RecSeeds g;
    RecWin q;
    int2 *d_seeds = nullptr;
    unsigned *d_cnt = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_cnt = cv.take<unsigned>(2 * (size_t)P);
        g.T = cv.take<unsigned long long>(fp);
        g.G = cv.take<unsigned long long>(fp);
        g.U = cv.take<long long>(fp);
        q.w1 = cv.take<unsigned long long>(P * nw);
        q.w2 = cv.take<unsigned long long>(P * nw);
        q.c = cv.take<long long>(P * nw);
        q.u1 = cv.take<long long>(P);
        q.u2 = cv.take<long long>(P);
    });
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_cnt, cnt.data(), 2 * (size_t)P * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.P = P; g.R = Rg;
    g.seeds = d_seeds; g.rd2 = rd2; g.ri2 = ri2; g.ro2 = ro2; g.nT = d_cnt; g.nG = d_cnt + P;
    hipLaunchKernelGGL(k_rec_seed_traces, dim3(hm_cdiv((int)fp, 4)), dim3(256), 0, h->stream, g);
    q.b = h->rec.box; q.chunks = g.chunks; q.F = F; q.P = P; q.R = R; q.seeds = d_seeds; q.U = g.U;
    hipLaunchKernelGGL(k_rec_window_sums, dim3(hm_cdiv((int)nw, 256), P), dim3(256), 0, h->stream, q);
    HM_HIP(hipGetLastError());
    if (n_T) memcpy(n_T, cnt.data(), (size_t)P * sizeof(uint32_t));
    if (n_G) memcpy(n_G, cnt.data() + P, (size_t)P * sizeof(uint32_t));
    if (T) HM_HIP(hipMemcpyAsync(T, g.T, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (G) HM_HIP(hipMemcpyAsync(G, g.G, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (U) HM_HIP(hipMemcpyAsync(U, g.U, fp * 8, hipMemcpyDeviceToHost, h->stream));
    if (w1) HM_HIP(hipMemcpyAsync(w1, q.w1, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (w2) HM_HIP(hipMemcpyAsync(w2, q.w2, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (c) HM_HIP(hipMemcpyAsync(c, q.c, P * nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (u1) HM_HIP(hipMemcpyAsync(u1, q.u1, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
    if (u2) HM_HIP(hipMemcpyAsync(u2, q.u2, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_weighted_sums(hm_ctx_t h, int P, const int32_t *seeds, int R, const uint16_t *weights, uint64_t *out)
{
    HM_ARG(P >= 1 && seeds && weights && out, "hm_body_rec_weighted_sums: NULL argument or %d seeds", P);
    HM_ARG(R >= 0 && R <= REC_RMAX, "hm_body_rec_weighted_sums: window radius %d outside 0..%d", R, REC_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_weighted_sums: NULL handle");
    int rc = body_rec_seeded(h, P, seeds, "hm_body_rec_weighted_sums");
    if (rc) return rc;
    const int F = h->rec.frames;
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    int2 *d_seeds = nullptr;
    uint16_t *d_w = nullptr;
    unsigned long long *d_out = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_w = cv.take<uint16_t>(P * nw);
        d_out = cv.take<unsigned long long>(fp);
    });
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_w, weights, P * nw * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_rec_weighted_sums, dim3(hm_cdiv((int)fp, 4)), dim3(256), 0, h->stream, h->rec.box,
                       (const uint8_t *const *)h->rec.tab, F, P, R, (const int2 *)d_seeds, (const uint16_t *)d_w, d_out);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, d_out, fp * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_trace_products(hm_ctx_t h, int P, const int32_t *seeds, int R, const int32_t *q, int64_t *out)
{
    HM_ARG(P >= 1 && seeds && q && out, "hm_body_rec_trace_products: NULL argument or %d seeds", P);
    HM_ARG(R >= 0 && R <= REC_WIN_RMAX, "hm_body_rec_trace_products: window radius %d outside 0..%d", R, REC_WIN_RMAX);
    HM_ARG(h != nullptr, "hm_body_rec_trace_products: NULL handle");
    int rc = body_rec_seeded(h, P, seeds, "hm_body_rec_trace_products");
    if (rc) return rc;
    const int F = h->rec.frames;
    // |v q| <= 255 x 2^31 per frame
    HM_ARG((unsigned __int128)F * 255u * ((unsigned __int128)1 << 31) < ((unsigned __int128)1 << 63),
           "hm_body_rec_trace_products: F x 255 x 2^31 = %d x 255 x 2^31 could pass 2^63", F);
    const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1), fp = (size_t)F * P;
    const int tiles = hm_cdiv((int)nw, 64);
    HM_ARG((long long)P * tiles < (1ll << 31), "hm_body_rec_trace_products: %d seeds x %d tiles of the window", P, tiles);
    RecTP g;
    int2 *d_seeds = nullptr;
    int *d_q = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_seeds = cv.take<int2>(P);
        d_q = cv.take<int>(fp);
        g.out = cv.take<unsigned long long>(P * nw);
    });
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_q, q, fp * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, P * nw * sizeof(unsigned long long), h->stream));
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = F; g.P = P; g.R = R;
    g.tpf = h->rec.tp_frames; g.seeds = d_seeds; g.q = d_q;
    const int runs = hm_cdiv(F, g.tpf);
    hipLaunchKernelGGL(k_rec_trace_products, dim3(P * tiles, std::min(runs, 65535)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, P * nw * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// ---- residual motion of the record: patch sums, sums at given shifts, the shift in place, the smooth field (stab_kernels.h)
#define STAB_SCRATCH_BYTES ((size_t)16 << 20)

// the core of every patch on the host: core[y * pitch + x] = 1 where every box pixel within S of (x, y) is in the map
// (two passes of prefix sums: rows, then columns); n_core: per patch
static void stab_core(const hm_ctx *h, int B, int S, std::vector<uint8_t> &core, std::vector<uint32_t> &n_core)
{
    const RecBox &b = h->rec.box;
    const int npx = hm_cdiv(b.bw, B), npy = hm_cdiv(b.bh, B), n1 = 2 * S + 1;
    core.assign((size_t)b.pitch * b.bh, 0);
    n_core.assign((size_t)npx * npy, 0);
    std::vector<uint8_t> hor((size_t)b.bw * b.bh, 0);
    std::vector<int> pre((size_t)std::max(b.bw, b.bh) + 1);
    for (int y = 0; y < b.bh; y++) {
        pre[0] = 0;
        for (int x = 0; x < b.bw; x++) pre[x + 1] = pre[x] + (h->body.h_tri[(size_t)(b.r0 + y) * h->W + b.c0 + x] >= 0);
        for (int x = S; x + S < b.bw; x++) hor[(size_t)y * b.bw + x] = pre[x + S + 1] - pre[x - S] == n1;
    }
    for (int x = 0; x < b.bw; x++) {
        pre[0] = 0;
        for (int y = 0; y < b.bh; y++) pre[y + 1] = pre[y] + hor[(size_t)y * b.bw + x];
        for (int y = S; y + S < b.bh; y++)
            if (pre[y + S + 1] - pre[y - S] == n1) {
                core[(size_t)y * b.pitch + x] = 1;
                n_core[(size_t)(y / B) * npx + x / B]++;
            }
    }
}

extern "C" int hm_body_rec_match(hm_ctx_t h, int k0, int n_frames, int B, int S, const uint8_t *tmpl, uint32_t *n_core,
                                 uint32_t *A, uint32_t *V1, uint32_t *V2)
{
    HM_ARG(B >= STAB_BMIN && B <= STAB_BMAX, "hm_body_rec_match: patch size %d outside %d..%d", B, STAB_BMIN, STAB_BMAX);
    HM_ARG(S >= 0 && S <= STAB_SMAX, "hm_body_rec_match: search radius %d outside 0..%d", S, STAB_SMAX);
    HM_ARG(h && tmpl, "hm_body_rec_match: NULL handle or template");
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_match");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n_frames >= 0 && k0 <= h->rec.frames && n_frames <= h->rec.frames - k0,
           "hm_body_rec_match: frames %d .. %d of a record of %d", k0, k0 + n_frames - 1, h->rec.frames);
    const RecBox &b = h->rec.box;
    const int npx = hm_cdiv(b.bw, B), np = npx * hm_cdiv(b.bh, B), nsh = (2 * S + 1) * (2 * S + 1);
    std::vector<uint8_t> core;
    std::vector<uint32_t> cnt;
    stab_core(h, B, S, core, cnt);
    if (n_core) memcpy(n_core, cnt.data(), (size_t)np * sizeof(uint32_t));
    if (n_frames == 0 || !(A || V1 || V2)) {
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const size_t n = (size_t)h->W * h->H, no = (size_t)n_frames * np * nsh;
    StabMatch g;
    uint8_t *d_tmpl = nullptr, *d_core = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_tmpl = cv.take<uint8_t>(n);
        d_core = cv.take<uint8_t>(core.size());
        g.A = A ? cv.take<unsigned>(no) : nullptr;
        g.V1 = V1 ? cv.take<unsigned>(no) : nullptr;
        g.V2 = V2 ? cv.take<unsigned>(no) : nullptr;
    });
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(d_tmpl, tmpl, n, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_core, core.data(), core.size(), hipMemcpyHostToDevice, h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames; g.tpf = h->rec.tp_frames;
    g.B = B; g.S = S; g.npx = npx; g.np = np; g.tmpl = d_tmpl; g.core = d_core;
    const int runs = hm_cdiv(n_frames, g.tpf);
    hipLaunchKernelGGL(k_stab_match, dim3(np, std::min(runs, 65535)), dim3(256), stab_lds_bytes(B, S), h->stream, g);
    HM_HIP(hipGetLastError());
    if (A) HM_HIP(hipMemcpyAsync(A, g.A, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (V1) HM_HIP(hipMemcpyAsync(V1, g.V1, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (V2) HM_HIP(hipMemcpyAsync(V2, g.V2, no * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

// every shift of `count` (dx, dy) pairs within +-STAB_DMAX
static int stab_shifts_ok(const int8_t *shifts, size_t count, int np, const char *who)
{
    for (size_t i = 0; i < 2 * count; i++)
        HM_ARG(shifts[i] >= -STAB_DMAX && shifts[i] <= STAB_DMAX, "%s: shift %d (%s of patch %zu, frame %zu of those given) outside -%d..%d",
               who, (int)shifts[i], i & 1 ? "dy" : "dx", (i / 2) % (size_t)np, (i / 2) / (size_t)np, STAB_DMAX, STAB_DMAX);
    return HM_OK;
}

extern "C" int hm_body_rec_frame_sums(hm_ctx_t h, int k0, int n_frames, int B, const int8_t *shifts, uint32_t *out)
{
    HM_ARG(!shifts || (B >= STAB_BMIN && B <= STAB_BMAX), "hm_body_rec_frame_sums: patch size %d outside %d..%d", B, STAB_BMIN,
           STAB_BMAX);
    HM_ARG((long long)n_frames * 255 < (1ll << 32), "hm_body_rec_frame_sums: %d frames x 255 could pass 2^32", n_frames);
    HM_ARG(h && out, "hm_body_rec_frame_sums: NULL handle or output");
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_frame_sums");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n_frames >= 0 && k0 <= h->rec.frames && n_frames <= h->rec.frames - k0,
           "hm_body_rec_frame_sums: frames %d .. %d of a record of %d", k0, k0 + n_frames - 1, h->rec.frames);
    const RecBox &b = h->rec.box;
    StabSum g;
    g.B = shifts ? B : 1;
    g.npx = hm_cdiv(b.bw, g.B); g.np = g.npx * hm_cdiv(b.bh, g.B);
    const size_t n = (size_t)h->W * h->H, ns = shifts ? (size_t)n_frames * g.np : 0;
    if (shifts) {
        rc = stab_shifts_ok(shifts, ns, g.np, "hm_body_rec_frame_sums");
        if (rc) return rc;
    }
    int8_t *d_sh = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        g.out = cv.take<unsigned>(n);
        d_sh = cv.take<int8_t>(2 * ns);
    });
    if (rc) return rc;
    if (ns) HM_HIP(hipMemcpyAsync(d_sh, shifts, 2 * ns, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, n * sizeof(unsigned), h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames;
    g.tri_of = h->body.tri; g.shifts = ns ? d_sh : nullptr;
    hipLaunchKernelGGL(k_stab_frame_sums, dim3(hm_cdiv(b.bw * b.bh, 256)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_shift(hm_ctx_t h, int B, const int8_t *shifts)
{
    HM_ARG(B >= STAB_BMIN && B <= STAB_BMAX, "hm_body_rec_shift: patch size %d outside %d..%d", B, STAB_BMIN, STAB_BMAX);
    HM_ARG(h && shifts, "hm_body_rec_shift: NULL handle or shifts");
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_shift");
    if (rc) return rc;
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    StabShift g;
    g.b = b; g.W = h->W; g.B = B; g.npx = hm_cdiv(b.bw, B); g.np = g.npx * hm_cdiv(b.bh, B); g.tri_of = h->body.tri;
    const size_t ns = (size_t)F * g.np;
    rc = stab_shifts_ok(shifts, ns, g.np, "hm_body_rec_shift");
    if (rc) return rc;
    int8_t *d_sh = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) { d_sh = cv.take<int8_t>(2 * ns); });
    if (rc) return rc;
    // runs of frames within a chunk: copied aside as they are, then gathered back into the record
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(b.fpc, F), STAB_SCRATCH_BYTES / b.fs));
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        HM_HIP(hipMemcpyAsync(d_sh, shifts, 2 * ns, hipMemcpyHostToDevice, h->stream));
        const int blocks = hm_cdiv((b.pitch >> 2) * b.bh, 256);
        for (int k = 0; k < F;) {
            const int ch = k / b.fpc, m = std::min(per, std::min(F, (ch + 1) * b.fpc) - k);
            uint8_t *dst = h->rec.chunks[ch] + (size_t)(k - ch * b.fpc) * b.fs;
            HM_HIP(hipMemcpyAsync(h->rec.scr, dst, (size_t)m * b.fs, hipMemcpyDeviceToDevice, h->stream));
            g.frames = m; g.shifts = d_sh + 2 * (size_t)k * g.np; g.src = h->rec.scr; g.dst = dst;
            hipLaunchKernelGGL(k_stab_shift, dim3(blocks, std::min(m, 65535)), dim3(256), 0, h->stream, g);
            HM_HIP(hipGetLastError());
            k += m;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    };
    rc = run();
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

// every q of `count` (dx, dy) pairs within +-STAB_QMAX; packed with its validity for the device
static int stab_field_pack(const int16_t *q, const uint8_t *valid, size_t count, int np, const char *who, std::vector<unsigned> &qv)
{
    qv.resize(count);
    for (size_t i = 0; i < count; i++) {
        for (int c = 0; c < 2; c++)
            HM_ARG(q[2 * i + c] >= -STAB_QMAX && q[2 * i + c] <= STAB_QMAX,
                   "%s: q %d (%s of patch %zu, frame %zu of those given) outside -%d..%d", who, (int)q[2 * i + c], c ? "dy" : "dx",
                   i % (size_t)np, i / (size_t)np, STAB_QMAX, STAB_QMAX);
        qv[i] = stab_pack(q[2 * i], q[2 * i + 1], valid[i]);
    }
    return HM_OK;
}

extern "C" int hm_body_rec_field_sums(hm_ctx_t h, int k0, int n_frames, int B, const int16_t *q, const uint8_t *valid, uint32_t *out)
{
    HM_ARG(B >= STAB_BMIN && B <= STAB_BMAX, "hm_body_rec_field_sums: patch size %d outside %d..%d", B, STAB_BMIN, STAB_BMAX);
    HM_ARG((long long)n_frames * 255 < (1ll << 32), "hm_body_rec_field_sums: %d frames x 255 could pass 2^32", n_frames);
    HM_ARG(h && q && valid && out, "hm_body_rec_field_sums: NULL handle, q, valid or output");
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_field_sums");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n_frames >= 0 && k0 <= h->rec.frames && n_frames <= h->rec.frames - k0,
           "hm_body_rec_field_sums: frames %d .. %d of a record of %d", k0, k0 + n_frames - 1, h->rec.frames);
    const RecBox &b = h->rec.box;
    StabFieldSum g;
    g.B = B; g.npx = hm_cdiv(b.bw, B); g.npy = hm_cdiv(b.bh, B); g.np = g.npx * g.npy;
    const size_t n = (size_t)h->W * h->H, ns = (size_t)n_frames * g.np;
    std::vector<unsigned> qv;
    rc = stab_field_pack(q, valid, ns, g.np, "hm_body_rec_field_sums", qv);
    if (rc) return rc;
    unsigned *d_qv = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) {
        g.out = cv.take<unsigned>(n);
        d_qv = cv.take<unsigned>(ns);
    });
    if (rc) return rc;
    if (ns) HM_HIP(hipMemcpyAsync(d_qv, qv.data(), ns * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(g.out, 0, n * sizeof(unsigned), h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.W = h->W; g.k0 = k0; g.F = n_frames;
    g.tri_of = h->body.tri; g.qv = d_qv;
    hipLaunchKernelGGL(k_stab_field_sums, dim3(hm_cdiv(b.bw * b.bh, 256)), dim3(256), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, g.out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_body_rec_warp(hm_ctx_t h, int B, const int16_t *q, const uint8_t *valid)
{
    HM_ARG(B >= STAB_BMIN && B <= STAB_BMAX, "hm_body_rec_warp: patch size %d outside %d..%d", B, STAB_BMIN, STAB_BMAX);
    HM_ARG(h && q && valid, "hm_body_rec_warp: NULL handle, q or valid");
    HM_JOIN_LAZY(h);
    int rc = body_rec_ready(h, "hm_body_rec_warp");
    if (rc) return rc;
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames;
    StabWarp g;
    g.b = b; g.W = h->W; g.B = B; g.npx = hm_cdiv(b.bw, B); g.npy = hm_cdiv(b.bh, B); g.np = g.npx * g.npy; g.tri_of = h->body.tri;
    const size_t ns = (size_t)F * g.np;
    std::vector<unsigned> qv;
    rc = stab_field_pack(q, valid, ns, g.np, "hm_body_rec_warp", qv);
    if (rc) return rc;
    unsigned *d_qv = nullptr;
    rc = body_rec_carve(h, [&](RecCarve &cv) { d_qv = cv.take<unsigned>(ns); });
    if (rc) return rc;
    // runs of frames within a chunk: copied aside as they are, then sampled back into the record (as hm_body_rec_shift)
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(b.fpc, F), STAB_SCRATCH_BYTES / b.fs));
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        HM_HIP(hipMemcpyAsync(d_qv, qv.data(), ns * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
        const int blocks = hm_cdiv((b.pitch >> 2) * b.bh, 256);
        for (int k = 0; k < F;) {
            const int ch = k / b.fpc, m = std::min(per, std::min(F, (ch + 1) * b.fpc) - k);
            uint8_t *dst = h->rec.chunks[ch] + (size_t)(k - ch * b.fpc) * b.fs;
            HM_HIP(hipMemcpyAsync(h->rec.scr, dst, (size_t)m * b.fs, hipMemcpyDeviceToDevice, h->stream));
            g.frames = m; g.qv = d_qv + (size_t)k * g.np; g.src = h->rec.scr; g.dst = dst;
            hipLaunchKernelGGL(k_stab_warp, dim3(blocks, std::min(m, 65535)), dim3(256), 0, h->stream, g);
            HM_HIP(hipGetLastError());
            k += m;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    };
    rc = run();
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

// ---- the running baseline per pixel of the record: baseline, excess and dF/F planes (detrend_kernels.h) -------------
static int det_args_ok(const char *who, int what, int half, int q, int floor, int gain)
{
    HM_ARG(what >= 0 && what <= 3, "%s: kind of plane %d outside 0..3 (0 as recorded, 1 baseline, 2 excess, 3 dF/F byte)", who, what);
    HM_ARG(half >= 0 && half <= DET_HALF_MAX, "%s: half %d outside 0..%d", who, half, DET_HALF_MAX);
    HM_ARG(q >= 0 && q <= 100, "%s: q %d outside 0..100", who, q);
    HM_ARG(floor >= 1 && floor <= 255, "%s: floor %d outside 1..255", who, floor);
    HM_ARG(gain >= 1 && gain <= 65535, "%s: gain %d outside 1..65535", who, gain);
    return HM_OK;
}

// frames scratch of at most STAB_SCRATCH_BYTES holds (one frame at least), of `want` frames
static int det_scratch_frames(const RecBox &b, int want)
{
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(want, 1), STAB_SCRATCH_BYTES / b.fs));
}

// queue planes `what` (1..3) of the frames k .. k + m - 1 into dst (m frames in the record's layout)
static int det_queue(hm_ctx *h, int k, int m, int what, int half, int q, int floor, int gain, uint8_t *dst)
{
    RecRunning g;
    g.b = h->rec.box; g.chunks = (const uint8_t *const *)h->rec.tab; g.F = h->rec.frames; g.k0 = k; g.n = m;
    g.run = h->rec.bl_frames; g.what = what; g.half = half; g.q = q; g.floor = floor; g.gain = gain; g.out = dst;
    const int segs = hm_cdiv(g.b.pitch * g.b.bh, 64), runs = hm_cdiv(m, g.run);
    hipLaunchKernelGGL(k_rec_running, dim3(segs, std::min(runs, 65535)), dim3(64), DET_LDS_BYTES, h->stream, g);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_body_rec_planes(hm_ctx_t h, int k0, int n_frames, int what, int half, int q, int floor, int gain, uint8_t *out)
{
    int rc = det_args_ok("hm_body_rec_planes", what, half, q, floor, gain);
    if (rc) return rc;
    HM_ARG(h != nullptr, "hm_body_rec_planes: NULL handle");
    HM_JOIN_LAZY(h);
    rc = body_rec_ready(h, "hm_body_rec_planes");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n_frames >= 0 && k0 <= h->rec.frames && n_frames <= h->rec.frames - k0,
           "hm_body_rec_planes: frames %d .. %d of a record of %d", k0, k0 + n_frames - 1, h->rec.frames);
    HM_ARG(out || n_frames == 0, "hm_body_rec_planes: NULL output");
    const RecBox &b = h->rec.box;
    const size_t px = (size_t)h->W * h->H;
    // one box frame on the device -> a full plane of the caller's (as hm_body_rec_fetch lays it out)
    auto expand = [&](const uint8_t *src, uint8_t *o) -> int {
        memset(o, 0, px);
        HM_HIP(hipMemcpy2D(o + (size_t)b.r0 * h->W + b.c0, (size_t)h->W, src, (size_t)b.pitch, (size_t)b.bw, (size_t)b.bh,
                           hipMemcpyDeviceToHost));
        return HM_OK;
    };
    if (what == 0) {
        HM_HIP(hipStreamSynchronize(h->stream));
        for (int k = 0; k < n_frames; k++) {
            const int ch = (k0 + k) / b.fpc;
            rc = expand(h->rec.chunks[ch] + (size_t)(k0 + k - ch * b.fpc) * b.fs, out + (size_t)k * px);
            if (rc) return rc;
        }
        return HM_OK;
    }
    const int per = det_scratch_frames(b, n_frames);
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        for (int k = 0; k < n_frames;) {
            const int m = std::min(per, n_frames - k);
            int r = det_queue(h, k0 + k, m, what, half, q, floor, gain, h->rec.scr);
            if (r) return r;
            HM_HIP(hipStreamSynchronize(h->stream));
            for (int j = 0; j < m; j++) {
                r = expand(h->rec.scr + (size_t)j * b.fs, out + (size_t)(k + j) * px);
                if (r) return r;
            }
            k += m;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    };
    rc = run();
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

extern "C" int hm_body_rec_stats_add(hm_ctx_t h, int what, int half, int q, int floor, int gain)
{
    int rc = det_args_ok("hm_body_rec_stats_add", what, half, q, floor, gain);
    if (rc) return rc;
    HM_ARG(h != nullptr, "hm_body_rec_stats_add: NULL handle");
    HM_JOIN_LAZY(h);
    rc = body_rec_ready(h, "hm_body_rec_stats_add");
    if (rc) return rc;
    if (!h->body.stats_on) { hm_set_error("hm_body_rec_stats_add: no statistics (hm_body_stats_begin first)"); return HM_ERR_STATE; }
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames, n = h->W * h->H;
    if (h->body.stats_frames + F > h->body.stats_cap) {
        hm_set_error("hm_body_rec_stats_add: the statistics hold %d frames and the record %d, their capacity is %d (sums of 32 bits "
                     "are exact up to %d frames): nothing added", h->body.stats_frames, F, h->body.stats_cap, BODY_STATS_CAP);
        return HM_ERR_STATE;
    }
    const BodyStats st = body_stats_planes(h);
    // a box frame pasted into the registered plane, then added as a warp's frame is
    auto add = [&](const uint8_t *src) -> int {
        hipLaunchKernelGGL(k_rec_paste, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W, b, src, h->body.reg);
        hipLaunchKernelGGL(k_body_stats_add, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W,
                           (const int *)h->body.tri, (const uint8_t *)h->body.reg, st);
        HM_HIP(hipGetLastError());
        h->body.stats_frames++;
        return HM_OK;
    };
    if (what == 0) {
        for (int k = 0; k < F; k++) {
            const int ch = k / b.fpc;
            rc = add(h->rec.chunks[ch] + (size_t)(k - ch * b.fpc) * b.fs);
            if (rc) return rc;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    }
    const int per = det_scratch_frames(b, F);
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        for (int k = 0; k < F;) {
            const int m = std::min(per, F - k);
            int r = det_queue(h, k, m, what, half, q, floor, gain, h->rec.scr);     // (behind the adds that read the scratch)
            for (int j = 0; !r && j < m; j++) r = add(h->rec.scr + (size_t)j * b.fs);
            if (r) return r;
            k += m;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return HM_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(h->stream);            // (nothing queued reads the scratch once it is freed)
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

// ---- the residual of the record: what the cells' model leaves of every frame (residual_kernels.h) --------------------
static int res_args_ok(const char *who, int n_layers, const int32_t *labels, int L, const int32_t *traces, int offset)
{
    HM_ARG(n_layers >= 1 && n_layers <= 4, "%s: %d layers outside 1..4", who, n_layers);
    HM_ARG(L >= 1 && L <= REC_RES_LMAX, "%s: %d labels outside 1..%d", who, L, REC_RES_LMAX);
    HM_ARG(offset >= 0 && offset <= 255, "%s: offset %d outside 0..255", who, offset);
    HM_ARG(labels && traces, "%s: NULL labels or traces", who);
    return HM_OK;
}

// The cells of the box, packed for k_rec_residual and sent to the device with the traces; a label outside -1 .. L - 1
// anywhere in the planes is refused here.  Off the map and under a blank nothing is packed: a segment of such pixels
// alone costs no layer.
static int res_pack(hm_ctx *h, const char *who, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                    const int32_t *traces, const uint8_t *blank, int offset, bool want_clipped, RecResidual &g)
{
    const RecBox &b = h->rec.box;
    const size_t n = (size_t)h->W * h->H, npx = (size_t)b.pitch * b.bh;
    const int F = h->rec.frames, segs = hm_cdiv((int)(npx >> 2), 64);
    HM_ARG((long long)F * L < (1ll << 30), "%s: %d frames x %d labels", who, F, L);
    for (int j = 0; j < n_layers; j++)
        for (size_t p = 0; p < n; p++) {
            const int s = labels[(size_t)j * n + p];
            HM_ARG(s >= -1 && s < L, "%s: label %d at pixel %zu of layer %d outside -1..%d", who, s, p, j, L - 1);
        }
    std::vector<unsigned> lay((size_t)n_layers * npx, 0u);
    std::vector<uint8_t> live(npx, 0), seg_nl(segs, 0);
    for (int yb = 0; yb < b.bh; yb++)
        for (int x = 0; x < b.bw; x++) {
            const size_t p = (size_t)(b.r0 + yb) * h->W + b.c0 + x, i = (size_t)yb * b.pitch + x;
            if (h->body.h_tri[p] < 0 || (blank && blank[p])) continue;
            live[i] = 1;
            for (int j = 0; j < n_layers; j++) {
                const int s = labels[(size_t)j * n + p];
                if (s < 0) continue;
                lay[(size_t)j * npx + i] = ((unsigned)s << 16) | (weights ? (unsigned)weights[(size_t)j * n + p] : 65535u);
                uint8_t &top = seg_nl[i >> 8];
                top = std::max<uint8_t>(top, (uint8_t)(j + 1));
            }
        }
    unsigned *d_lay = nullptr, *d_live = nullptr;
    uint8_t *d_seg = nullptr;
    int *d_tr = nullptr;
    unsigned long long *d_clip = nullptr;
    const int rc = body_rec_carve(h, [&](RecCarve &cv) {
        d_lay = cv.take<unsigned>(lay.size());
        d_live = cv.take<unsigned>(npx >> 2);
        d_seg = cv.take<uint8_t>(segs);
        d_tr = cv.take<int>((size_t)F * L);
        d_clip = cv.take<unsigned long long>(1);
    });
    if (rc) return rc;
    // (pageable sources: each copy has left the host array when the call returns)
    HM_HIP(hipMemcpyAsync(d_lay, lay.data(), lay.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_live, live.data(), npx, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_seg, seg_nl.data(), (size_t)segs, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(d_tr, traces, (size_t)F * L * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemsetAsync(d_clip, 0, sizeof(unsigned long long), h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    g.b = b; g.chunks = (const uint8_t *const *)h->rec.tab; g.run = h->rec.res_frames; g.nl = n_layers; g.L = L; g.offset = offset;
    g.lay = d_lay; g.live = d_live; g.seg_nl = d_seg; g.traces = d_tr; g.clipped = want_clipped ? d_clip : nullptr;
    return HM_OK;
}

// queue the residual planes of the frames k .. k + m - 1 into dst (m frames in the record's layout)
static int res_queue(hm_ctx *h, RecResidual g, int k, int m, uint8_t *dst)
{
    g.k0 = k; g.n = m; g.out = dst;
    const int segs = hm_cdiv((g.b.pitch * g.b.bh) >> 2, 64), runs = hm_cdiv(m, g.run);
    hipLaunchKernelGGL(k_rec_residual, dim3(segs, std::min(runs, 65535)), dim3(64), 0, h->stream, g);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

static int res_clipped(hm_ctx *h, const RecResidual &g, uint64_t *clipped)
{
    if (!clipped) return HM_OK;
    unsigned long long c = 0;
    HM_HIP(hipMemcpyAsync(&c, g.clipped, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    *clipped = c;
    return HM_OK;
}

extern "C" int hm_body_rec_residual_planes(hm_ctx_t h, int k0, int n_frames, int n_layers, const int32_t *labels,
                                           const uint16_t *weights, int L, const int32_t *traces, const uint8_t *blank,
                                           int offset, uint8_t *out, uint64_t *clipped)
{
    int rc = res_args_ok("hm_body_rec_residual_planes", n_layers, labels, L, traces, offset);
    if (rc) return rc;
    HM_ARG(h != nullptr, "hm_body_rec_residual_planes: NULL handle");
    HM_JOIN_LAZY(h);
    rc = body_rec_ready(h, "hm_body_rec_residual_planes");
    if (rc) return rc;
    HM_ARG(k0 >= 0 && n_frames >= 0 && k0 <= h->rec.frames && n_frames <= h->rec.frames - k0,
           "hm_body_rec_residual_planes: frames %d .. %d of a record of %d", k0, k0 + n_frames - 1, h->rec.frames);
    HM_ARG(out || n_frames == 0, "hm_body_rec_residual_planes: NULL output");
    RecResidual g;
    rc = res_pack(h, "hm_body_rec_residual_planes", n_layers, labels, weights, L, traces, blank, offset, clipped != nullptr, g);
    if (rc) return rc;
    const RecBox &b = h->rec.box;
    const size_t px = (size_t)h->W * h->H;
    const int per = det_scratch_frames(b, n_frames);
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        for (int k = 0; k < n_frames;) {
            const int m = std::min(per, n_frames - k);
            int r = res_queue(h, g, k0 + k, m, h->rec.scr);
            if (r) return r;
            HM_HIP(hipStreamSynchronize(h->stream));
            for (int j = 0; j < m; j++) {
                uint8_t *o = out + (size_t)(k + j) * px;
                memset(o, 0, px);
                HM_HIP(hipMemcpy2D(o + (size_t)b.r0 * h->W + b.c0, (size_t)h->W, h->rec.scr + (size_t)j * b.fs, (size_t)b.pitch,
                                   (size_t)b.bw, (size_t)b.bh, hipMemcpyDeviceToHost));
            }
            k += m;
        }
        return res_clipped(h, g, clipped);
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(h->stream);
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

extern "C" int hm_body_rec_residual_stats_add(hm_ctx_t h, int n_layers, const int32_t *labels, const uint16_t *weights, int L,
                                              const int32_t *traces, const uint8_t *blank, int offset, uint64_t *clipped)
{
    int rc = res_args_ok("hm_body_rec_residual_stats_add", n_layers, labels, L, traces, offset);
    if (rc) return rc;
    HM_ARG(h != nullptr, "hm_body_rec_residual_stats_add: NULL handle");
    HM_JOIN_LAZY(h);
    rc = body_rec_ready(h, "hm_body_rec_residual_stats_add");
    if (rc) return rc;
    if (!h->body.stats_on) {
        hm_set_error("hm_body_rec_residual_stats_add: no statistics (hm_body_stats_begin first)");
        return HM_ERR_STATE;
    }
    const RecBox &b = h->rec.box;
    const int F = h->rec.frames, n = h->W * h->H;
    if (h->body.stats_frames + F > h->body.stats_cap) {
        hm_set_error("hm_body_rec_residual_stats_add: the statistics hold %d frames and the record %d, their capacity is %d (sums "
                     "of 32 bits are exact up to %d frames): nothing added", h->body.stats_frames, F, h->body.stats_cap,
                     BODY_STATS_CAP);
        return HM_ERR_STATE;
    }
    RecResidual g;
    rc = res_pack(h, "hm_body_rec_residual_stats_add", n_layers, labels, weights, L, traces, blank, offset, clipped != nullptr, g);
    if (rc) return rc;
    const BodyStats st = body_stats_planes(h);
    const int per = det_scratch_frames(b, F);
    HM_HIP(h->own.grow(&h->rec.scr, (size_t)per * b.fs));
    auto run = [&]() -> int {
        for (int k = 0; k < F;) {
            const int m = std::min(per, F - k);
            const int r = res_queue(h, g, k, m, h->rec.scr);                    // (behind the adds that read the scratch)
            if (r) return r;
            // a box frame pasted into the registered plane, then added as a warp's frame is (as hm_body_rec_stats_add)
            for (int j = 0; j < m; j++) {
                hipLaunchKernelGGL(k_rec_paste, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W, b,
                                   (const uint8_t *)(h->rec.scr + (size_t)j * b.fs), h->body.reg);
                hipLaunchKernelGGL(k_body_stats_add, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W,
                                   (const int *)h->body.tri, (const uint8_t *)h->body.reg, st);
                HM_HIP(hipGetLastError());
                h->body.stats_frames++;
            }
            k += m;
        }
        HM_HIP(hipStreamSynchronize(h->stream));
        return res_clipped(h, g, clipped);
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(h->stream);            // (nothing queued reads the scratch once it is freed)
    const hipError_t fe = h->own.free(&h->rec.scr);           // on the error paths too (the first error is the one reported)
    if (rc) return rc;
    HM_HIP(fe);
    return HM_OK;
}

// ---- the flow tool's preview video (reference src/optical_flow_ext.cpp:172-281, 336-389) ---------------------------
extern "C" int hm_flow_preview(int device, int n, int W, int H, int channels, const uint8_t *frames, const float *fx,
                               const float *fy, uint8_t *out, int on_device, void *stream)
{
    HM_ARG(frames && fx && fy && out, "hm_flow_preview: NULL argument");
    HM_ARG(n >= 1 && W >= 1 && H >= 1 && (channels == 1 || channels == 3),
           "hm_flow_preview: bad size n=%d %dx%d channels=%d", n, W, H, channels);
    HM_HIP(hipSetDevice(device));
    const long long px = (long long)n * W * H;
    const dim3 grid((unsigned)((px + 255) / 256));
    if (on_device) {
        hipLaunchKernelGGL(k_flow_preview, grid, dim3(256), 0, (hipStream_t)stream, frames, channels, fx, fy, px, out);
        HM_HIP(hipGetLastError());
        return HM_OK;
    }
    uint8_t *d_f = nullptr, *d_o = nullptr;
    float *d_x = nullptr, *d_y = nullptr;
    int rc = HM_OK;
    auto run = [&]() -> int {
        HM_HIP(hm_malloc((void **)&d_f, (size_t)px * channels));
        HM_HIP(hm_malloc((void **)&d_o, (size_t)px * 3));
        HM_HIP(hm_malloc((void **)&d_x, (size_t)px * sizeof(float)));
        HM_HIP(hm_malloc((void **)&d_y, (size_t)px * sizeof(float)));
        HM_HIP(hipMemcpy(d_f, frames, (size_t)px * channels, hipMemcpyHostToDevice));
        HM_HIP(hipMemcpy(d_x, fx, (size_t)px * sizeof(float), hipMemcpyHostToDevice));
        HM_HIP(hipMemcpy(d_y, fy, (size_t)px * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_flow_preview, grid, dim3(256), 0, 0, (const uint8_t *)d_f, channels, (const float *)d_x,
                           (const float *)d_y, px, d_o);
        HM_HIP(hipGetLastError());
        HM_HIP(hipMemcpy(out, d_o, (size_t)px * 3, hipMemcpyDeviceToHost));
        return HM_OK;
    };
    rc = run();
    void *ptrs[] = {d_f, d_o, d_x, d_y};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    return rc;
}

