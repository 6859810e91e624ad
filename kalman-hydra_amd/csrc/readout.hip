// The readout of a filter handle: views (hm_view*), the body-frame readout and its statistics (hm_body_*, hm_body_stats_*),
// the deformation readout (hm_strain_*, hm_view_strain*) and the flow tool's preview.  Host orchestration and C-ABI
// (include/hydra_mi.h); the kernels are in view_kernels.h, body_kernels.h and strain_kernels.h, which this translation unit
// alone compiles.  Of the handle (ctx.h) it uses view, body and strain and reads W, H,
// N, T, device, own, stream, the mesh (d_tri, d_uv, d_tex) and, for the overlay view, have_tex, have_obs and o_yim.  The
// registered video kept on the device (hm_body_rec_*) is record.hip's: of rec, this file reads `on` alone, and a warp
// reaches the record through body_rec_slot and body_rec_queue_copy (ctx.h).
#include "ctx.h"
#include "view_kernels.h"
#include "body_kernels.h"
#include "strain_kernels.h"
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
    HM_ARG(((uintptr_t)d_bgr & 3) == 0, "hm_view_dev: d_bgr is not 4-byte aligned");      // (k_view_compose writes dwords)
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
        HM_TRY(hm_labels_ok("hm_view_set_cells", n_layers, labels, (size_t)h->W * h->H, L));
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

// What a queued view reads of its caller's arrays goes through ViewState's slots: the next page-locked slot, free and at
// least `bytes` long (waits only for the copy out of that very slot), with the device block c_in grown to hold it ...
static int view_stage(hm_ctx *h, size_t bytes, uint8_t **slot)
{
    ViewState &v = h->view;
    const int s = v.c_next;
    HM_HIP(h->own.event(&v.c_slot_ev[s]));
    if (v.c_slot_used[s]) HM_HIP(hipEventSynchronize(v.c_slot_ev[s]));      // (the copy out of this slot has run)
    v.c_slot_used[s] = false;
    HM_HIP(h->own.host_grow(&v.c_slot[s], bytes, hipHostMallocDefault));
    const auto it = h->own.mem.find(v.c_in);
    if (!v.c_in || it == h->own.mem.end() || it->second.bytes < bytes) {
        HM_HIP(hipStreamSynchronize(h->stream));      // (a view in flight reads the block that grows)
        HM_HIP(h->own.grow(&v.c_in, bytes));
    }
    *slot = v.c_slot[s];
    return HM_OK;
}
// ... and, filled, copied to c_in on the handle's stream: the caller's arrays are free when this returns
static int view_stage_send(hm_ctx *h, size_t bytes)
{
    ViewState &v = h->view;
    const int s = v.c_next;
    HM_HIP(hipMemcpyAsync(v.c_in, v.c_slot[s], bytes, hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipEventRecord(v.c_slot_ev[s], h->stream));
    v.c_slot_used[s] = true;
    v.c_next = (s + 1) % VIEW_CELL_SLOTS;
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
    uint8_t *slot = nullptr;
    HM_TRY(view_stage(h, bytes, &slot));
    memcpy(slot + oX, X, oP);
    if (P) memcpy(slot + oP, points, (size_t)2 * P * sizeof(double));
    if (levels && L) memcpy(slot + oL, levels, (size_t)L);
    if (P) memcpy(slot + oC, point_colours, (size_t)3 * P);
    HM_TRY(view_stage_send(h, bytes));
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
int body_map_build(hm_ctx *h)
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
    if (labels) HM_TRY(hm_labels_ok("hm_body_set_labels", 0, labels, n, L));
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

int body_stats_queue_add(hm_ctx *h, const uint8_t *d_reg)
{
    const int n = h->W * h->H;
    hipLaunchKernelGGL(k_body_stats_add, dim3(hm_cdiv(hm_cdiv(n, 4), 256)), dim3(256), 0, h->stream, n, h->W,
                       (const int *)h->body.tri, d_reg, body_stats_planes(h));
    HM_HIP(hipGetLastError());
    h->body.stats_frames++;
    return HM_OK;
}

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
    // (before anything is queued: a refused warp leaves statistics and record as they were)
    if (h->rec.on) HM_TRY(body_rec_slot(h, who, &rec_dst));
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
    // (behind the event: whoever waits for the warp's output does not wait for these)
    if (h->body.stats_on) HM_TRY(body_stats_queue_add(h, h->body.reg));
    if (h->rec.on) HM_TRY(body_rec_queue_copy(h, rec_dst));
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

// ---- the deformation readout (strain_kernels.h) ---------------------------------------------------------------------
// n_frames rows of 4N doubles (host) into strain.X, k_strain_tri of all of them into strain.v (n_frames x T x 7), queued
static int strain_queue_tri(hm_ctx *h, int n_frames, const double *X)
{
    StrainState &st = h->strain;
    const size_t row = (size_t)4 * h->N, nx = (size_t)n_frames * row, nv = (size_t)n_frames * h->T * STRAIN_VALS;
    {
        // (a launch in flight reads the buffers that grow)
        const auto ix = h->own.mem.find(st.X), iv = h->own.mem.find(st.v);
        if (!st.X || !st.v || ix->second.bytes < nx * sizeof(double) || iv->second.bytes < nv * sizeof(double))
            HM_HIP(hipStreamSynchronize(h->stream));
    }
    HM_HIP(h->own.grow(&st.X, nx * sizeof(double)));
    HM_HIP(h->own.grow(&st.v, nv * sizeof(double)));
    HM_HIP(hipMemcpyAsync(st.X, X, nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const long long total = (long long)n_frames * h->T;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, STRAIN_MAX_GRID);
    hipLaunchKernelGGL(k_strain_tri, dim3(grid), dim3(256), 0, h->stream, total, h->T, row, (const int4 *)h->body.tidx,
                       (const float *)h->d_uv, (const double *)st.X, st.v);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_strain_tri(hm_ctx_t h, int n_frames, const double *X, double *out)
{
    HM_ARG(h && X && out, "hm_strain_tri: NULL argument");
    HM_ARG(n_frames > 0, "hm_strain_tri: %d frames (need at least 1)", n_frames);
    HM_JOIN_LAZY(h);
    HM_TRY(body_map_build(h));
    HM_TRY(strain_queue_tri(h, n_frames, X));
    HM_HIP(hipMemcpyAsync(out, h->strain.v, (size_t)n_frames * h->T * STRAIN_VALS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));
    return HM_OK;
}

extern "C" int hm_strain_labels(hm_ctx_t h, int n_frames, const double *X, const int32_t *labels, int L, double *out,
                                uint32_t *counts)
{
    HM_ARG(h && X && out, "hm_strain_labels: NULL argument");
    HM_ARG(n_frames > 0, "hm_strain_labels: %d frames (need at least 1)", n_frames);
    HM_ARG(L >= 1, "hm_strain_labels: %d labels (need at least 1)", L);
    const size_t n = (size_t)h->W * h->H;
    if (labels) HM_TRY(hm_labels_ok("hm_strain_labels", 0, labels, n, L));
    HM_JOIN_LAZY(h);
    HM_TRY(body_map_build(h));
    StrainState &st = h->strain;
    std::vector<int32_t> own;
    if (!labels) {
        if (h->body.L == 0) { hm_set_error("hm_strain_labels: no label image given, and hm_body_set_labels has set none"); return HM_ERR_STATE; }
        HM_ARG(L == h->body.L, "hm_strain_labels: %d labels, the image of hm_body_set_labels has %d", L, h->body.L);
        own.resize(n);
        HM_HIP(hipMemcpyAsync(own.data(), h->body.lab, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        labels = own.data();
    }
    if (h->body.h_tri.empty()) {
        h->body.h_tri.resize(n);
        HM_HIP(hipMemcpyAsync(h->body.h_tri.data(), h->body.tri, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HM_HIP(hipStreamSynchronize(h->stream));
    // cnt[s, t] as compressed rows: the (label, triangle) pairs of the map's pixels sorted, runs of equal pairs counted
    std::vector<uint64_t> key;
    for (size_t p = 0; p < n; p++)
        if (h->body.h_tri[p] >= 0 && labels[p] >= 0) key.push_back((uint64_t)labels[p] * h->T + h->body.h_tri[p]);
    std::sort(key.begin(), key.end());
    std::vector<int> off(L + 1, 0), ent_t;
    std::vector<unsigned> ent_c, n_s(L, 0u);
    for (size_t i = 0; i < key.size();) {
        size_t j = i;
        while (j < key.size() && key[j] == key[i]) j++;
        const int s = (int)(key[i] / h->T);
        ent_t.push_back((int)(key[i] % h->T));
        ent_c.push_back((unsigned)(j - i));
        off[s + 1]++;
        n_s[s] += (unsigned)(j - i);
        i = j;
    }
    for (int s = 0; s < L; s++) off[s + 1] += off[s];
    const size_t ne = ent_t.size(), no = (size_t)n_frames * L * 3;
    // (waits for the stream above: nothing in flight reads what grows here)
    HM_HIP(h->own.grow(&st.off, (size_t)(L + 1) * sizeof(int)));
    HM_HIP(h->own.grow(&st.n_s, (size_t)L * sizeof(unsigned)));
    HM_HIP(h->own.grow(&st.ent_t, (ne + 1) * sizeof(int)));
    HM_HIP(h->own.grow(&st.ent_c, (ne + 1) * sizeof(unsigned)));
    HM_HIP(h->own.grow(&st.trace, no * sizeof(double)));
    HM_HIP(hipMemcpyAsync(st.off, off.data(), (size_t)(L + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HM_HIP(hipMemcpyAsync(st.n_s, n_s.data(), (size_t)L * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (ne) {
        HM_HIP(hipMemcpyAsync(st.ent_t, ent_t.data(), ne * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HM_HIP(hipMemcpyAsync(st.ent_c, ent_c.data(), ne * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    }
    HM_TRY(strain_queue_tri(h, n_frames, X));
    const long long total = (long long)n_frames * L;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, STRAIN_MAX_GRID);
    hipLaunchKernelGGL(k_strain_label, dim3(grid), dim3(256), 0, h->stream, total, L, h->T, (const int *)st.off,
                       (const int *)st.ent_t, (const unsigned *)st.ent_c, (const unsigned *)st.n_s, (const double *)st.v, st.trace);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(out, st.trace, no * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HM_HIP(hipStreamSynchronize(h->stream));      // (the host vectors above are read until here)
    if (counts) memcpy(counts, n_s.data(), (size_t)L * sizeof(uint32_t));
    return HM_OK;
}

// Queue the strain view of frame d_frame (device) at state X (host) into d_out (device, W*H*3) on the handle's stream.
static int view_strain_queue(hm_ctx *h, const double *X, const uint8_t *d_frame, int which, double gain, int alpha,
                             const uint8_t *lut, int flags, uint8_t *d_out, const char *who)
{
    ViewState &v = h->view;
    HM_ARG(X && d_frame && d_out, "%s: NULL state, frame or output", who);
    HM_ARG(lut != nullptr, "%s: NULL lut (256 x 3 bytes, B G R)", who);
    HM_ARG(which >= 0 && which <= 2, "%s: which %d outside 0..2 (J, l1, l2)", who, which);
    HM_ARG(alpha >= 0 && alpha <= 255, "%s: alpha %d outside 0..255", who, alpha);
    HM_ARG(flags == 0 || flags == CV_WIRE, "%s: flags %d (0, or %d: the wireframe)", who, flags, CV_WIRE);
    HM_ARG(((uintptr_t)d_out & 3) == 0, "%s: the output is not 4-byte aligned", who);
    HM_TRY(body_map_build(h));                        // (the first call on a handle waits for the map)
    const int n = h->W * h->H;
    const bool wire = (flags & CV_WIRE) != 0;
    // the frame's block: X | lut
    const size_t oL = (size_t)2 * h->N * sizeof(double), bytes = oL + 768;
    HM_HIP(h->own.event(&v.ev));
    if (wire) HM_HIP(h->own.alloc(&v.wire, (size_t)n * sizeof(unsigned)));
    uint8_t *slot = nullptr;
    HM_TRY(view_stage(h, bytes, &slot));
    memcpy(slot, X, oL);
    memcpy(slot + oL, lut, 768);
    HM_TRY(view_stage_send(h, bytes));
    const double *dX = (const double *)v.c_in;
    if (wire) {
        HM_HIP(hipMemsetAsync(v.wire, 0, (size_t)n * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_view_wire, dim3(hm_cdiv(3 * h->T, 256 / VIEW_SEG_WAVE)), dim3(256), 0, h->stream,
                           (const int *)h->d_tri, h->T, dX, h->W, h->H, v.wire);
    }
    StrainViewArgs a;
    a.W = h->W; a.H = h->H; a.T = h->T; a.which = which; a.alpha = alpha; a.flags = flags;
    a.tiles_x = hm_cdiv(h->W, CV_W);
    a.gain = gain;
    a.tri = h->d_tri; a.tidx = h->body.tidx; a.uv = h->d_uv; a.X = dX; a.frame = d_frame;
    a.lut = v.c_in + oL; a.wire = v.wire; a.out = d_out;
    hipLaunchKernelGGL(k_view_strain, dim3(a.tiles_x * hm_cdiv(h->H, CV_H)), dim3(256), 0, h->stream, a);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_view_strain(hm_ctx_t h, const double *X, const uint8_t *frame, int which, double gain, int alpha,
                              const uint8_t *lut, int flags, uint8_t *bgr)
{
    HM_ARG(h && frame && bgr, "hm_view_strain: NULL argument");
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)h->W * h->H;
    HM_HIP(h->own.alloc(&h->view.c_frame, n));
    HM_HIP(h->own.alloc(&h->view.out, 3 * n));
    HM_HIP(hipMemcpyAsync(h->view.c_frame, frame, n, hipMemcpyHostToDevice, h->stream));
    const int rc = view_strain_queue(h, X, h->view.c_frame, which, gain, alpha, lut, flags, h->view.out, "hm_view_strain");
    if (rc) return rc;
    return view_download(h, bgr);
}

extern "C" int hm_view_strain_dev(hm_ctx_t h, const double *X, const void *d_frame, int which, double gain, int alpha,
                                  const uint8_t *lut, int flags, void *d_bgr, void *stream)
{
    HM_ARG(h != nullptr, "hm_view_strain_dev: NULL handle");
    HM_JOIN_LAZY(h);
    HM_HIP(hipSetDevice(h->device));
    const int rc = view_strain_queue(h, X, (const uint8_t *)d_frame, which, gain, alpha, lut, flags, (uint8_t *)d_bgr,
                                     "hm_view_strain_dev");
    if (rc) return rc;
    if (stream) {
        HM_HIP(hipEventRecord(h->view.ev, h->stream));
        HM_HIP(hipStreamWaitEvent((hipStream_t)stream, h->view.ev, 0));
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
    hipError_t e = h->rec.on ? hipSuccess : h->own.free(&h->body.reg);     // (BodyState::reg has the rule)
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


// ---- Motion-JPEG: the baseline JPEG encoder of the video writer (mjpeg_kernels.h) ----------------
#include "mjpeg_kernels.h"
#include "mjpeg_tables.h"


struct hm_mjpeg {
    int device = 0, quality = 0, restart_rows = 1;
    MjGeo g{};
    MjTables tab{};
    std::vector<uint8_t> header;
    uint64_t max_stream = 0;
    HmOwner own{1};
    // built by the first encode
    MjTables *d_tab = nullptr;
    int16_t *d_coef = nullptr;
    uint16_t *d_acbits = nullptr;
    unsigned *d_bitbuf = nullptr, *d_ibits = nullptr, *d_isize = nullptr, *d_ioff = nullptr;
    bool ready = false;
    // hm_mjpeg_encode's own
    hipStream_t stream = nullptr;
    uint8_t *d_frame = nullptr, *d_out = nullptr;
    unsigned *d_size = nullptr;
};

static void mj_header(hm_mjpeg *e)
{
    std::vector<uint8_t> &h = e->header;
    auto seg = [&](uint8_t marker, const std::vector<uint8_t> &body) {
        h.push_back(0xFF); h.push_back(marker);
        const size_t n = body.size() + 2;
        h.push_back((uint8_t)(n >> 8)); h.push_back((uint8_t)n);
        h.insert(h.end(), body.begin(), body.end());
    };
    const int C = e->g.C, sets = C == 3 ? 2 : 1;
    h.push_back(0xFF); h.push_back(0xD8);                                                       // SOI
    seg(0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                              // APP0: JFIF 1.01, 1:1
    for (int s = 0; s < sets; s++) {                                                            // DQT, 8 bits, zigzag order
        std::vector<uint8_t> b{(uint8_t)s};
        for (int k = 0; k < 64; k++) b.push_back((uint8_t)e->tab.quant[s][k]);
        seg(0xDB, b);
    }
    {                                                                                           // SOF0
        std::vector<uint8_t> b{8, (uint8_t)(e->g.H >> 8), (uint8_t)e->g.H, (uint8_t)(e->g.W >> 8), (uint8_t)e->g.W, (uint8_t)C};
        for (int c = 0; c < C; c++) { b.push_back((uint8_t)(c + 1)); b.push_back(0x11); b.push_back(c ? 1 : 0); }
        seg(0xC0, b);
    }
    for (int s = 0; s < sets; s++) {                                                            // DHT: DC then AC of each set
        std::vector<uint8_t> b{(uint8_t)s};
        b.insert(b.end(), MJ_DC_BITS[s], MJ_DC_BITS[s] + 16);
        b.insert(b.end(), MJ_DC_VALS, MJ_DC_VALS + 12);
        seg(0xC4, b);
        std::vector<uint8_t> a{(uint8_t)(0x10 | s)};
        a.insert(a.end(), MJ_AC_BITS[s], MJ_AC_BITS[s] + 16);
        a.insert(a.end(), MJ_AC_VALS[s], MJ_AC_VALS[s] + 162);
        seg(0xC4, a);
    }
    seg(0xDD, {(uint8_t)(e->g.ri >> 8), (uint8_t)e->g.ri});                                     // DRI
    {                                                                                           // SOS
        std::vector<uint8_t> b{(uint8_t)C};
        for (int c = 0; c < C; c++) { b.push_back((uint8_t)(c + 1)); b.push_back(c ? 0x11 : 0x00); }
        b.push_back(0); b.push_back(63); b.push_back(0);
        seg(0xDA, b);
    }
}

extern "C" int hm_mjpeg_create(int device, int W, int H, int channels, int quality, int restart_rows, hm_mjpeg_t *out)
{
    HM_ARG(out, "hm_mjpeg_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "hm_mjpeg_create: frame size %dx%d outside 1..32767", W, H);
    HM_ARG(channels == 1 || channels == 3, "hm_mjpeg_create: %d channels, not 1 or 3", channels);
    HM_ARG(quality >= 1 && quality <= 100, "hm_mjpeg_create: quality %d outside 1..100", quality);
    HM_ARG(restart_rows >= 1, "hm_mjpeg_create: restart_rows %d below 1", restart_rows);
    const int bw = (W + 7) / 8, bh = (H + 7) / 8;
    const long long ri = (long long)bw * std::min(restart_rows, bh);
    HM_ARG(ri <= 65535, "hm_mjpeg_create: %lld blocks in a restart interval (%d across, %d rows), more than 65535", ri, bw,
           std::min(restart_rows, bh));
    hm_mjpeg *e = new hm_mjpeg();
    e->device = device; e->quality = quality; e->restart_rows = restart_rows;
    MjGeo &g = e->g;
    g.W = W; g.H = H; g.C = channels; g.bw = bw; g.bh = bh;
    g.ri = (int)ri;
    g.n_mcu = bw * bh;
    g.n_int = (g.n_mcu + g.ri - 1) / g.ri;
    e->max_stream = (uint64_t)g.n_mcu * channels * (8 * MJ_BLOCK_WORDS) + 2ull * g.n_int;
    if (e->max_stream >= (1ull << 31)) {
        hm_set_error("hm_mjpeg_create: a frame of %dx%d x %d can code to %llu bytes, 2^31 or more", W, H, channels,
                     (unsigned long long)e->max_stream);
        delete e;
        return HM_ERR_ARG;
    }
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int s = 0; s < 2; s++) {
        for (int i = 0; i < 64; i++)
            e->tab.quant[s][mj_zigzag_pos(i)] = (uint16_t)std::min(255, std::max(1, (MJ_QUANT[s][i] * scale + 50) / 100));
        mj_huffman(MJ_DC_BITS[s], MJ_DC_VALS, e->tab.dc_code[s], e->tab.dc_len[s]);
        mj_huffman(MJ_AC_BITS[s], MJ_AC_VALS[s], e->tab.ac_code[s], e->tab.ac_len[s]);
    }
    mj_header(e);
    *out = e;
    return HM_OK;
}

extern "C" int hm_mjpeg_destroy(hm_mjpeg_t e)
{
    if (!e) return HM_OK;
    if (!e->own.mem.empty() || !e->own.streams.empty()) {      // (also what a first encode that failed part-way left)
        (void)hipSetDevice(e->device);
        (void)hipDeviceSynchronize();           // (encodes queued on the callers' streams read the handle's buffers)
        e->own.release();
    }
    delete e;
    return HM_OK;
}

extern "C" int hm_mjpeg_header(hm_mjpeg_t e, uint8_t *buf, uint64_t cap, uint64_t *n)
{
    HM_ARG(e && n, "hm_mjpeg_header: NULL argument");
    *n = e->header.size();
    if (!buf) return HM_OK;                     // (the size alone)
    HM_ARG(cap >= e->header.size(), "hm_mjpeg_header: the header has %zu bytes, the buffer %llu", e->header.size(),
           (unsigned long long)cap);
    memcpy(buf, e->header.data(), e->header.size());
    return HM_OK;
}

extern "C" uint64_t hm_mjpeg_max_bytes(hm_mjpeg_t e) { return e ? e->header.size() + e->max_stream : 0; }

static int mj_buffers(hm_mjpeg *e)
{
    if (e->ready) return HM_OK;
    const MjGeo &g = e->g;
    const size_t nblk = (size_t)g.n_mcu * g.C;
    HM_HIP(e->own.alloc(&e->d_tab, sizeof(MjTables)));
    HM_HIP(e->own.alloc(&e->d_coef, nblk * 64 * sizeof(int16_t)));
    HM_HIP(e->own.alloc(&e->d_acbits, nblk * sizeof(uint16_t)));
    HM_HIP(e->own.alloc(&e->d_bitbuf, nblk * MJ_BLOCK_WORDS * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_ibits, (size_t)g.n_int * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_isize, (size_t)g.n_int * sizeof(unsigned)));
    HM_HIP(e->own.alloc(&e->d_ioff, ((size_t)g.n_int + 1) * sizeof(unsigned)));
    HM_HIP(hipMemcpy(e->d_tab, &e->tab, sizeof(MjTables), hipMemcpyHostToDevice));
    HM_HIP(hipMemset(e->d_bitbuf, 0, nblk * MJ_BLOCK_WORDS * sizeof(unsigned)));     // k_mjpeg_pack keeps it zero
    HM_HIP(hipDeviceSynchronize());
    e->ready = true;
    return HM_OK;
}

extern "C" int hm_mjpeg_encode_dev(hm_mjpeg_t e, const void *d_frame, void *out, uint64_t cap, uint32_t *size_word, void *stream)
{
    HM_ARG(e && d_frame && out && size_word, "hm_mjpeg_encode_dev: NULL argument");
    HM_HIP(hipSetDevice(e->device));
    HM_TRY(mj_buffers(e));
    const MjGeo &g = e->g;
    hipStream_t s = (hipStream_t)stream;
    const unsigned cap32 = (unsigned)std::min<uint64_t>(cap, 0xFFFFFFFFull);
    hipLaunchKernelGGL(k_mjpeg_blocks, dim3((unsigned)hm_cdiv(g.n_mcu, mj_blocks_mcus(g.C))), dim3(MJ_THREADS), 0, s, g,
                       (const MjTables *)e->d_tab, (const uint8_t *)d_frame, e->d_coef, e->d_acbits);
    const int emit_threads = std::min(MJ_EMIT_MAX, (g.ri * g.C + 63) / 64 * 64);       // whole waves
    hipLaunchKernelGGL(k_mjpeg_emit, dim3((unsigned)g.n_int), dim3((unsigned)emit_threads), 0, s, g, (const MjTables *)e->d_tab,
                       (const int16_t *)e->d_coef, (const uint16_t *)e->d_acbits, e->d_bitbuf, e->d_ibits);
    hipLaunchKernelGGL(k_mjpeg_count, dim3((unsigned)g.n_int), dim3(MJ_THREADS), 0, s, g, (const unsigned *)e->d_bitbuf,
                       (const unsigned *)e->d_ibits, e->d_isize);
    hipLaunchKernelGGL(k_mjpeg_offsets, dim3(1), dim3(MJ_THREADS), 0, s, g, (const unsigned *)e->d_isize, e->d_ioff);
    hipLaunchKernelGGL(k_mjpeg_pack, dim3((unsigned)g.n_int), dim3(MJ_THREADS), 0, s, g, e->d_bitbuf, (const unsigned *)e->d_ibits,
                       (const unsigned *)e->d_isize, (const unsigned *)e->d_ioff, (uint8_t *)out, cap32, (unsigned *)size_word);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_mjpeg_encode(hm_mjpeg_t e, const uint8_t *frame, uint8_t *out, uint64_t cap, uint64_t *n)
{
    HM_ARG(e && frame && out && n, "hm_mjpeg_encode: NULL argument");
    *n = 0;
    const size_t hdr = e->header.size();
    HM_ARG(cap > hdr, "hm_mjpeg_encode: a buffer of %llu bytes does not hold the header's %zu", (unsigned long long)cap, hdr);
    HM_HIP(hipSetDevice(e->device));
    const size_t fb = (size_t)e->g.W * e->g.H * e->g.C;
    const uint64_t room = std::min<uint64_t>(cap - hdr, e->max_stream);
    HM_HIP(e->own.stream(&e->stream, false));
    HM_HIP(e->own.alloc(&e->d_frame, fb));
    HM_HIP(e->own.grow(&e->d_out, (size_t)room));
    HM_HIP(e->own.alloc(&e->d_size, sizeof(unsigned)));
    HM_HIP(hipMemcpyAsync(e->d_frame, frame, fb, hipMemcpyHostToDevice, e->stream));
    HM_TRY(hm_mjpeg_encode_dev(e, e->d_frame, e->d_out, room, e->d_size, e->stream));
    unsigned size = 0;
    HM_HIP(hipMemcpyAsync(&size, e->d_size, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    HM_HIP(hipStreamSynchronize(e->stream));
    *n = hdr + size;
    HM_ARG(size <= room, "hm_mjpeg_encode: the frame codes to %zu + %u bytes, the buffer has %llu", hdr, size,
           (unsigned long long)cap);
    memcpy(out, e->header.data(), hdr);
    HM_HIP(hipMemcpy(out + hdr, e->d_out, size, hipMemcpyDeviceToHost));
    return HM_OK;
}


// ---- Motion-JPEG, decoding (mjpeg_dec_kernels.h, mjpeg_dec.cpp) -----------------------------------
#include "mjpeg_dec_kernels.h"
#include <string>

static_assert(sizeof(MjdFrame) == HM_MJPEG_DESC_BYTES, "hydra_mi.h states the size of a frame's descriptor");

struct hm_mjpeg_dec {
    int device = 0, W = 0, H = 0, max_run = 1;
    int entropy = HM_MJPEG_ENTROPY_AUTO, pool = 4;                          // hm_mjpeg_dec_tune
    int auto_intervals = 512;                    // hm_mjpeg_dec_tune "auto_intervals": measured, DESIGN section 23 (256: the host pool still wins)
    size_t blk_cap = 0;                          // luma blocks of a frame's slot in the coefficient buffer
    HmOwner own{1};
    std::vector<MjdParsed> parsed;               // per frame of a run, reused
    MjdPool *workers = nullptr;                  // the host entropy path's threads: started by the first run that needs them
    uint64_t last_h2d = 0, total_h2d = 0;        // bytes the last run, and all runs, queued host-to-device
    // built by the first decode; the byte and interval buffers grow when a run is larger than any before
    bool ready = false;
    MjdFrame *d_frames = nullptr;
    MjdInterval *d_iv = nullptr;
    uint8_t *d_bytes = nullptr;
    int16_t *d_coef = nullptr;
    unsigned *d_bad = nullptr;
    size_t iv_cap = 0, bytes_cap = 0;
    struct Stage {                               // page-locked; two, used in turn, so that a run never writes what the copies
        MjdFrame *frames = nullptr;              // of the run before may still read
        MjdInterval *iv = nullptr;
        uint8_t *bytes = nullptr;
        int16_t *coef = nullptr;                 // host entropy path only
        hipEvent_t copied = nullptr;
        bool used = false;
    } stage[2];
    int turn = 0;
    // hm_mjpeg_decode's own
    hipStream_t stream = nullptr;
    uint8_t *d_out = nullptr;
    uint32_t *d_status = nullptr;
};

extern "C" int hm_mjpeg_dec_create(int device, int W, int H, int max_run, hm_mjpeg_dec_t *out)
{
    HM_ARG(out, "hm_mjpeg_dec_create: out is NULL");
    *out = nullptr;
    HM_ARG(W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "hm_mjpeg_dec_create: frame size %dx%d outside 1..32767", W, H);
    HM_ARG(max_run >= 1 && max_run <= 64, "hm_mjpeg_dec_create: max_run %d outside 1..64", max_run);
    hm_mjpeg_dec *d = new hm_mjpeg_dec();
    d->device = device; d->W = W; d->H = H; d->max_run = max_run;
    d->blk_cap = (size_t)(2 * ((W + 15) / 16)) * (size_t)(2 * ((H + 15) / 16));        // covers every accepted sampling
    d->parsed.resize((size_t)max_run);
    *out = d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_destroy(hm_mjpeg_dec_t d)
{
    if (!d) return HM_OK;
    if (!d->own.mem.empty() || !d->own.streams.empty() || !d->own.events.empty()) {
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();           // (decodes queued on the callers' streams read the handle's buffers)
        d->own.release();
    }
    delete d->workers;
    delete d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_uploaded(hm_mjpeg_dec_t d, uint64_t *last_run, uint64_t *total)
{
    HM_ARG(d, "hm_mjpeg_dec_uploaded: NULL handle");
    if (last_run) *last_run = d->last_h2d;
    if (total) *total = d->total_h2d;
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_tune(hm_mjpeg_dec_t d, const char *name, int value)
{
    HM_ARG(d && name, "hm_mjpeg_dec_tune: NULL argument");
    const std::string n(name);
    if (n == "entropy") {
        HM_ARG(value >= HM_MJPEG_ENTROPY_AUTO && value <= HM_MJPEG_ENTROPY_DEVICE, "hm_mjpeg_dec_tune: entropy %d is none of 0 auto, 1 host, 2 device", value);
        d->entropy = value;
    } else if (n == "pool") {
        HM_ARG(value >= 1 && value <= 16, "hm_mjpeg_dec_tune: pool %d outside 1..16", value);
        d->pool = value;
    } else if (n == "auto_intervals") {
        HM_ARG(value >= 0, "hm_mjpeg_dec_tune: auto_intervals %d below 0", value);
        d->auto_intervals = value;
    } else {
        HM_ARG(false, "hm_mjpeg_dec_tune: no tune named '%s' (entropy, pool, auto_intervals)", name);
    }
    return HM_OK;
}

static int mjd_parse_for(hm_mjpeg_dec *d, const char *who, const uint8_t *file, uint64_t n, MjdParsed *p)
{
    HM_TRY(mjd_parse(file, n, p));
    HM_ARG(p->W == d->W && p->H == d->H, "%s: a frame of %dx%d for a decoder of %dx%d", who, p->W, p->H, d->W, d->H);
    return HM_OK;
}

extern "C" int hm_mjpeg_dec_entropy_host(hm_mjpeg_dec_t d, const uint8_t *file, uint64_t n, int16_t *coef, uint64_t cap,
                                         uint32_t *bad)
{
    HM_ARG(d && file && coef && bad, "hm_mjpeg_dec_entropy_host: NULL argument");
    MjdParsed &p = d->parsed[0];
    HM_TRY(mjd_parse_for(d, "hm_mjpeg_dec_entropy_host", file, n, &p));
    const uint64_t need = (uint64_t)p.frame.scan.n_mcu * p.hs * p.vs * 64;
    HM_ARG(cap >= need, "hm_mjpeg_dec_entropy_host: %llu coefficients, room for %llu", (unsigned long long)need, (unsigned long long)cap);
    HM_ARG(((uintptr_t)coef & 7) == 0, "hm_mjpeg_dec_entropy_host: coef is not 8-byte aligned");
    *bad = mjd_entropy_host(p, file, coef);
    return HM_OK;
}

static int mjd_buffers(hm_mjpeg_dec *d)
{
    if (d->ready) return HM_OK;
    const size_t run = (size_t)d->max_run;
    HM_HIP(d->own.alloc(&d->d_frames, run * sizeof(MjdFrame)));
    HM_HIP(d->own.alloc(&d->d_coef, run * d->blk_cap * 64 * sizeof(int16_t)));
    HM_HIP(d->own.alloc(&d->d_bad, run * sizeof(unsigned)));
    for (hm_mjpeg_dec::Stage &s : d->stage) {
        HM_HIP(d->own.host_alloc(&s.frames, run * sizeof(MjdFrame), hipHostMallocDefault));
        HM_HIP(d->own.event(&s.copied));
    }
    HM_HIP(hipMemset(d->d_bad, 0, run * sizeof(unsigned)));       // k_mjdec_idct keeps it zero
    HM_HIP(hipDeviceSynchronize());
    d->ready = true;
    return HM_OK;
}

extern "C" int hm_mjpeg_decode_run_dev(hm_mjpeg_dec_t d, int nframes, const uint8_t *const *files, const uint64_t *sizes,
                                       void *d_frame, void *d_mask, void *d_shown, uint64_t frame_stride, uint64_t pitch,
                                       int threshold, uint32_t *status_words, void *stream)
{
    HM_ARG(d && files && sizes && d_frame, "hm_mjpeg_decode_run_dev: NULL argument");
    HM_ARG(nframes >= 1 && nframes <= d->max_run, "hm_mjpeg_decode_run_dev: %d frames outside 1..max_run = %d", nframes, d->max_run);
    HM_ARG(pitch >= (uint64_t)d->W, "hm_mjpeg_decode_run_dev: a row pitch of %llu for rows of %d", (unsigned long long)pitch, d->W);
    HM_ARG(nframes == 1 || frame_stride >= pitch * (uint64_t)(d->H - 1) + (uint64_t)d->W,
           "hm_mjpeg_decode_run_dev: a frame stride of %llu for frames of %d rows at pitch %llu", (unsigned long long)frame_stride, d->H,
           (unsigned long long)pitch);
    // the frames: parsed and refused before anything is queued
    size_t n_iv = 0, n_bytes = 0, n_host = 0;
    unsigned max_int = 0, max_blk = 0;
    for (int i = 0; i < nframes; i++) {
        HM_ARG(files[i], "hm_mjpeg_decode_run_dev: frame %d is NULL", i);
        MjdParsed &p = d->parsed[(size_t)i];
        HM_TRY(mjd_parse_for(d, "hm_mjpeg_decode_run_dev", files[i], sizes[i], &p));
        MjdFrame &f = p.frame;
        const bool dev = d->entropy == HM_MJPEG_ENTROPY_DEVICE ||
                         (d->entropy == HM_MJPEG_ENTROPY_AUTO && (d->auto_intervals > 0 ? f.n_int >= (unsigned)d->auto_intervals : p.ri != 0));
        f.dev_entropy = dev ? 1 : 0;
        f.bad_host = 0;
        f.int_off = (uint32_t)n_iv;
        f.data_off = (uint32_t)n_bytes;
        const unsigned nblk = f.scan.n_mcu * (unsigned)(p.hs * p.vs);
        HM_ARG(nblk <= d->blk_cap, "hm_mjpeg_decode_run_dev: %u blocks in frame %d, room for %zu", nblk, i, d->blk_cap);
        max_blk = std::max(max_blk, nblk);
        if (dev) {
            n_iv += f.n_int;
            n_bytes += ((size_t)sizes[i] + 15) & ~(size_t)15;
            max_int = std::max(max_int, f.n_int);
        } else {
            n_host++;
        }
    }
    HM_ARG(n_bytes < (1ull << 32), "hm_mjpeg_decode_run_dev: %zu bytes in a run, 2^32 or more", n_bytes);
    HM_HIP(hipSetDevice(d->device));
    HM_TRY(mjd_buffers(d));
    hipStream_t s = (hipStream_t)stream;
    hm_mjpeg_dec::Stage &st = d->stage[d->turn];
    d->turn ^= 1;
    if (st.used) HM_HIP(hipEventSynchronize(st.copied));          // (the copies of the run before last: long done)
    if (n_iv) {
        HM_HIP(d->own.host_grow(&st.iv, n_iv * sizeof(MjdInterval), hipHostMallocDefault));
        HM_HIP(d->own.host_grow(&st.bytes, n_bytes, hipHostMallocDefault));
        if (n_iv > d->iv_cap || n_bytes > d->bytes_cap) {
            HM_HIP(hipDeviceSynchronize());                       // (queued decodes may read the buffers that move)
            d->iv_cap = std::max(d->iv_cap, n_iv + n_iv / 2);
            d->bytes_cap = std::max(d->bytes_cap, n_bytes + n_bytes / 2);
            HM_HIP(d->own.grow(&d->d_iv, d->iv_cap * sizeof(MjdInterval)));
            HM_HIP(d->own.grow(&d->d_bytes, d->bytes_cap));
        }
    }
    if (n_host) {
        HM_HIP(d->own.host_grow(&st.coef, (size_t)d->max_run * d->blk_cap * 64 * sizeof(int16_t), hipHostMallocDefault));
        const MjdParsed *ps[64];
        const uint8_t *fs[64];
        int16_t *cs[64];
        uint32_t bad[64];
        int which[64], k = 0;
        for (int i = 0; i < nframes; i++)
            if (!d->parsed[(size_t)i].frame.dev_entropy) {
                ps[k] = &d->parsed[(size_t)i]; fs[k] = files[i]; cs[k] = st.coef + (size_t)i * d->blk_cap * 64; which[k++] = i;
            }
        if (d->workers && d->workers->threads() != d->pool) { delete d->workers; d->workers = nullptr; }      // (re-tuned)
        if (!d->workers) d->workers = new MjdPool(d->pool);
        d->workers->run(k, ps, fs, cs, bad);
        for (int j = 0; j < k; j++) d->parsed[(size_t)which[j]].frame.bad_host = bad[j];
    }
    for (int i = 0; i < nframes; i++) {
        const MjdParsed &p = d->parsed[(size_t)i];
        st.frames[i] = p.frame;
        if (p.frame.dev_entropy) {
            memcpy(st.iv + p.frame.int_off, p.intervals.data(), p.intervals.size() * sizeof(MjdInterval));
            memcpy(st.bytes + p.frame.data_off, files[i], (size_t)sizes[i]);
        }
    }
    uint64_t h2d = (uint64_t)nframes * sizeof(MjdFrame);         // every host-to-device copy below adds its size
    HM_HIP(hipMemcpyAsync(d->d_frames, st.frames, (size_t)nframes * sizeof(MjdFrame), hipMemcpyHostToDevice, s));
    if (n_iv) {
        HM_HIP(hipMemcpyAsync(d->d_iv, st.iv, n_iv * sizeof(MjdInterval), hipMemcpyHostToDevice, s));
        HM_HIP(hipMemcpyAsync(d->d_bytes, st.bytes, n_bytes, hipMemcpyHostToDevice, s));
        h2d += n_iv * sizeof(MjdInterval) + n_bytes;
    }
    for (int i = 0; i < nframes; i++) {
        const MjdFrame &f = d->parsed[(size_t)i].frame;
        if (f.dev_entropy) continue;
        const size_t at = (size_t)i * d->blk_cap * 64, count = (size_t)f.scan.n_mcu * (size_t)(f.scan.hs * f.scan.vs) * 64;
        HM_HIP(hipMemcpyAsync(d->d_coef + at, st.coef + at, count * sizeof(int16_t), hipMemcpyHostToDevice, s));
        h2d += count * sizeof(int16_t);
    }
    d->last_h2d = h2d;
    d->total_h2d += h2d;
    HM_HIP(hipEventRecord(st.copied, s));
    st.used = true;
    if (n_iv)
        hipLaunchKernelGGL(k_mjdec_entropy, dim3((unsigned)hm_cdiv((int)max_int, MJD_ENT_THREADS), (unsigned)nframes), dim3(MJD_ENT_THREADS),
                           0, s, (const MjdFrame *)d->d_frames, (const MjdInterval *)d->d_iv, (const uint8_t *)d->d_bytes, d->d_coef,
                           d->blk_cap, d->d_bad);
    MjdOut o{};
    o.frame = (uint8_t *)d_frame; o.mask = (uint8_t *)d_mask; o.shown = (uint8_t *)d_shown;
    o.frame_stride = (size_t)frame_stride; o.pitch = (size_t)pitch;
    o.W = d->W; o.H = d->H; o.threshold = threshold;
    o.words = (((uintptr_t)d_frame | (uintptr_t)d_mask | (uintptr_t)d_shown | (uintptr_t)frame_stride | (uintptr_t)pitch) & 3) == 0;
    hipLaunchKernelGGL(k_mjdec_idct, dim3((unsigned)hm_cdiv((int)max_blk, MJD_IDCT_BLOCKS), (unsigned)nframes), dim3(MJD_IDCT_THREADS), 0, s,
                       (const MjdFrame *)d->d_frames, (const int16_t *)d->d_coef, d->blk_cap, o, d->d_bad, status_words);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_mjpeg_decode(hm_mjpeg_dec_t d, const uint8_t *file, uint64_t n, uint8_t *out, int strict, uint32_t *bad)
{
    HM_ARG(d && file && out, "hm_mjpeg_decode: NULL argument");
    if (bad) *bad = 0;
    HM_HIP(hipSetDevice(d->device));
    const size_t fb = (size_t)d->W * d->H;
    HM_HIP(d->own.stream(&d->stream, false));
    HM_HIP(d->own.alloc(&d->d_out, fb));
    HM_HIP(d->own.alloc(&d->d_status, sizeof(uint32_t)));
    const uint8_t *files[1] = {file};
    const uint64_t sizes[1] = {n};
    HM_TRY(hm_mjpeg_decode_run_dev(d, 1, files, sizes, d->d_out, nullptr, nullptr, fb, (uint64_t)d->W, 0, d->d_status, d->stream));
    uint32_t status = 0;
    HM_HIP(hipMemcpyAsync(&status, d->d_status, sizeof(status), hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipMemcpyAsync(out, d->d_out, fb, hipMemcpyDeviceToHost, d->stream));
    HM_HIP(hipStreamSynchronize(d->stream));
    if (bad) *bad = status;
    HM_ARG(!strict || status == 0, "hm_mjpeg_decode: %u bad restart intervals (malformed entropy-coded data)", status);
    return HM_OK;
}
