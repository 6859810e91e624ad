// The readout of a filter handle: views (hm_view*), the body-frame readout and its statistics (hm_body_*, hm_body_stats_*),
// the deformation readout (hm_strain_*, hm_view_strain*) and the flow tool's preview (the Motion-JPEG encoder and decoder,
// which work on handles of their own, are in mjpeg.hip).  Host orchestration and C-ABI
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

// the finished map, lent to hm_deep_body_* (hm_types.h)
int body_map_view(hm_ctx *h, BodyMapView *v)
{
    HM_JOIN_LAZY(h);                             // (body_map_build creates resources: the helper must not be queueing)
    HM_TRY(body_map_build(h));
    *v = BodyMapView{h->device, h->W, h->H, h->N, h->T, h->body.tri, h->body.bary, h->body.tidx, h->body.deep_col_entries};
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
