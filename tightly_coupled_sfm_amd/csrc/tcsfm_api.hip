// tcsfm_api.hip -- C ABI (include/tcsfm.h) over the gfx950 kernels in kernels.h.
// Host logic only: create / destroy / stream entries and the operator entry points.  The handle, staging and the argument checks are
// context.h's, over the owners and guard bands of device_owned.h.  The drivers are headers of this translation unit, included where their
// helpers are first needed: pose_host.h (the pose modes), dense_host.h (the dense modes), call_host.h (graph replay, queued calls, lanes),
// sequence_host.h and the networks' hosts.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <chrono>
#include <math.h>

#include "../../include/tcsfm.h"
#include "arg_overlap.h"
#include "kernels.h"
#include "dense_kernel.h"
#include "joint_kernel.h"
#include "dense_ref_kernel.h"
#include "scale_kernel.h"
#include "frame_scale_kernel.h"
#include "posenet_kernel.h"
#include "depthnet_kernel.h"
#include "depthnet_grad_kernel.h"
#include "posenet_grad_kernel.h"
#include "posenet_wgrad_kernel.h"
#include "warp_grad_kernel.h"
#include "photo_grad_kernel.h"
#include "loss_grad_kernel.h"
#include "window_loss_kernel.h"
#include "optim_kernel.h"
#include "frames_u8_kernel.h"
#include "resize_u8_kernel.h"
#include "disp_post_kernel.h"
#include "depth_eval_kernel.h"
#include "dense_plan.h"
#include "call_plan.h"

using namespace tc;

#include "context.h"       // the handle (tcsfm_ctx) over the owners of device_owned.h, HIPCHK / RESERVE, fail, Staging, ProfScope

#include "pose_host.h"      // the pose modes: launch helpers, PoseDriver, pose_refine / pose_evaluate

namespace {

// tiny export kernel of tcsfm_linearize_dense_window: d loss / d rho = a_f x the joint kernel's per-pixel record
__global__ __launch_bounds__(256) void k_dref_export_grho(const float *jrec, int jrec_stride, const double *exp_out, int exp_stride, float *out, int hw) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= hw) return;
    out[(size_t)b * hw + idx] = (float)(exp_out[(size_t)b * exp_stride + 1] * (double)jrec[((size_t)b * hw + idx) * jrec_stride]);
}

}  // namespace

#include "dense_host.h"

// shared body of tcsfm_refine_dense (win_B == 0), tcsfm_refine_dense_window and the merged sequence of queued dense calls (m: per-pair
// Gauss-Newton form or reference loss only, every array comes per call from the tables and `a` is the first call's): the argument checks
// and the staging; the launches are the three drivers' (dense_host.h)
static int dense_body(tcsfm_handle h, const tcsfm_opts *o, int N, int win_B, int win_S, const CallArgs &a, const WinOff *wo, bool depth_on_input = false,
                      const MergedCalls *m = nullptr) {
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!a.tgt || !a.src || !a.depth_t || !a.depth_s || !a.pose_in || !a.pose_out || !a.depth_out || !a.K) return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: NULL argument");
    const bool ref_mode = win_B && o->window_rule == TCSFM_WINDOW_REFERENCE;      // the reference's own loss (dense_ref_kernel.h)
    if (o->w_dc > 0.f && !ref_mode) return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: w_dc must be 0 (use prior_depth), except under window_rule = TCSFM_WINDOW_REFERENCE");
    if (ref_mode && (win_S > JMAXS || o->solver != TCSFM_SOLVER_GN || !(o->prior_init >= 0.f)))
        return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense_window: window_rule REFERENCE needs S <= 4, the Gauss-Newton solver and prior_init >= 0");
    if (!(o->w_pose_consist >= 0.f) || (o->w_pose_consist > 0.f && (!ref_mode || o->param != TCSFM_PARAM_SE3)))
        return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: w_pose_consist needs the window form under window_rule = TCSFM_WINDOW_REFERENCE and the SE(3) chart");
    if (o->free_source_depths != 0 && !ref_mode)
        return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: free_source_depths needs the window form under window_rule = TCSFM_WINDOW_REFERENCE");
    if (!(o->w_smooth >= 0.f) || (o->w_smooth > 0.f && !ref_mode))
        return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: w_smooth needs the window form under window_rule = TCSFM_WINDOW_REFERENCE");
    if (o->depth_param != TCSFM_DEPTH_FULL && !(o->depth_param == TCSFM_DEPTH_QUARTER && ref_mode && h->H % 4 == 0 && h->W % 4 == 0))
        return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: depth_param QUARTER needs window_rule = TCSFM_WINDOW_REFERENCE (window form) and H, W multiples of 4");
    if (o->param != TCSFM_PARAM_SE3) return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense: SE(3) chart only");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    Staging st(h, o);
    if (st.rc) return st.rc;
    const PosePlan pl = pose_plan_of(o, N, win_B, win_S, m);      // (the image sets and extents of a dense call are the pose call's)
    if (!m && (rc = check_intrinsics(h, o, a.K, pl.nimg_t))) return rc;
    const size_t hw = (size_t)h->H * h->W;
    if (m && !ref_mode && (pl.n_sel || o->solver != TCSFM_SOLVER_GN || o->host_ptrs || o->n_iters < 1 || (o->dense_joint && win_S >= 2)))
        return fail(h, TCSFM_E_ARG, "internal: only per-pair Gauss-Newton dense calls on device pointers are merged");
    if (m && ref_mode && (o->host_ptrs || o->n_iters < 1 || a.stats_out)) return fail(h, TCSFM_E_ARG, "internal: merged reference-loss calls take device pointers and no statistics");
    const float *d_tgt = st.in("tgt", a.tgt, pl.tgt(hw)), *d_src = st.in("src", a.src, pl.src(hw)), *d_dt = st.in("depth_t", a.depth_t, pl.depth_t(hw));
    const float *d_ds = st.in("depth_s", a.depth_s, pl.depth_s(hw)), *d_K = st.in("K", a.K, pl.K()), *d_pose_in = st.in("pose_in", a.pose_in, pl.pose());
    float *d_pose_out = st.out("pose_out", a.pose_out, pl.pose()), *d_depth_out = st.out("depth_out", a.depth_out, pl.maps(hw)), *d_stats = st.out("stats_out", a.stats_out, pl.stats());
    if (st.ready(nullptr)) return st.rc;
    if (d_stats) HIPCHK(h, hipMemsetAsync(d_stats, 0, pl.stats() * sizeof(float), h->stream));
    const DenseCall c{h, o, win_B ? win_B : N, win_S, d_tgt, d_src, d_dt, d_ds, d_K, d_pose_in, d_pose_out, d_depth_out, d_stats, wo, m ? &m->ct : nullptr, m ? m->pose_out : nullptr, m ? m->depth_out : nullptr, depth_on_input, nullptr};
    if (ref_mode) rc = dense_ref_run(c);
    // one depth map per target, 6S x 6S reduced system (joint_kernel.h); the library's own joint mode stays at S <= JMAXS_OWN = 3: wider windows
    // there keep the per-pair depth copies of the pair form
    else if (win_B && o->dense_joint && win_S >= 2 && win_S <= JMAXS_OWN) rc = dense_joint_run(c);
    else rc = dense_pair_run(c);
    if (rc) return rc;
    return st.finish();
}

#include "call_host.h"      // the routing of the refine calls: graph replay, the queue of the *_queued entries, lanes

// =================================================================================================
// Entry points: include/tcsfm.h declares every one of them extern "C", so the definitions below have C linkage.
void tcsfm_default_opts(tcsfm_opts *o) {
    memset(o, 0, sizeof(*o));
    o->n_iters = 4; o->solver = TCSFM_SOLVER_GN; o->param = TCSFM_PARAM_SE3; o->refine = TCSFM_REFINE_POSE;
    o->automask = 1; o->depth_is_disp = 0; o->host_ptrs = 0;
    o->w_l1 = 0.15f; o->w_ssim = 0.85f; o->w_dc = 0.f; o->irls_eps = 1e-3f;
    o->lambda0 = 1e-4f; o->lambda_up = 10.f; o->lambda_down = 0.1f; o->lambda_min = 1e-5f;
    o->min_depth = 0.06f; o->max_depth = 2.67f;
    o->prior_scale = 1.0f;
    o->lambda_depth = 1.0f; o->prior_depth = 10.0f;
    o->window_rule = TCSFM_WINDOW_PAIR; o->dense_joint = 1;
    o->prior_init = 0.1f;
    o->depth_param = TCSFM_DEPTH_FULL;
    o->w_pose_consist = 0.f;
    o->w_smooth = 0.f;
    o->free_source_depths = 0;
}

int tcsfm_algorithmic_bytes_per_pixel(const tcsfm_opts *) { return 32; }

const char *tcsfm_last_error(tcsfm_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int tcsfm_create(tcsfm_handle *out, int device, int H, int W, int max_pairs) {
    if (!out) return TCSFM_E_ARG;
    *out = nullptr;
    // (the warp gathers address a bordered image with 32-bit byte offsets -- tap4_fetch: (H + 2)(W + 2) 16 B must stay below 4 GiB)
    if (H < 4 || W < 4 || H > 16384 || W > 16384 || max_pairs < 1 || (size_t)H * W * max_pairs > ((size_t)1 << 33) ||
        (size_t)(H + 2) * (W + 2) >= ((size_t)1 << 28)) {
        g_create_error = "tcsfm_create: bad sizes";
        return TCSFM_E_ARG;
    }
    tcsfm_ctx *h = new tcsfm_ctx();
    h->device = device; h->H = H; h->W = W; h->max_pairs = h->queue.max_pairs = max_pairs;
    h->tiles_x = (W + TILE_W - 1) / TILE_W; h->tiles_y = (H + TILE_H - 1) / TILE_H;
    const DenseCaps &cp = h->caps = dense_caps(H, W, max_pairs);      // (dense_plan.h: the pose grid and what the record buffers below hold per pair)
    h->nblk = cp.nblk; h->ngrp = cp.ngrp; h->nblk_alloc = cp.nblk_alloc; h->ngrp_alloc = cp.ngrp_alloc; h->ngrp_pad = cp.ngrp_pad;
    size_t hw = (size_t)H * W, n = max_pairs;
    DeviceGuard dev_guard(device);
    int cur = -1;
    hipError_t e = hipGetDevice(&cur);
    if (e == hipSuccess && cur != device) e = hipErrorInvalidDevice;
    if (e == hipSuccess) e = h->own_stream.create();
    if (e == hipSuccess) e = h->err_word.create();
    h->stream = h->own_stream;
    if (e == hipSuccess) e = DEV_RESERVE(h->tgtpack, n * hw);
    if (e == hipSuccess) e = DEV_RESERVE(h->srcpack, n * (size_t)(H + 2) * (W + 2));   // zero-bordered
    if (e == hipSuccess) e = DEV_RESERVE(h->depth_work, n * hw);
    if (e == hipSuccess) e = DEV_RESERVE(h->partials, n * h->ngrp_pad * kMaxAcc);
    if (e == hipSuccess) e = hipMemset(h->partials, 0, n * h->ngrp_pad * kMaxAcc * sizeof(float));  // pad records stay 0
    if (e == hipSuccess) e = DEV_RESERVE(h->blockrec, n * h->nblk_alloc * kMaxAcc);
    if (e == hipSuccess) e = DEV_RESERVE(h->tickets, n * h->ngrp_alloc);
    if (e == hipSuccess) e = hipMemset(h->tickets, 0, n * h->ngrp_alloc * sizeof(int));
    if (e == hipSuccess) e = DEV_RESERVE(h->state, n);
    if (e == hipSuccess) e = DEV_RESERVE(h->pconst, n);
    if (e == hipSuccess) e = DEV_RESERVE(h->lin_out, n * kLinOut);
    if (e == hipSuccess) e = DEV_RESERVE(h->pose_dev, n * 6);
    if (e == hipSuccess) e = DEV_RESERVE(h->ls_dev, n);
    if (e == hipSuccess) e = DEV_RESERVE(h->K_dev, n * 9);
    if (e == hipSuccess) e = DEV_RESERVE(h->pair_idx, 2 * n);
    if (e == hipSuccess) e = DEV_RESERVE(h->pose_lin, 2 * n * 12);
    if (e != hipSuccess) {
        g_create_error = std::string("tcsfm_create: ") + hipGetErrorString(e);
        tcsfm_destroy(h);
        return e == hipErrorOutOfMemory ? TCSFM_E_NOMEM : TCSFM_E_HIP;
    }
    if (getenv("TCSFM_DEBUG_STAMPS") && DEV_RESERVE(h->dbg_stamps, 8) == hipSuccess) (void)hipMemset(h->dbg_stamps, 0, 8 * sizeof(long long));
    *out = h;
    return TCSFM_OK;
}

// The sequence is the contract: queued calls run, the lanes go, every stream that work may be on is drained, the graphs are dropped --
// and only then do the handle's members release themselves (tcsfm_ctx: buffers and events before the streams).
void tcsfm_destroy(tcsfm_handle h) {
    if (!h) return;
    (void)drain_queued(h);                // queued calls are not dropped: they run, and the synchronisations below wait for them
    for (tcsfm_ctx *c : h->lanes) tcsfm_destroy(c);
    h->lanes.clear();
    DeviceGuard dev_guard(h->device);
    for (hipStream_t s : {(hipStream_t)h->seq_copy, (hipStream_t)h->aux_stream, (hipStream_t)h->seq_pack})
        if (s) (void)hipStreamSynchronize(s);
    drop_graphs(h);                       // (a replay may still be running: it drains the streams one can be on before the executables go)
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    delete h;
}

int tcsfm_set_stream(tcsfm_handle h, void *hip_stream) {
    if (!h) return TCSFM_E_ARG;
    if ((hipStream_t)hip_stream != h->stream)           // queued calls were noted while bound to the old stream: they run there, behind its producers
        if (int rc_q = drain_queued(h)) return rc_q;
    if ((hipStream_t)hip_stream != h->stream && !h->graphs.entries.empty()) {   // captured calls may still be running on the old stream, and a graph
        DeviceGuard dev_guard(h->device);                              // captured there is not replayed on another producer's stream
        drop_graphs(h);
    }
    h->stream = (hipStream_t)hip_stream;  // NULL = legacy default stream
    k_forget(h);                          // a new stream is a new producer of the caller's buffers: validate intrinsics again
    return TCSFM_OK;
}

int tcsfm_use_own_stream(tcsfm_handle h) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    h->stream = h->own_stream;
    return TCSFM_OK;
}

int tcsfm_synchronize(tcsfm_handle h) {
    if (!h) return TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = flush_pending(h)) return rc_;          // queued calls (tcsfm_refine_window_queued) are launched first
    if (int rc_ = join_coalesce_lanes(h)) return rc_;    // (merged sequences that ran on lanes: the handle's stream waits for them)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (tcsfm_ctx *c : h->lanes)
        if (int rc_ = pending_error(c)) { h->err = c->err; return rc_; }
    return pending_error(h);
}

int tcsfm_disp_to_depth(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, float *scaled, float *depth) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !disp || n < 1) return fail(h, TCSFM_E_ARG, "tcsfm_disp_to_depth: bad argument");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    Staging st(h, o);
    const float *d_in = st.in("disp", disp, (size_t)n);
    float *d_s = st.out("scaled_disp", scaled, (size_t)n), *d_d = st.out("depth", depth, (size_t)n);
    st.bless("scaled_disp", "disp"); st.bless("depth", "disp");      // k_disp_to_depth: a thread loads disp[i] before it stores element i
    if (st.ready("tcsfm_disp_to_depth")) return st.rc;
    hipLaunchKernelGGL(k_disp_to_depth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_in, d_s, d_d, (long long)n,
                       1.f / o->max_depth, 1.f / o->min_depth);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_ssim(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, float *out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !x || !y || !out || planes < 1) return fail(h, TCSFM_E_ARG, "tcsfm_ssim: bad argument");
    Staging st(h, o);
    size_t hw = (size_t)h->H * h->W, n = hw * planes;
    const float *d_x = st.in("x", x, n), *d_y = st.in("y", y, n);
    float *d_o = st.out("out", out, n);
    if (st.ready("tcsfm_ssim")) return st.rc;
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)((hw + 255) / 256), planes), dim3(256), 0, h->stream, d_x, d_y, d_o, h->H, h->W);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_disp_to_depth_backward(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, const float *g_scaled, const float *g_depth,
                                 float *g_disp) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !disp || !g_disp || n < 1) return fail(h, TCSFM_E_ARG, "tcsfm_disp_to_depth_backward: bad argument");
    if (!g_scaled && !g_depth) return fail(h, TCSFM_E_ARG, "tcsfm_disp_to_depth_backward: no cotangent given");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    Staging st(h, o);
    const float *d_in = st.in("disp", disp, (size_t)n), *d_gs = st.in("g_scaled", g_scaled, (size_t)n), *d_gd = st.in("g_depth", g_depth, (size_t)n);
    float *d_out = st.out("g_disp", g_disp, (size_t)n);
    // k_disp_to_depth_bwd: a thread loads its float4 (or tail element) of all three inputs before its one store to the same elements
    st.bless("g_disp", "disp"); st.bless("g_disp", "g_scaled"); st.bless("g_disp", "g_depth");
    if (st.ready("tcsfm_disp_to_depth_backward")) return st.rc;
    // float4 accesses need 16-byte alignment of every array in use: otherwise the scalar tail takes everything
    const bool aligned = (((uintptr_t)d_in | (uintptr_t)d_gs | (uintptr_t)d_gd | (uintptr_t)d_out) & 15) == 0;
    const long long n4 = aligned ? (long long)(n / 4) : 0, threads = n4 + ((long long)n - 4 * n4);
    hipLaunchKernelGGL(k_disp_to_depth_bwd, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, d_in, d_gs, d_gd, d_out,
                       (long long)n, n4, 1.f / o->max_depth, 1.f / o->min_depth);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_ssim_backward(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, const float *g_out, float *g_x,
                        float *g_y) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !x || !y || !g_out || planes < 1) return fail(h, TCSFM_E_ARG, "tcsfm_ssim_backward: bad argument");
    if (!g_x && !g_y) return fail(h, TCSFM_E_ARG, "tcsfm_ssim_backward: no output wanted");
    if (planes > 65535) return fail(h, TCSFM_E_ARG, "tcsfm_ssim_backward: more than 65535 planes");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W, n = hw * planes;
    SsimGradParams P;
    P.x = st.in("x", x, n); P.y = st.in("y", y, n); P.g_out = st.in("g_out", g_out, n);
    P.g_x = st.out("g_x", g_x, n); P.g_y = st.out("g_y", g_y, n);
    P.H = h->H; P.W = h->W;
    if (st.ready("tcsfm_ssim_backward")) return st.rc;
    const dim3 grid((unsigned)((h->W + PG_TW - 1) / PG_TW), (unsigned)((h->H + PG_TH - 1) / PG_TH), (unsigned)planes);
    hipLaunchKernelGGL(k_ssim_bwd, grid, dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_warp(tcsfm_handle h, const tcsfm_opts *o, int N, const float *src, const float *depth_t, const float *depth_s,
               const float *pose, const float *K, float *img_rec, float *valid, float *proj_depth, float *comp_depth) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!src || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_warp: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp takes depth maps (call tcsfm_disp_to_depth first)");
    size_t hw = (size_t)h->H * h->W;
    const float *d_src = st.in("src", src, N * 3 * hw), *d_dt = st.in("depth_t", depth_t, N * hw), *d_ds = st.in("depth_s", depth_s, N * hw);
    const float *d_pose = st.in("pose", pose, (size_t)N * 6), *d_K = st.in("K", K, (size_t)N * 9);
    float *d_rec = st.out("img_rec", img_rec, N * 3 * hw), *d_valid = st.out("valid", valid, N * hw), *d_pd = st.out("proj_depth", proj_depth, N * hw), *d_cd = st.out("comp_depth", comp_depth, N * hw);
    if (st.ready("tcsfm_warp")) return st.rc;
    if ((rc = run_init(h, o, N, d_pose, nullptr, d_K, 0))) return rc;
    WarpParams P;
    P.src = d_src; P.depth_t = d_dt; P.depth_s = d_ds; P.pc = h->pconst;
    P.rec = d_rec; P.valid = d_valid; P.pd = d_pd; P.cd = d_cd; P.H = h->H; P.W = h->W;
    P.tgt = nullptr; P.posenet_in = nullptr; P.win_B = 0; P.win_S = 0;
    hipLaunchKernelGGL(k_warp, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_warp_posenet_input(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                             const float *depth_s, const float *pose, const float *K, float *posenet_in, float *valid) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !src || !depth_t || !depth_s || !pose || !K || !posenet_in) return fail(h, TCSFM_E_ARG, "tcsfm_warp_posenet_input: NULL argument");
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp_posenet_input takes depth maps");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, N * 3 * hw), *d_src = st.in("src", src, N * 3 * hw), *d_dt = st.in("depth_t", depth_t, N * hw), *d_ds = st.in("depth_s", depth_s, N * hw);
    const float *d_pose = st.in("pose", pose, (size_t)N * 6), *d_K = st.in("K", K, (size_t)N * 9);
    float *d_out = st.out("posenet_in", posenet_in, N * 6 * hw), *d_valid = st.out("valid", valid, N * hw);
    if (st.ready("tcsfm_warp_posenet_input")) return st.rc;
    if ((rc = run_init(h, o, N, d_pose, nullptr, d_K, 0))) return rc;
    WarpParams P;
    P.src = d_src; P.depth_t = d_dt; P.depth_s = d_ds; P.pc = h->pconst;
    P.rec = nullptr; P.valid = d_valid; P.pd = nullptr; P.cd = nullptr; P.tgt = d_tgt; P.posenet_in = d_out; P.H = h->H; P.W = h->W;
    P.win_B = 0; P.win_S = 0;
    hipLaunchKernelGGL(k_warp, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

// The launches of the warp's backward on device pointers (shared by tcsfm_warp_backward and tcsfm_photometric_backward): cotangents may
// be null (= zero), outputs may be null (= not wanted).  `inited`: run_init has already formed this call's pair constants.
static int warp_backward_dev(tcsfm_ctx *h, const tcsfm_opts *o, int N, const float *d_src, const float *d_dt, const float *d_ds,
                             const float *d_pose_in, const float *d_K, const float *d_grec, const float *d_gpd, const float *d_gcd,
                             float *o_dt, float *o_ds, float *o_pose, bool inited) {
    int rc;
    const size_t hw = (size_t)h->H * h->W;
    const unsigned nblk = (unsigned)((hw + 255) / 256);
    if (!o_dt && !o_ds && !o_pose) return TCSFM_OK;
    if (o_pose) RESERVE(h, h->wgrad_rec, (size_t)h->max_pairs * nblk * 12);
    if (o_ds && d_gpd) RESERVE(h, h->wgrad_fix, (size_t)h->max_pairs * hw);
    if (o_ds && d_gpd) RESERVE(h, h->wgrad_gmax, (size_t)h->max_pairs);
    const dim3 grid(nblk, N);
    if (o_ds && !d_gpd) HIPCHK(h, hipMemsetAsync(o_ds, 0, N * hw * sizeof(float), h->stream));      // nothing flows into the source depth
    if (!o_dt && !o_pose && !(o_ds && d_gpd)) return TCSFM_OK;                                      // ... and nothing else is wanted: no kernel at all
    if (!inited && (rc = run_init(h, o, N, d_pose_in, nullptr, d_K, 0))) return rc;
    if (o_ds && d_gpd) {
        int lg_hw = 0;
        while (((size_t)1 << lg_hw) < hw) lg_hw++;
        HIPCHK(h, hipMemsetAsync(h->wgrad_fix, 0, N * hw * sizeof(long long), h->stream));
        HIPCHK(h, hipMemsetAsync(h->wgrad_gmax, 0, (size_t)N * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_warp_gmax, grid, dim3(256), 0, h->stream, d_gpd, h->wgrad_gmax, (int)hw);
        WarpScatterParams S;
        S.depth_t = d_dt; S.pc = h->pconst; S.g_pd = d_gpd; S.gmax = h->wgrad_gmax; S.fix = h->wgrad_fix; S.H = h->H; S.W = h->W; S.lg_hw = lg_hw;
        hipLaunchKernelGGL(k_warp_scatter, grid, dim3(256), 0, h->stream, S);
        hipLaunchKernelGGL(k_warp_fix_out, grid, dim3(256), 0, h->stream, (const long long *)h->wgrad_fix, (const unsigned *)h->wgrad_gmax, o_ds, (int)hw, lg_hw);
        HIPCHK(h, hipGetLastError());
    }
    if (o_dt || o_pose) {
        WarpGradParams P;
        P.src = d_src; P.depth_t = d_dt; P.depth_s = d_ds; P.pc = h->pconst; P.st = h->state; P.g_rec = d_grec; P.g_pd = d_gpd; P.g_cd = d_gcd;
        P.d_depth_t = o_dt; P.blockrec = o_pose ? h->wgrad_rec : nullptr; P.H = h->H; P.W = h->W;
        hipLaunchKernelGGL(k_warp_bwd, grid, dim3(256), 0, h->stream, P);
        if (o_pose) hipLaunchKernelGGL(k_warp_pose_tail, dim3(N), dim3(64), 0, h->stream, (const double *)h->wgrad_rec, (int)nblk, d_pose_in, d_K, o_pose);
        HIPCHK(h, hipGetLastError());
    }
    return TCSFM_OK;
}

int tcsfm_warp_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *src, const float *depth_t, const float *depth_s,
                        const float *pose, const float *K, const float *g_rec, const float *g_proj_depth, const float *g_comp_depth,
                        float *d_depth_t, float *d_depth_s, float *d_pose) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!src || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_warp_backward: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp_backward takes depth maps (call tcsfm_disp_to_depth first)");
    const size_t hw = (size_t)h->H * h->W;
    const float *d_src = st.in("src", src, N * 3 * hw), *d_dt = st.in("depth_t", depth_t, N * hw), *d_ds = st.in("depth_s", depth_s, N * hw);
    const float *d_pose_in = st.in("pose", pose, (size_t)N * 6), *d_K = st.in("K", K, (size_t)N * 9);
    const float *d_grec = st.in("g_rec", g_rec, N * 3 * hw), *d_gpd = st.in("g_proj_depth", g_proj_depth, N * hw), *d_gcd = st.in("g_comp_depth", g_comp_depth, N * hw);
    float *o_dt = st.out("d_depth_t", d_depth_t, N * hw), *o_ds = st.out("d_depth_s", d_depth_s, N * hw), *o_pose = st.out("d_pose", d_pose, (size_t)N * 6);
    if (st.ready("tcsfm_warp_backward")) return st.rc;
    if ((rc = warp_backward_dev(h, o, N, d_src, d_dt, d_ds, d_pose_in, d_K, d_grec, d_gpd, d_gcd, o_dt, o_ds, o_pose, false))) return rc;
    return st.finish();
}

// k_photo_bwd on device pointers.  A requested output whose cotangent is absent is zeroed without a launch.
static int photo_maps_backward_dev(tcsfm_ctx *h, const tcsfm_opts *o, int N, const float *d_tgt, const float *d_rec, const float *d_pd,
                                   const float *d_cd, const float *d_gdiff, const float *d_gweight, const float *d_grec_add,
                                   float *o_grec, float *o_gpd, float *o_gcd) {
    const size_t hw = (size_t)h->H * h->W;
    const bool rec_on = o_grec && d_gdiff, dep_on = (o_gpd || o_gcd) && d_gweight;
    if (o_grec && !rec_on) HIPCHK(h, hipMemsetAsync(o_grec, 0, N * 3 * hw * sizeof(float), h->stream));
    if (o_gpd && !dep_on) HIPCHK(h, hipMemsetAsync(o_gpd, 0, N * hw * sizeof(float), h->stream));
    if (o_gcd && !dep_on) HIPCHK(h, hipMemsetAsync(o_gcd, 0, N * hw * sizeof(float), h->stream));
    if (!rec_on && !dep_on) return TCSFM_OK;
    PhotoGradParams P;
    P.tgt = d_tgt; P.rec = d_rec; P.pd = d_pd; P.cd = d_cd;
    P.g_diff = rec_on ? d_gdiff : nullptr; P.g_weight = dep_on ? d_gweight : nullptr; P.g_rec_add = d_grec_add;
    P.g_rec = rec_on ? o_grec : nullptr; P.g_pd = dep_on ? o_gpd : nullptr; P.g_cd = dep_on ? o_gcd : nullptr;
    P.H = h->H; P.W = h->W; P.wl = o->w_l1 / 3.f; P.ws = o->w_ssim / 3.f;
    const dim3 grid((unsigned)((h->W + PG_TW - 1) / PG_TW), (unsigned)((h->H + PG_TH - 1) / PG_TH), (unsigned)N);
    hipLaunchKernelGGL(k_photo_bwd, grid, dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int tcsfm_photometric_maps_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *img_rec, const float *proj_depth,
                                    const float *comp_depth, const float *g_diff, const float *g_weight, float *g_rec, float *g_proj_depth,
                                    float *g_comp_depth) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !img_rec || !proj_depth || !comp_depth) return fail(h, TCSFM_E_ARG, "tcsfm_photometric_maps_backward: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    const size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, N * 3 * hw), *d_rec = st.in("img_rec", img_rec, N * 3 * hw), *d_pd = st.in("proj_depth", proj_depth, N * hw), *d_cd = st.in("comp_depth", comp_depth, N * hw);
    const float *d_gdiff = st.in("g_diff", g_diff, N * hw), *d_gweight = st.in("g_weight", g_weight, N * hw);
    float *o_grec = st.out("g_rec", g_rec, N * 3 * hw), *o_gpd = st.out("g_proj_depth", g_proj_depth, N * hw), *o_gcd = st.out("g_comp_depth", g_comp_depth, N * hw);
    if (st.ready("tcsfm_photometric_maps_backward")) return st.rc;
    if ((rc = photo_maps_backward_dev(h, o, N, d_tgt, d_rec, d_pd, d_cd, d_gdiff, d_gweight, nullptr, o_grec, o_gpd, o_gcd))) return rc;
    return st.finish();
}

int tcsfm_photometric_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                               const float *depth_s, const float *pose, const float *K, const float *g_diff, const float *g_weight,
                               const float *g_img_rec, float *d_depth_t, float *d_depth_s, float *d_pose) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !src || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_photometric_backward: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_photometric_backward takes depth maps (call tcsfm_disp_to_depth first)");
    const size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, N * 3 * hw), *d_src = st.in("src", src, N * 3 * hw), *d_dt = st.in("depth_t", depth_t, N * hw), *d_ds = st.in("depth_s", depth_s, N * hw);
    const float *d_pose_in = st.in("pose", pose, (size_t)N * 6), *d_K = st.in("K", K, (size_t)N * 9);
    const float *d_gdiff = st.in("g_diff", g_diff, N * hw), *d_gweight = st.in("g_weight", g_weight, N * hw), *d_gimg = st.in("g_img_rec", g_img_rec, N * 3 * hw);
    float *o_dt = st.out("d_depth_t", d_depth_t, N * hw), *o_ds = st.out("d_depth_s", d_depth_s, N * hw), *o_pose = st.out("d_pose", d_pose, (size_t)N * 6);
    if (st.ready("tcsfm_photometric_backward")) return st.rc;
    if (!o_dt && !o_ds && !o_pose) return st.finish();
    // the cotangents that reach the warp: g_rec = (assembly's, from g_diff) + g_img_rec; g_proj_depth, g_comp_depth from g_weight
    const float *w_grec = d_gimg, *w_gpd = nullptr, *w_gcd = nullptr;
    bool inited = false;
    if (d_gdiff || d_gweight) {
        const size_t plane = (size_t)h->max_pairs * hw;
        RESERVE(h, h->pgrad_fwd, 5 * plane);
        RESERVE(h, h->pgrad_cot, 5 * plane);
        float *f_rec = h->pgrad_fwd, *f_pd = h->pgrad_fwd + 3 * plane, *f_cd = h->pgrad_fwd + 4 * plane;
        float *c_rec = h->pgrad_cot, *c_pd = h->pgrad_cot + 3 * plane, *c_cd = h->pgrad_cot + 4 * plane;
        if ((rc = run_init(h, o, N, d_pose_in, nullptr, d_K, 0))) return rc;
        inited = true;
        WarpFwd64Params P;
        P.src = d_src; P.depth_t = d_dt; P.depth_s = d_ds; P.pc = h->pconst; P.st = h->state;
        P.rec = d_gdiff ? f_rec : nullptr; P.pd = d_gweight ? f_pd : nullptr; P.cd = d_gweight ? f_cd : nullptr; P.H = h->H; P.W = h->W;
        hipLaunchKernelGGL(k_warp_fwd64, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, P);
        HIPCHK(h, hipGetLastError());
        if ((rc = photo_maps_backward_dev(h, o, N, d_tgt, f_rec, f_pd, f_cd, d_gdiff, d_gweight, d_gimg, d_gdiff ? c_rec : nullptr,
                                          d_gweight ? c_pd : nullptr, d_gweight ? c_cd : nullptr))) return rc;
        if (d_gdiff) w_grec = c_rec;
        if (d_gweight) { w_gpd = c_pd; w_gcd = c_cd; }
    }
    if ((rc = warp_backward_dev(h, o, N, d_src, d_dt, d_ds, d_pose_in, d_K, w_grec, w_gpd, w_gcd, o_dt, o_ds, o_pose, inited))) return rc;
    return st.finish();
}

int tcsfm_photometric(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                      const float *depth_s, const float *pose, const float *K, float *diff, float *valid, float *weight,
                      float *auto_err, float *auto_mask, float *img_rec) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !src || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_photometric: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, N * 3 * hw), *d_src = st.in("src", src, N * 3 * hw), *d_dt = st.in("depth_t", depth_t, N * hw), *d_ds = st.in("depth_s", depth_s, N * hw);
    const float *d_pose = st.in("pose", pose, (size_t)N * 6), *d_K = st.in("K", K, (size_t)N * 9);
    float *outs[6] = {diff, valid, weight, auto_err, auto_mask, img_rec}, *d_out[6];
    static const char *const out_names[6] = {"diff", "valid", "weight", "auto_err", "auto_mask", "img_rec"};
    for (int i = 0; i < 6; i++) d_out[i] = st.out(out_names[i], outs[i], (i == 5 ? 3 : 1) * N * hw);
    if (st.ready("tcsfm_photometric")) return st.rc;
    if ((rc = run_pack(h, o, N, d_tgt, d_src, d_dt, d_ds))) return rc;
    if ((rc = run_init(h, o, N, d_pose, nullptr, d_K, 0))) return rc;
    LinParams P = lin_params(h, o, 6);
    P.o_diff = d_out[0]; P.o_valid = d_out[1]; P.o_weight = d_out[2]; P.o_auto_err = d_out[3]; P.o_auto_mask = d_out[4]; P.o_rec = d_out[5];
    launch_lin(h, P, N, 6, false, MODE_MAPS);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_linearize(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                    const float *depth_s, const float *pose, const float *log_scale, const float *K, double *Hmat, double *g,
                    double *stats) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !src || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_linearize: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    size_t hw = (size_t)h->H * h->W;
    PoseCall c{h, o, N, 0, 0};
    c.tgt = st.in("tgt", tgt, N * 3 * hw); c.src = st.in("src", src, N * 3 * hw); c.dt = st.in("depth_t", depth_t, N * hw); c.ds = st.in("depth_s", depth_s, N * hw);
    c.pose_in = st.in("pose", pose, (size_t)N * 6); c.K = st.in("K", K, (size_t)N * 9); c.ls_in = st.in("log_scale", log_scale, (size_t)N);
    {
        const size_t np_ = (size_t)np_of(o);
        st.host_out("Hmat", Hmat, N * np_ * np_ * sizeof(double)); st.host_out("g", g, N * np_ * sizeof(double)); st.host_out("stats", stats, (size_t)N * 4 * sizeof(double));
    }
    if (st.ready("tcsfm_linearize")) return st.rc;
    std::vector<double> host;
    if ((rc = pose_evaluate(c, N, MODE_LIN, host))) return rc;
    unpack_lin_records(host, N, np_of(o), Hmat, g, stats);
    return TCSFM_OK;
}

int tcsfm_linearize_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                           const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *log_scale,
                           double *Hmat, double *g, double *stats) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (B < 1 || S < 1 || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_linearize_window: need 1 <= 2*B*S <= max_pairs");
    const int N = 2 * B * S;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !srcs || !depth_t || !depth_s || !pose || !K) return fail(h, TCSFM_E_ARG, "tcsfm_linearize_window: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, B))) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const int np = np_of(o);
    PoseCall c{h, o, N, B, S};
    c.tgt = st.in("tgt", tgt, B * 3 * hw); c.src = st.in("srcs", srcs, (size_t)B * S * 3 * hw); c.dt = st.in("depth_t", depth_t, B * hw);
    c.ds = st.in("depth_s", depth_s, (size_t)B * S * hw); c.K = st.in("K", K, (size_t)B * 9); c.pose_in = st.in("pose", pose, (size_t)N * 6);
    const float *d_ls = st.in("log_scale", log_scale, (size_t)N);
    c.ls_in = np == 7 ? d_ls : nullptr;
    st.host_out("Hmat", Hmat, (size_t)N * np * np * sizeof(double)); st.host_out("g", g, (size_t)N * np * sizeof(double));
    st.host_out("stats", stats, (size_t)N * 4 * sizeof(double));
    if (st.ready("tcsfm_linearize_window")) return st.rc;
    std::vector<double> host;
    if ((rc = pose_evaluate(c, N, MODE_LIN, host))) return rc;
    unpack_lin_records(host, N, np, Hmat, g, stats);
    return TCSFM_OK;
}

int tcsfm_loss_surface(tcsfm_handle h, const tcsfm_opts *o, const float *tgt, const float *src, const float *depth_t,
                       const float *depth_s, const float *K, int P, const float *poses, double *cost_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, P);
    if (rc) return rc;
    if (!tgt || !src || !depth_t || !depth_s || !poses || !K || !cost_out) return fail(h, TCSFM_E_ARG, "tcsfm_loss_surface: NULL argument");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, 1))) return rc;
    size_t hw = (size_t)h->H * h->W;
    tcsfm_opts oo = *o;
    oo.refine = TCSFM_REFINE_POSE;
    PoseCall c{h, &oo, P, 0, 0};
    c.tgt = st.in("tgt", tgt, 3 * hw); c.src = st.in("src", src, 3 * hw); c.dt = st.in("depth_t", depth_t, hw); c.ds = st.in("depth_s", depth_s, hw);
    c.pose_in = st.in("poses", poses, (size_t)P * 6); c.K = st.in("K", K, (size_t)9); c.ls_in = nullptr;
    st.host_out("cost_out", cost_out, (size_t)P * sizeof(double));
    if (st.ready("tcsfm_loss_surface")) return st.rc;
    std::vector<double> host;
    if ((rc = pose_evaluate(c, 1, MODE_COST, host))) return rc;
    const int rec = 6 * 6 + 6 + 4;
    for (int i = 0; i < P; i++) cost_out[i] = host[(size_t)i * rec + 42];
    return TCSFM_OK;
}

int tcsfm_refine(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                 const float *depth_s, const float *K, const float *pose_in, const float *log_scale_in, float *pose_out,
                 float *log_scale_out, float *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    const CallArgs a{tgt, src, depth_t, depth_s, K, pose_in, log_scale_in, pose_out, log_scale_out, nullptr, stats_out};
    if (int rc_a = refine_overlap(h, "tcsfm_refine", o, N, 0, 0, a, false)) return rc_a;
    return refine_impl(h, o, N, 0, 0, a);
}

int tcsfm_refine_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                        const float *depth_t, const float *depth_s, const float *K, const float *pose_in,
                        const float *log_scale_in, float *pose_out, float *log_scale_out, float *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (B < 1 || S < 1 || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_refine_window: need 1 <= 2*B*S <= max_pairs");
    const CallArgs a{tgt, srcs, depth_t, depth_s, K, pose_in, log_scale_in, pose_out, log_scale_out, nullptr, stats_out};
    if (int rc_a = refine_overlap(h, "tcsfm_refine_window", o, 2 * B * S, B, S, a, false)) return rc_a;
    return refine_impl(h, o, 2 * B * S, B, S, a);
}

int tcsfm_scale_recovery(tcsfm_handle h, const tcsfm_opts *o, int N, const float *depth, const float *K, float real_cam_height,
                         int pad_to_batch, float *scale_out, float *median_out, float *height_out, float *mask_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!depth || !K || !scale_out) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery: NULL argument");
    if (h->H < 5 || h->W < 5) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery: image too small");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, N))) return rc;
    const size_t hw = (size_t)h->H * h->W;
    RESERVE(h, h->scale_keys, (size_t)h->max_pairs * hw);
    RESERVE(h, h->scale_hist, 260);
    const float *d_depth = st.in("depth", depth, N * hw), *d_K = st.in("K", K, (size_t)N * 9);
    float *d_scale = st.out("scale_out", scale_out, (size_t)1), *d_med = st.out("median_out", median_out, (size_t)1), *d_h = st.out("height_out", height_out, N * hw), *d_m = st.out("mask_out", mask_out, N * hw);
    if (st.ready("tcsfm_scale_recovery")) return st.rc;
    HIPCHK(h, hipMemsetAsync(h->scale_hist, 0, 260 * sizeof(unsigned), h->stream));
    GroundParams G;
    G.depth = d_depth; G.K = d_K; G.height = d_h; G.mask = d_m; G.keys = h->scale_keys; G.H = h->H; G.W = h->W; G.err = h->err_word.dev;
    hipLaunchKernelGGL(k_ground, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, G);
    // the reference pads the batch to config['minibatch'] with copies of image 0 (dnet_layers.py:307-311): weight image 0
    const int w0 = 1 + (pad_to_batch > N ? pad_to_batch - N : 0);
    unsigned *hist = h->scale_hist, *state = h->scale_hist + 256;
    const int nb = (int)((hw + 255) / 256) < 64 ? (int)((hw + 255) / 256) : 64;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_sel_hist, dim3(nb, N), dim3(256), 0, h->stream, (const unsigned *)h->scale_keys, (int)hw, w0,
                           (const unsigned *)state, shift, hist);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(64), 0, h->stream, hist, state, shift, real_cam_height, d_scale, d_med);
    }
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

// k_ground + k_median_frames over `n` depth planes on `stream`: two launches, one workgroup of the second per plane.
// TCSFM_MEDIAN_LDS_KEYS (measurement and test hook, read at every call): the masked keys a workgroup keeps in LDS after its first
// pass, 0 .. kMedianLdsKeys (the default); a frame with more reads its plane in every round.  The results do not depend on it.
static void launch_frame_scales(tcsfm_ctx *h, hipStream_t stream, int n, const float *depth, const float *K, int k_stride, unsigned *keys,
                                float real_cam_height, float *scale, float *median, int *count) {
    const size_t hw = (size_t)h->H * h->W;
    GroundParams G;
    G.depth = depth; G.K = K; G.height = nullptr; G.mask = nullptr; G.keys = keys; G.H = h->H; G.W = h->W; G.err = h->err_word.dev; G.k_stride = k_stride;
    hipLaunchKernelGGL(k_ground, dim3((unsigned)((hw + 255) / 256), n), dim3(256), 0, stream, G);
    const char *lds_env = getenv("TCSFM_MEDIAN_LDS_KEYS");
    const int lds_keys = lds_env ? atoi(lds_env) : kMedianLdsKeys;
    hipLaunchKernelGGL(k_median_frames, dim3(n), dim3(kMedianThreads), 0, stream, (const unsigned *)keys, (int)hw, lds_keys, real_cam_height, scale, median, count);
}

int tcsfm_scale_recovery_frames(tcsfm_handle h, const tcsfm_opts *o, int N, const void *depth, const void *K, float real_cam_height,
                                void *scale_out, void *median_out, int *count_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!depth || !K || !scale_out) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery_frames: NULL argument");
    if (h->H < 5 || h->W < 5) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery_frames: image too small");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery_frames: host_ptrs must be 0 (device pointers); a host caller has the sequence calls (tcsfm_sequence_scale)");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("depth", depth, (size_t)N * hw * sizeof(float)); a.in("K", K, (size_t)N * 9 * sizeof(float));
    a.out("scale_out", scale_out, (size_t)N * sizeof(float)); a.out("median_out", median_out, (size_t)N * sizeof(float));
    a.out("count_out", count_out, (size_t)N * sizeof(int));
    if ((rc = check_overlap(h, "tcsfm_scale_recovery_frames", a))) return rc;
    DeviceGuard dev_guard(h->device);
    if ((rc = pending_error(h))) return rc;
    if ((rc = check_intrinsics(h, o, (const float *)K, N))) return rc;
    RESERVE(h, h->scale_keys, (size_t)h->max_pairs * hw);
    RESERVE(h, h->scale_hist, 260);
    launch_frame_scales(h, h->stream, N, (const float *)depth, (const float *)K, 9, h->scale_keys, real_cam_height, (float *)scale_out,
                        (float *)median_out, count_out);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int tcsfm_smooth_loss(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, double *loss_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!disp || !img || !loss_out) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss: NULL argument");
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    const int nb = (int)((hw + 255) / 256);
    const float *d_disp = st.in("disp", disp, N * hw), *d_img = st.in("img", img, N * 3 * hw);
    // scratch: N means (double) + N * nb * 2 partial sums, carved from the next staging slot
    float *scratch = (float *)st.scratch(((size_t)N * 2 + (size_t)N * nb * 2) * sizeof(float));
    st.host_out("loss_out", loss_out, sizeof(double));
    if (st.ready("tcsfm_smooth_loss")) return st.rc;
    double *mean = reinterpret_cast<double *>(scratch);
    float *partial = scratch + (size_t)N * 2;
    hipLaunchKernelGGL(k_smooth_mean, dim3(N), dim3(1024), 0, h->stream, d_disp, (int)hw, mean);
    hipLaunchKernelGGL(k_smooth, dim3(nb, N), dim3(256), 0, h->stream, d_disp, d_img, (const double *)mean, h->H, h->W, partial);
    HIPCHK(h, hipGetLastError());
    std::vector<float> hp((size_t)N * nb * 2);
    HIPCHK(h, hipMemcpyAsync(hp.data(), partial, hp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double sx = 0.0, sy = 0.0;
    for (size_t i = 0; i < hp.size(); i += 2) { sx += hp[i]; sy += hp[i + 1]; }
    *loss_out = sx / ((double)N * h->H * (h->W - 1)) + sy / ((double)N * (h->H - 1) * h->W);
    return TCSFM_OK;
}

int tcsfm_smooth_loss_device(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, float *loss_out,
                             double *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!disp || !img || !loss_out || !stats_out) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_device: NULL argument");
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_device: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    const int nb = (int)((hw + 255) / 256);
    const float *d_disp = st.in("disp", disp, N * hw), *d_img = st.in("img", img, N * 3 * hw);
    float *d_loss = st.out("loss_out", loss_out, (size_t)1);
    double *d_stats = st.out("stats_out", stats_out, (size_t)N * 3);
    // scratch as in tcsfm_smooth_loss: N means (double) + N * nb * 2 partial sums
    float *scratch = (float *)st.scratch(((size_t)N * 2 + (size_t)N * nb * 2) * sizeof(float));
    if (st.ready("tcsfm_smooth_loss_device")) return st.rc;
    double *mean = reinterpret_cast<double *>(scratch);
    float *partial = scratch + (size_t)N * 2;
    hipLaunchKernelGGL(k_smooth_mean, dim3(N), dim3(1024), 0, h->stream, d_disp, (int)hw, mean);
    hipLaunchKernelGGL(k_smooth, dim3(nb, N), dim3(256), 0, h->stream, d_disp, d_img, (const double *)mean, h->H, h->W, partial);
    hipLaunchKernelGGL(k_smooth_reduce, dim3(1), dim3(256), 0, h->stream, (const float *)partial, (const double *)mean, N, nb, h->H, h->W,
                       d_stats, d_loss);
    HIPCHK(h, hipGetLastError());
    return st.finish();          // (device pointers: no copy, no synchronisation)
}

int tcsfm_smooth_loss_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, const double *stats,
                               const float *g_loss, float *g_disp) {
    if (int rc_q = drain_queued(h)) return rc_q;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!disp || !img || !stats || !g_loss || !g_disp) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_backward: NULL argument");
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_backward: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    SmoothGradParams P;
    P.disp = st.in("disp", disp, N * hw); P.img = st.in("img", img, N * 3 * hw); P.stats = st.in("stats", stats, (size_t)N * 3); P.g_loss = st.in("g_loss", g_loss, (size_t)1);
    P.g_disp = st.out("g_disp", g_disp, N * hw);
    P.H = h->H; P.W = h->W; P.N = N;
    if (st.ready("tcsfm_smooth_loss_backward")) return st.rc;
    hipLaunchKernelGGL(k_smooth_bwd, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

// the window loss (optimizer.py:47-86) and its backward: csrc/window_loss_kernel.h
static int window_loss_args(tcsfm_handle h, const tcsfm_opts *o, const char *who, int B, int S, int argmin, int inverse, const float *fwd_diff,
                            const float *fwd_valid, const float *fwd_weight, const float *fwd_auto_err, const float *inv_diff,
                            const float *inv_valid, const float *inv_weight, const float *inv_auto_mask) {
    if (!h) return TCSFM_E_ARG;
    const std::string w(who);
    if (S < 1 || S > WL_MAXS) return fail(h, TCSFM_E_ARG, (w + ": S must be 1 .. 4 source images per target").c_str());
    if (B < 1) return fail(h, TCSFM_E_ARG, (w + ": B must be at least 1").c_str());
    if (int rc = check_common(h, o, B * S)) return rc;
    if (!(o->w_dc >= 0.f)) return fail(h, TCSFM_E_ARG, (w + ": opts.w_dc must be >= 0").c_str());
    if (!fwd_diff || !fwd_valid || !fwd_weight || (argmin && o->automask && !fwd_auto_err))
        return fail(h, TCSFM_E_ARG, (w + ": NULL forward map").c_str());
    if (inverse && (!inv_diff || !inv_valid || !inv_weight || (o->automask && !inv_auto_mask)))
        return fail(h, TCSFM_E_ARG, (w + ": NULL inverse map").c_str());
    return TCSFM_OK;
}

static WindowLossParams window_loss_params(tcsfm_handle h, const tcsfm_opts *o, Staging &st, int B, int S, int argmin, int inverse,
                                           const float *fwd_diff, const float *fwd_valid, const float *fwd_weight, const float *fwd_auto_err,
                                           const float *inv_diff, const float *inv_valid, const float *inv_weight, const float *inv_auto_mask) {
    const size_t n = (size_t)S * B * h->H * h->W;
    WindowLossParams P;
    P.f_diff = st.in("fwd_diff", fwd_diff, n); P.f_valid = st.in("fwd_valid", fwd_valid, n); P.f_weight = st.in("fwd_weight", fwd_weight, n); P.f_ame = st.in("fwd_auto_err", fwd_auto_err, n);
    P.i_diff = st.in("inv_diff", inv_diff, n); P.i_valid = st.in("inv_valid", inv_valid, n); P.i_weight = st.in("inv_weight", inv_weight, n); P.i_am = st.in("inv_auto_mask", inv_auto_mask, n);
    P.B = B; P.S = S; P.hw = h->H * h->W; P.argmin = argmin ? 1 : 0; P.automask = o->automask ? 1 : 0; P.inverse = inverse ? 1 : 0;
    P.w = (double)o->w_dc;
    return P;
}

int tcsfm_window_loss(tcsfm_handle h, const tcsfm_opts *o, int B, int S, int argmin, int inverse, const float *fwd_diff, const float *fwd_valid,
                      const float *fwd_weight, const float *fwd_auto_err, const float *inv_diff, const float *inv_valid,
                      const float *inv_weight, const float *inv_auto_mask, float *loss_out, double *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (int rc = window_loss_args(h, o, "tcsfm_window_loss", B, S, argmin, inverse, fwd_diff, fwd_valid, fwd_weight, fwd_auto_err, inv_diff,
                                  inv_valid, inv_weight, inv_auto_mask)) return rc;
    if (!loss_out || !stats_out) return fail(h, TCSFM_E_ARG, "tcsfm_window_loss: NULL output");
    Staging st(h, o);
    WindowLossParams P = window_loss_params(h, o, st, B, S, argmin, inverse, fwd_diff, fwd_valid, fwd_weight, fwd_auto_err, inv_diff, inv_valid,
                                            inv_weight, inv_auto_mask);
    float *d_loss = st.out("loss_out", loss_out, (size_t)1);
    double *d_stats = st.out("stats_out", stats_out, (size_t)WL_NSTAT);
    const int nu = (P.hw >> 2) + (P.hw & 3), per = 256 * WL_UNITS, nbx = (nu + per - 1) / per;      // the grid: a function of the shape only
    double *partial = (double *)st.scratch((size_t)nbx * B * WL_NSUM * sizeof(double));
    if (st.ready("tcsfm_window_loss")) return st.rc;
    hipLaunchKernelGGL(k_window_loss, dim3(nbx, B), dim3(256), 0, h->stream, P, partial);
    hipLaunchKernelGGL(k_window_loss_final, dim3(1), dim3(256), 0, h->stream, (const double *)partial, nbx * B, P, d_stats, d_loss);
    HIPCHK(h, hipGetLastError());
    return st.finish();          // (device pointers: no copy, no synchronisation)
}

int tcsfm_window_loss_backward(tcsfm_handle h, const tcsfm_opts *o, int B, int S, int argmin, int inverse, const float *fwd_diff,
                               const float *fwd_valid, const float *fwd_weight, const float *fwd_auto_err, const float *inv_diff,
                               const float *inv_valid, const float *inv_weight, const float *inv_auto_mask, const double *stats,
                               const float *g_loss, float *g_fwd_diff, float *g_fwd_weight, float *g_inv_diff, float *g_inv_weight) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (int rc = window_loss_args(h, o, "tcsfm_window_loss_backward", B, S, argmin, inverse, fwd_diff, fwd_valid, fwd_weight, fwd_auto_err,
                                  inv_diff, inv_valid, inv_weight, inv_auto_mask)) return rc;
    if (!stats || !g_loss) return fail(h, TCSFM_E_ARG, "tcsfm_window_loss_backward: NULL argument");
    if (!g_fwd_diff && !g_fwd_weight && !g_inv_diff && !g_inv_weight) return fail(h, TCSFM_E_ARG, "tcsfm_window_loss_backward: no output requested");
    Staging st(h, o);
    WindowLossGradParams G;
    G.in = window_loss_params(h, o, st, B, S, argmin, inverse, fwd_diff, fwd_valid, fwd_weight, fwd_auto_err, inv_diff, inv_valid, inv_weight,
                              inv_auto_mask);
    const size_t n = (size_t)S * B * G.in.hw;
    G.stats = st.in("stats", stats, (size_t)WL_NSTAT); G.g_loss = st.in("g_loss", g_loss, (size_t)1);
    G.g_f_diff = st.out("g_fwd_diff", g_fwd_diff, n); G.g_f_weight = st.out("g_fwd_weight", g_fwd_weight, n); G.g_i_diff = st.out("g_inv_diff", g_inv_diff, n); G.g_i_weight = st.out("g_inv_weight", g_inv_weight, n);
    if (st.ready("tcsfm_window_loss_backward")) return st.rc;
    const int nu = (G.in.hw >> 2) + (G.in.hw & 3);
    hipLaunchKernelGGL(k_window_loss_bwd, dim3((nu + 255) / 256, B), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_refine_dense(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                       const float *depth_s, const float *K, const float *pose_in, float *pose_out, float *depth_out,
                       float *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    const CallArgs a{tgt, src, depth_t, depth_s, K, pose_in, nullptr, pose_out, nullptr, depth_out, stats_out};
    bool on_input = false;
    if (int rc_a = refine_overlap(h, "tcsfm_refine_dense", o, N, 0, 0, a, true, &on_input)) return rc_a;
    return dense_impl(h, o, N, 0, 0, a, nullptr, on_input);
}

int tcsfm_refine_dense_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                              const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out,
                              float *depth_out, float *stats_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (B < 1 || S < 1 || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense_window: need 1 <= 2*B*S <= max_pairs");
    const CallArgs a{tgt, srcs, depth_t, depth_s, K, pose_in, nullptr, pose_out, nullptr, depth_out, stats_out};
    bool on_input = false;
    if (int rc_a = refine_overlap(h, "tcsfm_refine_dense_window", o, 2 * B * S, B, S, a, true, &on_input)) return rc_a;
    return dense_impl(h, o, 2 * B * S, B, S, a, nullptr, on_input);
}

static int linearize_dense_window_impl(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                       const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *depth0,
                                       double *scal_out, double *g_pose_out, float *g_rho_out, float *g_rho_src_out, const char *entry) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (B < 1 || S < 1 || S > JMAXS || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_linearize_dense_window: need 1 <= S <= 4 and 2*B*S <= max_pairs");
    const int N = 2 * B * S;
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!tgt || !srcs || !depth_t || !depth_s || !K || !pose || !scal_out || !g_pose_out || !g_rho_out) return fail(h, TCSFM_E_ARG, "tcsfm_linearize_dense_window: NULL argument");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth) || !(o->prior_init >= 0.f)) return fail(h, TCSFM_E_ARG, "min_depth / max_depth / prior_init invalid");
    Staging st(h, o);
    if (st.rc) return st.rc;
    if ((rc = check_intrinsics(h, o, K, B))) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, (size_t)B * 3 * hw), *d_src = st.in("srcs", srcs, (size_t)S * B * 3 * hw), *d_dt = st.in("depth_t", depth_t, (size_t)B * hw);
    const float *d_ds = st.in("depth_s", depth_s, (size_t)S * B * hw), *d_K = st.in("K", K, (size_t)B * 9), *d_pose = st.in("pose", pose, (size_t)N * 6);
    const float *d_d0 = st.in("depth0", depth0, (size_t)B * hw);
    float *d_g = st.out("g_rho_out", g_rho_out, (size_t)B * hw), *d_gs = st.out("g_rho_src_out", g_rho_src_out, (size_t)S * B * hw);
    st.host_out("scal_out", scal_out, 8 * sizeof(double)); st.host_out("g_pose_out", g_pose_out, (size_t)N * 6 * sizeof(double));
    if (st.ready(entry)) return st.rc;
    tcsfm_opts oo = *o;
    oo.n_iters = 1; oo.solver = TCSFM_SOLVER_GN;
    DrefExport ex{scal_out, g_pose_out, d_g, d_d0, d_gs};
    if ((rc = dense_ref_run(DenseCall{h, &oo, B, S, d_tgt, d_src, d_dt, d_ds, d_K, d_pose, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, &ex}))) return rc;
    return st.finish();
}

int tcsfm_linearize_dense_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                 const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *depth0,
                                 double *scal_out, double *g_pose_out, float *g_rho_out) {
    return linearize_dense_window_impl(h, o, B, S, tgt, srcs, depth_t, depth_s, K, pose, depth0, scal_out, g_pose_out, g_rho_out, nullptr, "tcsfm_linearize_dense_window");
}
int tcsfm_linearize_dense_window_sources(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                         const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *depth0,
                                         double *scal_out, double *g_pose_out, float *g_rho_out, float *g_rho_src_out) {
    if (!g_rho_src_out) return h ? fail(h, TCSFM_E_ARG, "tcsfm_linearize_dense_window_sources: NULL argument") : TCSFM_E_ARG;
    return linearize_dense_window_impl(h, o, B, S, tgt, srcs, depth_t, depth_s, K, pose, depth0, scal_out, g_pose_out, g_rho_out, g_rho_src_out, "tcsfm_linearize_dense_window_sources");
}

int tcsfm_debug_check_guards(int *n_allocations, int *n_damaged) {
    if (n_allocations) *n_allocations = -1;
    if (n_damaged) *n_damaged = 0;
    if (!tcguard::on()) return TCSFM_OK;
    if (hipDeviceSynchronize() != hipSuccess) return TCSFM_E_HIP;
    std::lock_guard<std::mutex> lk(tcguard::mtx());
    int bad_allocs = 0;
    for (auto &r : tcguard::recs()) {
        long off = 0;
        const long bad = tcguard::damaged(r, &off);
        if (bad < 0) return TCSFM_E_HIP;
        if (bad > 0) {
            bad_allocs++;
            if (!r.reported)
                fprintf(stderr, "tcsfm guard: allocation of %zu bytes (%s:%d): %ld band bytes overwritten, first at offset %ld of the allocation\n", r.bytes, tcguard::at_file(r), r.line, bad, off);
            r.reported = true;
        }
    }
    if (n_allocations) *n_allocations = (int)tcguard::recs().size();
    if (n_damaged) *n_damaged = bad_allocs;
    return TCSFM_OK;
}

int tcsfm_debug_guard_selftest(int *detected) {
    if (detected) *detected = -1;
    if (!tcguard::on()) return TCSFM_OK;
    DevBuf<char> p, q;
    if (DEV_RESERVE(p, 1000) != hipSuccess) return TCSFM_E_HIP;
    if (hipMemset(p + 1000, 0, 4) != hipSuccess) return TCSFM_E_HIP;      // four bytes past the end
    int found = 0;
    {
        std::lock_guard<std::mutex> lk(tcguard::mtx());
        for (auto &r : tcguard::recs())
            if (r.base + tcguard::kBand == p.p) { long off = 0; found = tcguard::damaged(r, &off) == 4 && off == 1000; r.reported = true; }
    }
    // the check an entry runs over its OWN allocations before it frees them (tcsfm_debug_solve) sees the same damage, and only there
    if (DEV_RESERVE(q, 1000) != hipSuccess) return TCSFM_E_HIP;
    found = found && tcguard::damaged_among({(void *)p.p, (void *)q.p}) == 1 && tcguard::damaged_among({(void *)q.p}) == 0;
    if (detected) *detected = found;
    return TCSFM_OK;
}

// The flip post-processing's ramp table (flip_ramp.h) for the handle's W on the device: built on the host on first use,
// kept for the handle's life.  NULL: h->err says why.
static const double *flip_ramp_device(tcsfm_handle h) {
    if (h->flip_ramp) return h->flip_ramp;
    std::vector<double> ramp((size_t)h->W);
    flip_ramp(h->W, ramp.data());
    DevBuf<double> dev;
    if (hipError_t e = DEV_RESERVE(dev, ramp.size())) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return nullptr; }
    if (hipError_t e = hipMemcpy(dev, ramp.data(), ramp.size() * sizeof(double), hipMemcpyHostToDevice)) {      // (synchronous: ramp is a temporary)
        h->err = std::string("hipMemcpy: ") + hipGetErrorString(e);
        return nullptr;
    }
    return h->flip_ramp = std::move(dev);
}

// k_disp_post over n planes: the vector form where the row pairs are aligned (W even, 8-byte l / rf, 16-byte out), else the scalar one
static hipError_t launch_disp_post(hipStream_t s, int n, int H, int W, const float *l, const float *rf, const double *ramp, double *out) {
    const long long rows = (long long)n * H, threads = rows * ((W + 1) / 2);
    const dim3 grid((unsigned)((threads + 255) / 256));
    const bool vec = W % 2 == 0 && (((uintptr_t)l | (uintptr_t)rf) & 7) == 0 && ((uintptr_t)out & 15) == 0;
    if (vec) hipLaunchKernelGGL(k_disp_post<true>, grid, dim3(256), 0, s, l, rf, ramp, out, rows, W);
    else hipLaunchKernelGGL(k_disp_post<false>, grid, dim3(256), 0, s, l, rf, ramp, out, rows, W);
    return hipGetLastError();
}

#include "posenet_host.h"
#include "depthnet_host.h"

// The device copy of the resize tables for (src_h, src_w) -> the handle's (H, W): built on the host once per source size and kept for the
// handle's life (a handful of ints per output row and column).  NULL: h->err says why (the caller returns TCSFM_E_HIP / TCSFM_E_ARG).
static const ResizeTable *resize_table(tcsfm_handle h, int src_h, int src_w) {
    for (const auto &t : h->resize_tabs)
        if (t.sh == src_h && t.sw == src_w) return &t;
    tcsfm_ctx::OwnedResizeTable T;
    T.sh = src_h; T.sw = src_w; T.H = h->H; T.W = h->W;
    std::vector<int> blob;
    if (!resize_build_table(T, blob)) { h->err = "resize: the source size is beyond the kernel's tile (resize_u8_kernel.h)"; return nullptr; }
    if (hipError_t e = DEV_RESERVE(T.blob, blob.size())) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return nullptr; }
    if (hipError_t e = hipMemcpy(T.blob, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice)) {      // (synchronous: blob is a temporary)
        h->err = std::string("hipMemcpy: ") + hipGetErrorString(e);
        return nullptr;
    }
    T.dev = T.blob;
    h->resize_tabs.push_back(std::move(T));
    return &h->resize_tabs.back();
}

#include "sequence_host.h"

int tcsfm_disp_post_process(tcsfm_handle h, const tcsfm_opts *o, int N, const void *l_disp, const void *r_disp_mirrored, void *out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !l_disp || !r_disp_mirrored || !out) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: NULL argument");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: host_ptrs must be 0 (device pointers); a host caller has the sequence calls (tcsfm_sequence_disparity)");
    if (h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: the ramp needs W >= 2");
    if ((((uintptr_t)l_disp | (uintptr_t)r_disp_mirrored) & 3) != 0 || ((uintptr_t)out & 7) != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: the inputs must be aligned for float, out for double");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("l_disp", l_disp, (size_t)N * hw * sizeof(float)); a.in("r_disp_mirrored", r_disp_mirrored, (size_t)N * hw * sizeof(float));
    a.out("out", out, (size_t)N * hw * sizeof(double));
    if (int rc = check_overlap(h, "tcsfm_disp_post_process", a)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    const double *ramp = flip_ramp_device(h);
    if (!ramp) return TCSFM_E_HIP;
    HIPCHK(h, launch_disp_post(h->stream, N, h->H, h->W, (const float *)l_disp, (const float *)r_disp_mirrored, ramp, (double *)out));
    return TCSFM_OK;
}

int tcsfm_flip_ramp(int W, void *l_mask_out) {
    if (W < 2 || !l_mask_out) return TCSFM_E_ARG;
    tc::flip_ramp(W, (double *)l_mask_out);
    return TCSFM_OK;
}

int tcsfm_frames_from_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, const void *src, void *dst) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !src || !dst) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: NULL argument");
    if (format != TCSFM_FRAMES_U8_CHW && format != TCSFM_FRAMES_U8_HWC)
        return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: format must be TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC (float frames need no conversion)");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: host_ptrs must be 0 (device pointers); host frames go through the sequence calls (tcsfm_sequence_frame_format)");
    if (((uintptr_t)dst & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: dst must be aligned for float");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("src", src, (size_t)N * 3 * hw); a.out("dst", dst, (size_t)N * 3 * hw * sizeof(float));
    std::string msg;
    if (a.refused("tcsfm_frames_from_u8", msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    HIPCHK(h, launch_frames_u8(h->stream, format == TCSFM_FRAMES_U8_HWC, N, (const uint8_t *)src, (float *)dst, nullptr, 0, hw));
    return TCSFM_OK;
}

int tcsfm_resize_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, int src_h, int src_w, const void *src, int dst_format, void *dst) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !src || !dst) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: NULL argument");
    if (format != TCSFM_FRAMES_U8_CHW && format != TCSFM_FRAMES_U8_HWC)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: format must be TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC");
    if (dst_format != format && dst_format != TCSFM_FRAMES_F32_CHW)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: dst_format must be the source's format (bytes) or TCSFM_FRAMES_F32_CHW");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: host_ptrs must be 0 (device pointers); host frames go through the sequence calls (tcsfm_sequence_frame_source)");
    if (src_h <= 0 || src_w <= 0) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: src_h and src_w must be positive");
    if (const char *why = resize_refusal(src_h, src_w, h->H, h->W)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_resize_u8: ") + why).c_str());
    const bool f32 = dst_format == TCSFM_FRAMES_F32_CHW;
    if (f32 && ((uintptr_t)dst & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: a float dst must be aligned for float");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("src", src, (size_t)N * 3 * src_h * src_w); a.out("dst", dst, (size_t)N * 3 * hw * (f32 ? sizeof(float) : 1));
    std::string msg;
    if (a.refused("tcsfm_resize_u8", msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    const ResizeTable *T = resize_table(h, src_h, src_w);
    if (!T) return TCSFM_E_HIP;
    HIPCHK(h, launch_resize_u8(h->stream, *T, format == TCSFM_FRAMES_U8_HWC, f32, N, (const uint8_t *)src, dst, nullptr, 0));
    return TCSFM_OK;
}

int tcsfm_resize_coeffs(int in, int out, int *ksize_out, int *bounds, int *kk) {
    if (in < 1 || out < 1 || !ksize_out) return TCSFM_E_ARG;
    *ksize_out = tc::resize_coeffs(in, out, bounds, kk);
    return TCSFM_OK;
}

int tcsfm_scale_intrinsics(int src_h, int src_w, int H, int W, const void *K_src, void *K_out) {
    if (src_h < 1 || src_w < 1 || H < 1 || W < 1 || !K_src || !K_out) return TCSFM_E_ARG;
    tc::scale_intrinsics(src_h, src_w, H, W, (const float *)K_src, (float *)K_out);
    return TCSFM_OK;
}

int tcsfm_lane_wait(tcsfm_handle h, int lane) {
    tcsfm_ctx *c = lane_of(h, lane);
    if (!c) return h ? fail(h, TCSFM_E_ARG, "tcsfm_lane_wait: no such lane") : TCSFM_E_ARG;
    if (c == h) return TCSFM_OK;
    DeviceGuard dev_guard(h->device);
    HIPCHK(h, hipStreamWaitEvent(h->stream, c->done_ev, 0));     // consumers on the parent's stream see the lane's outputs
    return TCSFM_OK;
}

int tcsfm_lane_event(tcsfm_handle h, int lane, void **event_out) {
    tcsfm_ctx *c = lane_of(h, lane);
    if (!c || !event_out) return h ? fail(h, TCSFM_E_ARG, "tcsfm_lane_event: bad argument") : TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    constexpr size_t kMarks = 64;
    if (c->marks.size() < kMarks) {
        HIPCHK(h, c->marks.grow(c->marks.size() + 1));
        c->mark_next = c->marks.size() - 1;
    }
    hipEvent_t e = c->marks[c->mark_next];
    c->mark_next = (c->mark_next + 1) % kMarks;
    HIPCHK(h, hipEventRecord(e, (c == h || h->lanes_serial) ? h->stream : c->own_stream));      // (serial lanes: the lane's calls ran on the handle's stream)
    *event_out = (void *)e;
    return TCSFM_OK;
}

int tcsfm_stream_wait_event(tcsfm_handle h, void *hip_stream, void *event) {
    if (!h || !event) return TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    HIPCHK(h, hipStreamWaitEvent((hipStream_t)hip_stream, (hipEvent_t)event, 0));
    return TCSFM_OK;
}

int tcsfm_lane_synchronize(tcsfm_handle h, int lane) {
    tcsfm_ctx *c = lane_of(h, lane);
    if (!c) return h ? fail(h, TCSFM_E_ARG, "tcsfm_lane_synchronize: no such lane") : TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    HIPCHK(h, hipStreamSynchronize((c == h || h->lanes_serial) ? h->stream : c->own_stream));
    if (int rc = pending_error(c)) { h->err = c->err; return rc; }
    if (h->lanes_serial) return pending_error(h);
    return TCSFM_OK;
}

int tcsfm_debug_trace(tcsfm_handle h, uint16_t *bits, int64_t bits_capacity, int32_t *decide, int64_t decide_capacity) {
    if (!h) return TCSFM_E_ARG;
    if ((bits && bits_capacity < 1) || (decide && decide_capacity < 1)) return fail(h, TCSFM_E_ARG, "tcsfm_debug_trace: bad capacity");
    h->trace_bits = bits; h->trace_bits_cap = bits ? bits_capacity : 0;
    h->trace_decide = decide; h->trace_decide_cap = decide ? decide_capacity : 0;
    return TCSFM_OK;
}

// diagnostic: copy the k_solve phase stamps to the host (8 values; zeros unless TCSFM_DEBUG_STAMPS was set at create)
int tcsfm_debug_stamps(tcsfm_handle h, long long out[8]) {
    if (!h || !out) return TCSFM_E_ARG;
    memset(out, 0, 8 * sizeof(long long));
    if (!h->dbg_stamps) return TCSFM_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->dbg_stamps, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return TCSFM_OK;
}

int tcsfm_debug_solve_layout(int *sizeof_pair_state, int *sizeof_pair_const) {
    if (sizeof_pair_state) *sizeof_pair_state = (int)sizeof(PairState);
    if (sizeof_pair_const) *sizeof_pair_const = (int)sizeof(PairConst);
    return TCSFM_OK;
}

#include "debug_solve_host.h"      // DebugBufs, the joint entry

int tcsfm_debug_solve_joint_layout(int *sizeof_pair_state, int *sizeof_pair_const, int *sizeof_joint_state) {
    if (sizeof_joint_state) *sizeof_joint_state = (int)sizeof(JointState);
    return tcsfm_debug_solve_layout(sizeof_pair_state, sizeof_pair_const);
}
int tcsfm_debug_solve_joint(tcsfm_handle h, const tcsfm_opts *o, tcsfm_debug_solve_joint_args *a) { return debug_solve_joint_run(h, o, a); }

int tcsfm_debug_solve(tcsfm_handle h, const tcsfm_opts *o, tcsfm_debug_solve_args *a) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
#define DS_REFUSE(cond, msg) if (cond) return fail(h, TCSFM_E_ARG, "tcsfm_debug_solve: " msg)
    DS_REFUSE(!o || !a, "NULL argument");
    DS_REFUSE(!a->records || !a->state || !a->pconst, "records, state and pconst are required");
    DS_REFUSE(a->variant < 0 || a->variant > 3, "variant must be 0 .. 3");
    DS_REFUSE(a->mode < 0 || a->mode > 2, "mode must be 0, 1 or 2");
    DS_REFUSE(a->N < 1 || a->N > 4096 || a->ngrp < 1 || a->ngrp > 65536, "N and ngrp must be at least 1");
    DS_REFUSE(a->n_alloc < a->N || a->n_alloc > 8192, "n_alloc must be at least N");
    DS_REFUSE(o->n_iters < 0 || o->n_iters > 1024 || a->it < 0 || a->it > o->n_iters, "need 0 <= it <= n_iters");
    DS_REFUSE(o->solver != TCSFM_SOLVER_GN && o->solver != TCSFM_SOLVER_LM, "unknown solver");
    DS_REFUSE(o->param != TCSFM_PARAM_SE3 && o->param != TCSFM_PARAM_EULER, "unknown param");
    DS_REFUSE(o->refine != TCSFM_REFINE_POSE && o->refine != TCSFM_REFINE_POSE_SCALE, "unknown refine");
    const int np = np_of(o), N = a->N, nacc = nacc_of(np);
    const bool pc_asked = a->w_pc > 0.0 || a->w_pc != a->w_pc;
    DS_REFUSE(a->variant >= 1 && o->param != TCSFM_PARAM_SE3, "variants 1 to 3 have the SE(3) chart only");
    DS_REFUSE((a->variant == 1 || a->variant == 2) && pc_asked, "variants 1 and 2 have no pose-consistency term");
    DS_REFUSE(a->variant >= 2 && np == 7, "k_solve_front solves 6-DoF pairs only");
    DS_REFUSE(pc_asked && np == 7, "the pose-consistency term is 6-DoF only");
    DS_REFUSE(a->mode == 2 && !a->lin_out, "mode 2 needs lin_out");
    DS_REFUSE(a->grp_fwd < 0 || a->n_pairs < 0 || a->grp_fwd > a->n_pairs, "need 0 <= grp_fwd <= n_pairs");
    DS_REFUSE(a->pc_np < 0 || a->pc_self0 < 0 || a->pc_part0 < 0 || a->pose_lin_pairs < 0, "negative pose_lin geometry");
    DS_REFUSE(a->rule && a->n_pairs != N, "the window rule needs n_pairs == N");
    if (a->rule && a->norms) {
        DS_REFUSE(a->norm_B < 0 || a->norm_n < 1 || (a->norm_B > 0 && a->norm_Bt < 1), "bad norms geometry");
        for (int n = 0; n < N; n++)
            DS_REFUSE((a->norm_B > 0 ? (n % a->norm_Bt) / a->norm_B : 0) >= a->norm_n, "norms is shorter than a pair's group index needs");
    }
    if (a->pose_lin) {
        const int per = a->pc_np > 0 ? a->pc_np : a->n_pairs;
        DS_REFUSE(a->pc_np == 0 && a->n_pairs != N, "the unsliced pose-consistency form needs n_pairs == N");
        DS_REFUSE(per < 1 || per != a->pose_lin_pairs, "pose_lin_pairs must be the pairs per pose_lin buffer (pc_np, or n_pairs)");
        for (int n = 0; n < N; n++) {
            const long long self = a->pc_np > 0 ? (long long)a->pc_self0 + n : n;
            DS_REFUSE(self >= per, "a pair's own slot is outside pose_lin");
            if (a->rule && pc_asked) {
                const long long partner = a->pc_np > 0 ? (long long)a->pc_part0 + n : (n < a->grp_fwd ? (long long)n + a->grp_fwd : (long long)n - a->grp_fwd);
                DS_REFUSE(partner < 0 || partner >= per, "a partner index is outside pose_lin");
            }
        }
    }
    DS_REFUSE(a->c_ncall < 0 || a->c_ncall > TC_MAX_COAL, "c_ncall out of range");
    if (a->c_ncall > 0) {
        DS_REFUSE(a->c_B < 1 || a->c_S < 1 || a->c_n0 < 0 || a->c_B > 4096 || a->c_S > 4096 || a->c_n0 > (1 << 20), "bad coalesce geometry");
        for (int n = 0; n < N; n++) {
            const CoalIdx ci = coal_index(a->c_ncall, a->c_B, a->c_S, n + a->c_n0);
            DS_REFUSE(ci.call < 0 || ci.call >= a->c_ncall || !a->c_pose_out[ci.call] || ci.li < 0 || ci.li >= a->c_len[ci.call],
                      "a coalesced pair's output slot is outside the given per-call arrays");
        }
    }
#undef DS_REFUSE
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    SolveParams S = solve_params(h, o, np, 0);
    DebugBufs B;
    const size_t na = (size_t)a->n_alloc;
    void *p = nullptr;
#define DS_UP(dst, type, host, bytes, out) HIPCHK(h, B.up((host), (bytes), (out), &p)); dst = (type)p
    DS_UP(S.partials, const float *, a->records, na * a->ngrp * nacc * sizeof(float), false);
    DS_UP(S.st, PairState *, a->state, na * sizeof(PairState), true);
    DS_UP(S.pc, PairConst *, a->pconst, na * sizeof(PairConst), true);
    DS_UP(S.stats, float *, a->stats, na * (o->n_iters + 1) * TCSFM_NSTAT * sizeof(float), true);
    DS_UP(S.lin_out, double *, a->lin_out, na * (np * np + np + 4) * sizeof(double), true);
    DS_UP(S.delta_out, double *, a->delta_out, na * 8 * sizeof(double), true);
    DS_UP(S.accept_out, int *, a->accept_out, na * sizeof(int), true);
    DS_UP(S.trace_decide, int *, a->trace_decide, na * sizeof(int), true);
    DS_UP(S.pose_out, float *, a->pose_out, na * 6 * sizeof(float), true);
    DS_UP(S.log_scale_out, float *, a->log_scale_out, na * sizeof(float), true);
    DS_UP(S.pose_lin, double *, a->pose_lin, (size_t)2 * a->pose_lin_pairs * 12 * sizeof(double), true);
    DS_UP(S.norms, const int *, a->rule ? a->norms : nullptr, (size_t)a->norm_n * 2 * sizeof(int), false);
    for (int i = 0; i < a->c_ncall; i++) {
        DS_UP(S.c_pose_out[i], float *, a->c_pose_out[i], (size_t)a->c_len[i] * 6 * sizeof(float), true);
        DS_UP(S.c_ls_out[i], float *, a->c_ls_out[i], (size_t)a->c_len[i] * sizeof(float), true);
    }
#undef DS_UP
    S.ngrp = a->ngrp; S.it = a->it; S.mode = a->mode; S.dbg = nullptr;
    S.rule = a->rule ? 1 : 0; S.grp_fwd = a->grp_fwd; S.n_pairs = a->n_pairs; S.scale_fwd = a->scale_fwd; S.scale_inv = a->scale_inv;
    S.norm_Bt = a->norm_Bt; S.norm_B = a->norm_B;
    S.w_pc = a->w_pc; S.pc_eps = a->pc_eps; S.pc_np = a->pc_np; S.pc_self0 = a->pc_self0; S.pc_part0 = a->pc_part0;
    S.c_ncall = a->c_ncall; S.c_B = a->c_B; S.c_S = a->c_S; S.c_n0 = a->c_n0;
    if (a->variant <= 1) launch_solve_as(h, S, N, np, a->variant == 1);
    else {
        JointSolveParams Pj;
        memset(&Pj, 0, sizeof(Pj));       // B = 0: every workgroup takes the pair role
        if (a->variant == 3) hipLaunchKernelGGL((k_solve_front<1, true>), dim3(N), dim3(JSOLVE_NT), 0, h->stream, Pj, S);
        else hipLaunchKernelGGL((k_solve_front<1>), dim3(N), dim3(JSOLVE_NT), 0, h->stream, Pj, S);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (const auto &b : B.back) HIPCHK(h, hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    // the entry's allocations are freed when it returns, so tcsfm_debug_check_guards never sees them: their bands are checked here
    const int hit = tcguard::damaged_among(B.dev);
    if (hit < 0) return fail(h, TCSFM_E_HIP, "tcsfm_debug_solve: could not read the guard bands back");
    if (hit > 0) return fail(h, TCSFM_E_HIP, "tcsfm_debug_solve: the launch wrote outside the entry's device arrays (guard bands damaged, details on stderr)");
    return TCSFM_OK;
}

int tcsfm_profile_begin(tcsfm_handle h) {
    if (!h) return TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    h->stamp_cap = (size_t)4 << 20;         // 4 M workgroup stamps = 64 MB: ~8000 launches of the BASELINE config
    RESERVE(h, h->stamp_buf, h->stamp_cap * 2);
    h->stamp_used = 0;
    h->stamp_launch.clear();
    for (tcsfm_ctx *c : h->lanes)                       // the lanes are bracketed too: their figures are added in profile_end
        if (int rc = tcsfm_profile_begin(c)) { h->err = c->err; return rc; }
    h->profiling = true;
    h->ev_used = 0;
    h->ev_class.clear();
    return TCSFM_OK;
}

int tcsfm_profile_end(tcsfm_handle h, double ms_sum[3], int64_t launches[3]) {
    if (!h || !ms_sum || !launches) return TCSFM_E_ARG;
    h->profiling = false;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) { ms_sum[i] = 0.0; launches[i] = 0; }
    for (size_t k = 0; k < h->ev_class.size(); k++) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev_pool[2 * k], h->ev_pool[2 * k + 1]));
        ms_sum[h->ev_class[k]] += ms;
        launches[h->ev_class[k]]++;
    }
    h->ev_used = 0;
    h->ev_class.clear();
    for (tcsfm_ctx *c : h->lanes) {
        double ms[3]; int64_t n[3];
        if (int rc = tcsfm_profile_end(c, ms, n)) { h->err = c->err; return rc; }
        for (int i = 0; i < 3; i++) { ms_sum[i] += ms[i]; launches[i] += n[i]; }
    }
    return TCSFM_OK;
}

int tcsfm_profile_kernel_time(tcsfm_handle h, double *ms_sum, int64_t *launches) {
    if (!h || !ms_sum || !launches) return TCSFM_E_ARG;
    *ms_sum = 0.0; *launches = 0;
    DeviceGuard dev_guard(h->device);
    if (h->stamp_buf && h->stamp_used > 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<unsigned long long> st(h->stamp_used * 2);
        HIPCHK(h, hipMemcpy(st.data(), h->stamp_buf, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (const auto &l : h->stamp_launch) {     // duration of a launch = latest workgroup end - earliest workgroup start
            unsigned long long t0 = ~0ull, t1 = 0ull;
            for (size_t w = l.first; w < l.first + l.second; w++) { t0 = st[2 * w] < t0 ? st[2 * w] : t0; t1 = st[2 * w + 1] > t1 ? st[2 * w + 1] : t1; }
            if (t1 > t0) { *ms_sum += (double)(t1 - t0) * 1e-5; (*launches)++; }   // 100 MHz ticks -> ms
        }
    }
    for (tcsfm_ctx *c : h->lanes) {
        double ms = 0.0; int64_t n = 0;
        if (int rc = tcsfm_profile_kernel_time(c, &ms, &n)) { h->err = c->err; return rc; }
        *ms_sum += ms; *launches += n;
    }
    return TCSFM_OK;
}

// [start, end] of every stamped launch of the handle and of its lanes, in 100 MHz ticks of the device's s_memrealtime counter
static int profile_intervals(tcsfm_ctx *h, std::vector<std::pair<unsigned long long, unsigned long long>> &out) {
    DeviceGuard dev_guard(h->device);
    if (h->stamp_buf && h->stamp_used > 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<unsigned long long> st(h->stamp_used * 2);
        HIPCHK(h, hipMemcpy(st.data(), h->stamp_buf, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (const auto &l : h->stamp_launch) {
            unsigned long long t0 = ~0ull, t1 = 0ull;
            for (size_t w = l.first; w < l.first + l.second; w++) { t0 = st[2 * w] < t0 ? st[2 * w] : t0; t1 = st[2 * w + 1] > t1 ? st[2 * w + 1] : t1; }
            if (t1 > t0) out.push_back({t0, t1});
        }
    }
    for (tcsfm_ctx *c : h->lanes)
        if (int rc = profile_intervals(c, out)) { h->err = c->err; return rc; }
    return TCSFM_OK;
}

int tcsfm_profile_kernel_busy(tcsfm_handle h, double *ms_busy, int64_t *launches) {
    if (!h || !ms_busy || !launches) return TCSFM_E_ARG;
    *ms_busy = 0.0; *launches = 0;
    std::vector<std::pair<unsigned long long, unsigned long long>> iv;
    if (int rc = profile_intervals(h, iv)) return rc;
    std::sort(iv.begin(), iv.end());
    unsigned long long busy = 0, lo = 0, hi = 0;
    bool open = false;
    for (const auto &x : iv) {
        if (open && x.first <= hi) { hi = std::max(hi, x.second); continue; }
        if (open) busy += hi - lo;
        lo = x.first; hi = x.second; open = true;
    }
    if (open) busy += hi - lo;
    *ms_busy = (double)busy * 1e-5;
    *launches = (int64_t)iv.size();
    return TCSFM_OK;
}

#include "posenet_wgrad_host.h"
#include "posenet_grad_host.h"
#include "optim_host.h"
#include "depth_eval_host.h"

void tcsfm_pose_to_matrix(const double pose[6], double T[12]) { tc::pose_to_T(pose, T); }
void tcsfm_matrix_to_pose(const double T[12], double pose[6]) { tc::T_to_pose(T, pose); }
void tcsfm_se3_exp(const double xi[6], double T[12]) { tc::se3_exp(xi, T); }
void tcsfm_se3_log(const double T[12], double xi[6]) { tc::se3_log(T, xi); }
void tcsfm_se3_mul(const double A[12], const double B[12], double C[12]) { tc::se3_mul(A, B, C); }
void tcsfm_se3_inv(const double A[12], double B[12]) { tc::se3_inv(A, B); }
