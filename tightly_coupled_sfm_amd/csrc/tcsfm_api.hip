// tcsfm_api.hip -- C ABI (include/tcsfm.h) over the gfx950 kernels in kernels.h.
// Host logic only: the include order, create / destroy / stream / synchronize, the four refine forwards with dense_body, the lane event
// entries and the SE(3) forwards.  The handle, staging and the argument checks are context.h's, over the owners and guard bands of
// device_owned.h.  Every other entry lives in a driver, a header of this translation unit included where its helpers are first needed:
// pose_host.h (the pose modes), dense_host.h (the dense modes), call_host.h (graph replay, queued calls, lanes), operators_host.h (the
// drop-in operators and the evaluation entries), frames_host.h (frame preparation), sequence_host.h, the networks' hosts, profile_host.h
// and debug_solve_host.h.  DESIGN.md, "Where the host code lives", is the map.
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
#include "operator_plan.h"

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

#include "operators_host.h"      // the drop-in operators, forward and backward, and the evaluation entries

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

#include "frames_host.h"      // frame preparation: flip post-processing, 8-bit frames, resize tables
#include "posenet_host.h"
#include "depthnet_host.h"
#include "sequence_host.h"

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

#include "profile_host.h"      // guard-band readers, decision trace, stamps, tcsfm_profile_*
#include "debug_solve_host.h"      // DebugBufs, tcsfm_debug_solve and its joint sibling
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
