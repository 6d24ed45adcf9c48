// Host side of the drop-in operators, forward and backward, and of the evaluation entries (include/tcsfm.h: tcsfm_disp_to_depth, tcsfm_ssim,
// tcsfm_warp*, tcsfm_photometric*, tcsfm_smooth_loss*, tcsfm_window_loss*, tcsfm_scale_recovery*, tcsfm_linearize, tcsfm_linearize_window,
// tcsfm_loss_surface).  Every entry is four steps: enter (op_enter, then the entry's own option refusals), stage (Staging; stage_pairs for
// the pair inputs), launch, finish.  Which launches a backward makes when cotangents or outputs are NULL, and every grid and scratch size,
// are operator_plan.h's (no HIP there): nothing is decided here.  Part of tcsfm_api.hip, the library's only translation unit: included
// after call_host.h (drain_queued) and pose_host.h, whose run_init, run_pack, lin_params, launch_lin and pose_evaluate the entries use.
//
// The order of the refusals where several faults coincide: handle; options and sizes; NULL arguments; the entry's own option refusals
// (depth_is_disp, image too small); a pending device error; intrinsics; overlap.
#pragma once
#include "operator_plan.h"

namespace {

// Enter: queued calls run first; then the handle, the options and the sizes (check_common over N pairs; N < 0: an entry that takes an
// element or plane count has only the options to check and folds its count into args_ok), then the NULL test with the entry's message.
int op_enter(tcsfm_ctx *h, const tcsfm_opts *o, int N, bool args_ok, const char *msg) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (N >= 0) {
        if (int rc = check_common(h, o, N)) return rc;
    } else if (!h) return TCSFM_E_ARG;
    return (o && args_ok) ? TCSFM_OK : fail(h, TCSFM_E_ARG, msg);
}

// The pair inputs of an entry, as the caller gave them and as staged on the device.
struct PairArgs { const float *tgt, *src, *depth_t, *depth_s, *pose, *K; };
// Registered in the entries' argument order under their argument names -- the pair form: (tgt,) src, depth_t, depth_s, <pose_name>, K; the
// window form: tgt, srcs, depth_t, depth_s, K, pose -- for nt target image sets (and intrinsics), ns source sets and np poses.
PairArgs stage_pairs(Staging &st, const PairArgs &a, bool has_tgt, bool window, const char *pose_name, size_t nt, size_t ns, size_t np) {
    const size_t hw = (size_t)st.h->H * st.h->W;
    PairArgs d{};
    if (has_tgt) d.tgt = st.in("tgt", a.tgt, nt * 3 * hw);
    d.src = st.in(window ? "srcs" : "src", a.src, ns * 3 * hw);
    d.depth_t = st.in("depth_t", a.depth_t, nt * hw); d.depth_s = st.in("depth_s", a.depth_s, ns * hw);
    if (window) d.K = st.in("K", a.K, nt * 9);
    d.pose = st.in(pose_name, a.pose, np * 6);
    if (!window) d.K = st.in("K", a.K, nt * 9);
    return d;
}
PairArgs stage_pairs(Staging &st, const PairArgs &a, bool has_tgt, int N) { return stage_pairs(st, a, has_tgt, false, "pose", N, N, N); }

// the start of the staging of an entry that reads intrinsics: the pending device error, then the pinhole check of n matrices
int stage_K(Staging &st, const float *K, int n) { return st.rc ? st.rc : check_intrinsics(st.h, st.o, K, n); }

dim3 pixel_grid(const tcsfm_ctx *h, int planes) { return dim3(pixel_blocks((size_t)h->H * h->W), planes); }
dim3 tile_grid_of(const tcsfm_ctx *h, int planes) {
    const TileGrid t = tile_grid(h->W, h->H, PG_TW, PG_TH);
    return dim3(t.x, t.y, (unsigned)planes);
}

// k_warp over N pairs behind their pair constants: the warp's maps, or (tgt, posenet_in) the PoseNet's input
int launch_warp(tcsfm_ctx *h, const tcsfm_opts *o, int N, const PairArgs &d, float *rec, float *valid, float *pd, float *cd, float *posenet_in) {
    if (int rc = run_init(h, o, N, d.pose, nullptr, d.K, 0)) return rc;
    WarpParams P;
    P.src = d.src; P.depth_t = d.depth_t; P.depth_s = d.depth_s; P.pc = h->pconst;
    P.rec = rec; P.valid = valid; P.pd = pd; P.cd = cd; P.tgt = d.tgt; P.posenet_in = posenet_in; P.H = h->H; P.W = h->W;
    P.win_B = 0; P.win_S = 0;
    hipLaunchKernelGGL(k_warp, pixel_grid(h, N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

// The launches of the warp's backward on device pointers (shared by tcsfm_warp_backward and tcsfm_photometric_backward): cotangents may
// be null (= zero), outputs may be null (= not wanted); what runs is the plan's.  `inited`: run_init has already formed this call's pair
// constants.
int warp_backward_dev(tcsfm_ctx *h, const tcsfm_opts *o, int N, const PairArgs &d, const float *d_grec, const float *d_gpd, const float *d_gcd,
                      float *o_dt, float *o_ds, float *o_pose, bool inited) {
    const size_t hw = (size_t)h->H * h->W;
    const WarpBwdPlan pl = warp_bwd_plan(d_gpd != nullptr, o_dt != nullptr, o_ds != nullptr, o_pose != nullptr, hw);
    const dim3 grid = pixel_grid(h, N);
    if (pl.reserve_rec) RESERVE(h, h->wgrad_rec, (size_t)h->max_pairs * grid.x * 12);
    if (pl.reserve_scatter) {
        RESERVE(h, h->wgrad_fix, (size_t)h->max_pairs * hw);
        RESERVE(h, h->wgrad_gmax, (size_t)h->max_pairs);
    }
    if (pl.zero_ds) HIPCHK(h, hipMemsetAsync(o_ds, 0, N * hw * sizeof(float), h->stream));      // nothing flows into the source depth
    if (pl.pair_consts && !inited)
        if (int rc = run_init(h, o, N, d.pose, nullptr, d.K, 0)) return rc;
    if (pl.scatter) {
        HIPCHK(h, hipMemsetAsync(h->wgrad_fix, 0, N * hw * sizeof(long long), h->stream));
        HIPCHK(h, hipMemsetAsync(h->wgrad_gmax, 0, (size_t)N * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(k_warp_gmax, grid, dim3(256), 0, h->stream, d_gpd, h->wgrad_gmax, (int)hw);
        WarpScatterParams S;
        S.depth_t = d.depth_t; S.pc = h->pconst; S.g_pd = d_gpd; S.gmax = h->wgrad_gmax; S.fix = h->wgrad_fix; S.H = h->H; S.W = h->W; S.lg_hw = pl.lg_hw;
        hipLaunchKernelGGL(k_warp_scatter, grid, dim3(256), 0, h->stream, S);
        hipLaunchKernelGGL(k_warp_fix_out, grid, dim3(256), 0, h->stream, (const long long *)h->wgrad_fix, (const unsigned *)h->wgrad_gmax, o_ds, (int)hw, pl.lg_hw);
        HIPCHK(h, hipGetLastError());
    }
    if (pl.bwd) {
        WarpGradParams P;
        P.src = d.src; P.depth_t = d.depth_t; P.depth_s = d.depth_s; P.pc = h->pconst; P.st = h->state; P.g_rec = d_grec; P.g_pd = d_gpd; P.g_cd = d_gcd;
        P.d_depth_t = o_dt; P.blockrec = pl.tail ? h->wgrad_rec : nullptr; P.H = h->H; P.W = h->W;
        hipLaunchKernelGGL(k_warp_bwd, grid, dim3(256), 0, h->stream, P);
        if (pl.tail) hipLaunchKernelGGL(k_warp_pose_tail, dim3(N), dim3(64), 0, h->stream, (const double *)h->wgrad_rec, (int)grid.x, d.pose, d.K, o_pose);
        HIPCHK(h, hipGetLastError());
    }
    return TCSFM_OK;
}

// k_photo_bwd on device pointers.  A requested output whose cotangent is absent is zeroed without a launch (the plan says which).
int photo_maps_backward_dev(tcsfm_ctx *h, const tcsfm_opts *o, int N, const float *d_tgt, const float *d_rec, const float *d_pd,
                            const float *d_cd, const float *d_gdiff, const float *d_gweight, const float *d_grec_add, float *o_grec,
                            float *o_gpd, float *o_gcd) {
    const size_t hw = (size_t)h->H * h->W;
    const PhotoMapsBwdPlan pl = photo_maps_bwd_plan(d_gdiff != nullptr, d_gweight != nullptr, o_grec != nullptr, o_gpd != nullptr, o_gcd != nullptr);
    if (pl.zero_rec) HIPCHK(h, hipMemsetAsync(o_grec, 0, N * 3 * hw * sizeof(float), h->stream));
    if (pl.zero_pd) HIPCHK(h, hipMemsetAsync(o_gpd, 0, N * hw * sizeof(float), h->stream));
    if (pl.zero_cd) HIPCHK(h, hipMemsetAsync(o_gcd, 0, N * hw * sizeof(float), h->stream));
    if (!pl.launch) return TCSFM_OK;
    PhotoGradParams P;
    P.tgt = d_tgt; P.rec = d_rec; P.pd = d_pd; P.cd = d_cd;
    P.g_diff = pl.rec_on ? d_gdiff : nullptr; P.g_weight = pl.dep_on ? d_gweight : nullptr; P.g_rec_add = d_grec_add;
    P.g_rec = pl.rec_on ? o_grec : nullptr; P.g_pd = pl.dep_on ? o_gpd : nullptr; P.g_cd = pl.dep_on ? o_gcd : nullptr;
    P.H = h->H; P.W = h->W; P.wl = o->w_l1 / 3.f; P.ws = o->w_ssim / 3.f;
    hipLaunchKernelGGL(k_photo_bwd, tile_grid_of(h, N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

// The shared front of the two smooth-loss forwards: the scratch -- N means (double), then the blocks' partial sums, carved from the next
// staging slot -- and the two launches that fill it.
struct SmoothFront {
    SmoothScratch s;
    float *scratch;
    SmoothFront(Staging &st, int N) : s(smooth_scratch(N, (size_t)st.h->H * st.h->W)), scratch((float *)st.scratch(s.bytes)) {}
    double *mean() const { return reinterpret_cast<double *>(scratch); }
    float *partial() const { return scratch + s.partial_off; }
    void launch(tcsfm_ctx *h, int N, const float *d_disp, const float *d_img) const {
        hipLaunchKernelGGL(k_smooth_mean, dim3(N), dim3(1024), 0, h->stream, d_disp, h->H * h->W, mean());
        hipLaunchKernelGGL(k_smooth, dim3(s.nb, N), dim3(256), 0, h->stream, d_disp, d_img, (const double *)mean(), h->H, h->W, partial());
    }
};

// the window loss (optimizer.py:47-86) and its backward: csrc/window_loss_kernel.h
int window_loss_args(tcsfm_handle h, const tcsfm_opts *o, const char *who, int B, int S, int argmin, int inverse, const float *fwd_diff,
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

WindowLossParams window_loss_params(tcsfm_handle h, const tcsfm_opts *o, Staging &st, int B, int S, int argmin, int inverse,
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

// the scale recovery's scratch (keys of every plane, 256 bins + 4 state words) ...
int reserve_scale(tcsfm_ctx *h) {
    RESERVE(h, h->scale_keys, (size_t)h->max_pairs * h->H * h->W);
    RESERVE(h, h->scale_hist, 260);
    return TCSFM_OK;
}
// ... and k_ground over n depth planes: their keys, and the height and mask maps where wanted
void launch_ground(tcsfm_ctx *h, hipStream_t stream, int n, const float *depth, const float *K, int k_stride, float *height, float *mask, unsigned *keys) {
    GroundParams G;
    G.depth = depth; G.K = K; G.height = height; G.mask = mask; G.keys = keys; G.H = h->H; G.W = h->W; G.err = h->err_word.dev; G.k_stride = k_stride;
    hipLaunchKernelGGL(k_ground, pixel_grid(h, n), dim3(256), 0, stream, G);
}

// k_ground + k_median_frames over `n` depth planes on `stream`: two launches, one workgroup of the second per plane.
// TCSFM_MEDIAN_LDS_KEYS (measurement and test hook, read at every call): the masked keys a workgroup keeps in LDS after its first
// pass, 0 .. kMedianLdsKeys (the default); a frame with more reads its plane in every round.  The results do not depend on it.
void launch_frame_scales(tcsfm_ctx *h, hipStream_t stream, int n, const float *depth, const float *K, int k_stride, unsigned *keys,
                         float real_cam_height, float *scale, float *median, int *count) {
    launch_ground(h, stream, n, depth, K, k_stride, nullptr, nullptr, keys);
    const char *lds_env = getenv("TCSFM_MEDIAN_LDS_KEYS");
    const int lds_keys = lds_env ? atoi(lds_env) : kMedianLdsKeys;
    hipLaunchKernelGGL(k_median_frames, dim3(n), dim3(kMedianThreads), 0, stream, (const unsigned *)keys, h->H * h->W, lds_keys, real_cam_height, scale, median, count);
}

// the host results of an evaluation entry: pose_evaluate's records behind the staged call
int evaluate(Staging &st, const char *entry, PoseCall &c, int nimg, int mode, std::vector<double> &host) {
    if (st.ready(entry)) return st.rc;
    return pose_evaluate(c, nimg, mode, host);
}
PoseCall pose_call_of(tcsfm_ctx *h, const tcsfm_opts *o, int N, int B, int S, const PairArgs &d, const float *ls) {
    PoseCall c{h, o, N, B, S};
    c.tgt = d.tgt; c.src = d.src; c.dt = d.depth_t; c.ds = d.depth_s; c.pose_in = d.pose; c.K = d.K; c.ls_in = ls;
    return c;
}

}  // namespace

int tcsfm_disp_to_depth(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, float *scaled, float *depth) {
    if (int rc = op_enter(h, o, -1, disp && n >= 1, "tcsfm_disp_to_depth: bad argument")) return rc;
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    Staging st(h, o);
    const float *d_in = st.in("disp", disp, (size_t)n);
    float *d_s = st.out("scaled_disp", scaled, (size_t)n), *d_d = st.out("depth", depth, (size_t)n);
    st.bless("scaled_disp", "disp"); st.bless("depth", "disp");      // k_disp_to_depth: a thread loads disp[i] before it stores element i
    if (st.ready("tcsfm_disp_to_depth")) return st.rc;
    hipLaunchKernelGGL(k_disp_to_depth, dim3(pixel_blocks((size_t)n)), dim3(256), 0, h->stream, d_in, d_s, d_d, (long long)n,
                       1.f / o->max_depth, 1.f / o->min_depth);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_disp_to_depth_backward(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, const float *g_scaled, const float *g_depth,
                                 float *g_disp) {
    if (int rc = op_enter(h, o, -1, disp && g_disp && n >= 1, "tcsfm_disp_to_depth_backward: bad argument")) return rc;
    if (!g_scaled && !g_depth) return fail(h, TCSFM_E_ARG, "tcsfm_disp_to_depth_backward: no cotangent given");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    Staging st(h, o);
    const float *d_in = st.in("disp", disp, (size_t)n), *d_gs = st.in("g_scaled", g_scaled, (size_t)n), *d_gd = st.in("g_depth", g_depth, (size_t)n);
    float *d_out = st.out("g_disp", g_disp, (size_t)n);
    // k_disp_to_depth_bwd: a thread loads its float4 (or tail element) of all three inputs before its one store to the same elements
    st.bless("g_disp", "disp"); st.bless("g_disp", "g_scaled"); st.bless("g_disp", "g_depth");
    if (st.ready("tcsfm_disp_to_depth_backward")) return st.rc;
    // float4 accesses need 16-byte alignment of every array in use: otherwise the scalar tail takes everything
    const DispBwdSplit sp = disp_bwd_split((long long)n, (((uintptr_t)d_in | (uintptr_t)d_gs | (uintptr_t)d_gd | (uintptr_t)d_out) & 15) == 0);
    hipLaunchKernelGGL(k_disp_to_depth_bwd, dim3(pixel_blocks((size_t)sp.threads)), dim3(256), 0, h->stream, d_in, d_gs, d_gd, d_out,
                       (long long)n, sp.n4, 1.f / o->max_depth, 1.f / o->min_depth);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_ssim(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, float *out) {
    if (int rc = op_enter(h, o, -1, x && y && out && planes >= 1, "tcsfm_ssim: bad argument")) return rc;
    Staging st(h, o);
    const size_t n = (size_t)h->H * h->W * planes;
    const float *d_x = st.in("x", x, n), *d_y = st.in("y", y, n);
    float *d_o = st.out("out", out, n);
    if (st.ready("tcsfm_ssim")) return st.rc;
    hipLaunchKernelGGL(k_ssim, pixel_grid(h, planes), dim3(256), 0, h->stream, d_x, d_y, d_o, h->H, h->W);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_ssim_backward(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, const float *g_out, float *g_x,
                        float *g_y) {
    if (int rc = op_enter(h, o, -1, x && y && g_out && planes >= 1, "tcsfm_ssim_backward: bad argument")) return rc;
    if (!g_x && !g_y) return fail(h, TCSFM_E_ARG, "tcsfm_ssim_backward: no output wanted");
    if (planes > 65535) return fail(h, TCSFM_E_ARG, "tcsfm_ssim_backward: more than 65535 planes");
    Staging st(h, o);
    const size_t n = (size_t)h->H * h->W * planes;
    SsimGradParams P;
    P.x = st.in("x", x, n); P.y = st.in("y", y, n); P.g_out = st.in("g_out", g_out, n);
    P.g_x = st.out("g_x", g_x, n); P.g_y = st.out("g_y", g_y, n);
    P.H = h->H; P.W = h->W;
    if (st.ready("tcsfm_ssim_backward")) return st.rc;
    hipLaunchKernelGGL(k_ssim_bwd, tile_grid_of(h, planes), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_warp(tcsfm_handle h, const tcsfm_opts *o, int N, const float *src, const float *depth_t, const float *depth_s,
               const float *pose, const float *K, float *img_rec, float *valid, float *proj_depth, float *comp_depth) {
    if (int rc = op_enter(h, o, N, src && depth_t && depth_s && pose && K, "tcsfm_warp: NULL input")) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp takes depth maps (call tcsfm_disp_to_depth first)");
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const PairArgs d = stage_pairs(st, {nullptr, src, depth_t, depth_s, pose, K}, false, N);
    float *d_rec = st.out("img_rec", img_rec, N * 3 * hw), *d_valid = st.out("valid", valid, N * hw), *d_pd = st.out("proj_depth", proj_depth, N * hw), *d_cd = st.out("comp_depth", comp_depth, N * hw);
    if (st.ready("tcsfm_warp")) return st.rc;
    if (int rc = launch_warp(h, o, N, d, d_rec, d_valid, d_pd, d_cd, nullptr)) return rc;
    return st.finish();
}

int tcsfm_warp_posenet_input(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                             const float *depth_s, const float *pose, const float *K, float *posenet_in, float *valid) {
    if (int rc = op_enter(h, o, N, tgt && src && depth_t && depth_s && pose && K && posenet_in, "tcsfm_warp_posenet_input: NULL argument")) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp_posenet_input takes depth maps");
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const PairArgs d = stage_pairs(st, {tgt, src, depth_t, depth_s, pose, K}, true, N);
    float *d_out = st.out("posenet_in", posenet_in, N * 6 * hw), *d_valid = st.out("valid", valid, N * hw);
    if (st.ready("tcsfm_warp_posenet_input")) return st.rc;
    if (int rc = launch_warp(h, o, N, d, nullptr, d_valid, nullptr, nullptr, d_out)) return rc;
    return st.finish();
}

int tcsfm_warp_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *src, const float *depth_t, const float *depth_s,
                        const float *pose, const float *K, const float *g_rec, const float *g_proj_depth, const float *g_comp_depth,
                        float *d_depth_t, float *d_depth_s, float *d_pose) {
    if (int rc = op_enter(h, o, N, src && depth_t && depth_s && pose && K, "tcsfm_warp_backward: NULL input")) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_warp_backward takes depth maps (call tcsfm_disp_to_depth first)");
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const PairArgs d = stage_pairs(st, {nullptr, src, depth_t, depth_s, pose, K}, false, N);
    const float *d_grec = st.in("g_rec", g_rec, N * 3 * hw), *d_gpd = st.in("g_proj_depth", g_proj_depth, N * hw), *d_gcd = st.in("g_comp_depth", g_comp_depth, N * hw);
    float *o_dt = st.out("d_depth_t", d_depth_t, N * hw), *o_ds = st.out("d_depth_s", d_depth_s, N * hw), *o_pose = st.out("d_pose", d_pose, (size_t)N * 6);
    if (st.ready("tcsfm_warp_backward")) return st.rc;
    if (int rc = warp_backward_dev(h, o, N, d, d_grec, d_gpd, d_gcd, o_dt, o_ds, o_pose, false)) return rc;
    return st.finish();
}

int tcsfm_photometric_maps_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *img_rec, const float *proj_depth,
                                    const float *comp_depth, const float *g_diff, const float *g_weight, float *g_rec, float *g_proj_depth,
                                    float *g_comp_depth) {
    if (int rc = op_enter(h, o, N, tgt && img_rec && proj_depth && comp_depth, "tcsfm_photometric_maps_backward: NULL input")) return rc;
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    const float *d_tgt = st.in("tgt", tgt, N * 3 * hw), *d_rec = st.in("img_rec", img_rec, N * 3 * hw), *d_pd = st.in("proj_depth", proj_depth, N * hw), *d_cd = st.in("comp_depth", comp_depth, N * hw);
    const float *d_gdiff = st.in("g_diff", g_diff, N * hw), *d_gweight = st.in("g_weight", g_weight, N * hw);
    float *o_grec = st.out("g_rec", g_rec, N * 3 * hw), *o_gpd = st.out("g_proj_depth", g_proj_depth, N * hw), *o_gcd = st.out("g_comp_depth", g_comp_depth, N * hw);
    if (st.ready("tcsfm_photometric_maps_backward")) return st.rc;
    if (int rc = photo_maps_backward_dev(h, o, N, d_tgt, d_rec, d_pd, d_cd, d_gdiff, d_gweight, nullptr, o_grec, o_gpd, o_gcd)) return rc;
    return st.finish();
}

int tcsfm_photometric_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                               const float *depth_s, const float *pose, const float *K, const float *g_diff, const float *g_weight,
                               const float *g_img_rec, float *d_depth_t, float *d_depth_s, float *d_pose) {
    if (int rc = op_enter(h, o, N, tgt && src && depth_t && depth_s && pose && K, "tcsfm_photometric_backward: NULL input")) return rc;
    if (o->depth_is_disp) return fail(h, TCSFM_E_ARG, "tcsfm_photometric_backward takes depth maps (call tcsfm_disp_to_depth first)");
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const PairArgs d = stage_pairs(st, {tgt, src, depth_t, depth_s, pose, K}, true, N);
    const float *d_gdiff = st.in("g_diff", g_diff, N * hw), *d_gweight = st.in("g_weight", g_weight, N * hw), *d_gimg = st.in("g_img_rec", g_img_rec, N * 3 * hw);
    float *o_dt = st.out("d_depth_t", d_depth_t, N * hw), *o_ds = st.out("d_depth_s", d_depth_s, N * hw), *o_pose = st.out("d_pose", d_pose, (size_t)N * 6);
    if (st.ready("tcsfm_photometric_backward")) return st.rc;
    // the cotangents that reach the warp: g_rec = (assembly's, from g_diff) + g_img_rec; g_proj_depth, g_comp_depth from g_weight
    const PhotoBwdPlan pl = photo_bwd_plan(d_gdiff != nullptr, d_gweight != nullptr, d_gimg != nullptr, o_dt || o_ds || o_pose);
    const float *cot[3][3] = {{nullptr, d_gimg, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};      // [g_rec | g_pd | g_cd][COT_*]
    if (pl.fwd64) {
        const size_t plane = (size_t)h->max_pairs * hw;
        RESERVE(h, h->pgrad_fwd, 5 * plane);
        RESERVE(h, h->pgrad_cot, 5 * plane);
        float *f_rec = h->pgrad_fwd, *f_pd = h->pgrad_fwd + 3 * plane, *f_cd = h->pgrad_fwd + 4 * plane;
        float *c_rec = h->pgrad_cot, *c_pd = h->pgrad_cot + 3 * plane, *c_cd = h->pgrad_cot + 4 * plane;
        if (int rc = run_init(h, o, N, d.pose, nullptr, d.K, 0)) return rc;
        WarpFwd64Params P;
        P.src = d.src; P.depth_t = d.depth_t; P.depth_s = d.depth_s; P.pc = h->pconst; P.st = h->state;
        P.rec = pl.fwd_rec ? f_rec : nullptr; P.pd = pl.fwd_depth ? f_pd : nullptr; P.cd = pl.fwd_depth ? f_cd : nullptr; P.H = h->H; P.W = h->W;
        hipLaunchKernelGGL(k_warp_fwd64, pixel_grid(h, N), dim3(256), 0, h->stream, P);
        HIPCHK(h, hipGetLastError());
        if (int rc = photo_maps_backward_dev(h, o, N, d.tgt, f_rec, f_pd, f_cd, d_gdiff, d_gweight, d_gimg, pl.fwd_rec ? c_rec : nullptr,
                                             pl.fwd_depth ? c_pd : nullptr, pl.fwd_depth ? c_cd : nullptr)) return rc;
        cot[0][COT_ASSEMBLED] = c_rec; cot[1][COT_ASSEMBLED] = c_pd; cot[2][COT_ASSEMBLED] = c_cd;
    }
    if (int rc = warp_backward_dev(h, o, N, d, cot[0][pl.g_rec], cot[1][pl.g_pd], cot[2][pl.g_cd], o_dt, o_ds, o_pose, pl.fwd64)) return rc;
    return st.finish();
}

int tcsfm_photometric(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                      const float *depth_s, const float *pose, const float *K, float *diff, float *valid, float *weight,
                      float *auto_err, float *auto_mask, float *img_rec) {
    if (int rc = op_enter(h, o, N, tgt && src && depth_t && depth_s && pose && K, "tcsfm_photometric: NULL input")) return rc;
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    const PairArgs d = stage_pairs(st, {tgt, src, depth_t, depth_s, pose, K}, true, N);
    float *outs[6] = {diff, valid, weight, auto_err, auto_mask, img_rec}, *d_out[6];
    static const char *const out_names[6] = {"diff", "valid", "weight", "auto_err", "auto_mask", "img_rec"};
    for (int i = 0; i < 6; i++) d_out[i] = st.out(out_names[i], outs[i], (i == 5 ? 3 : 1) * N * hw);
    if (st.ready("tcsfm_photometric")) return st.rc;
    if (int rc = run_pack(h, o, N, d.tgt, d.src, d.depth_t, d.depth_s)) return rc;
    if (int rc = run_init(h, o, N, d.pose, nullptr, d.K, 0)) return rc;
    LinParams P = lin_params(h, o, 6);
    P.o_diff = d_out[0]; P.o_valid = d_out[1]; P.o_weight = d_out[2]; P.o_auto_err = d_out[3]; P.o_auto_mask = d_out[4]; P.o_rec = d_out[5];
    launch_lin(h, P, N, 6, false, MODE_MAPS);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_linearize(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                    const float *depth_s, const float *pose, const float *log_scale, const float *K, double *Hmat, double *g,
                    double *stats) {
    if (int rc = op_enter(h, o, N, tgt && src && depth_t && depth_s && pose && K, "tcsfm_linearize: NULL input")) return rc;
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const PairArgs d = stage_pairs(st, {tgt, src, depth_t, depth_s, pose, K}, true, N);
    PoseCall c = pose_call_of(h, o, N, 0, 0, d, st.in("log_scale", log_scale, (size_t)N));
    const size_t np = (size_t)np_of(o);
    st.host_out("Hmat", Hmat, N * np * np * sizeof(double)); st.host_out("g", g, N * np * sizeof(double)); st.host_out("stats", stats, (size_t)N * 4 * sizeof(double));
    std::vector<double> host;
    if (int rc = evaluate(st, "tcsfm_linearize", c, N, MODE_LIN, host)) return rc;
    unpack_lin_records(host, N, (int)np, Hmat, g, stats);
    return TCSFM_OK;
}

int tcsfm_linearize_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                           const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *log_scale,
                           double *Hmat, double *g, double *stats) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (B < 1 || S < 1 || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_linearize_window: need 1 <= 2*B*S <= max_pairs");
    const int N = 2 * B * S;
    if (int rc = op_enter(h, o, N, tgt && srcs && depth_t && depth_s && pose && K, "tcsfm_linearize_window: NULL input")) return rc;
    Staging st(h, o);
    if (int rc = stage_K(st, K, B)) return rc;
    const size_t np = (size_t)np_of(o);
    const PairArgs d = stage_pairs(st, {tgt, srcs, depth_t, depth_s, pose, K}, true, true, "pose", B, (size_t)B * S, N);
    const float *d_ls = st.in("log_scale", log_scale, (size_t)N);
    PoseCall c = pose_call_of(h, o, N, B, S, d, np == 7 ? d_ls : nullptr);
    st.host_out("Hmat", Hmat, N * np * np * sizeof(double)); st.host_out("g", g, N * np * sizeof(double)); st.host_out("stats", stats, (size_t)N * 4 * sizeof(double));
    std::vector<double> host;
    if (int rc = evaluate(st, "tcsfm_linearize_window", c, N, MODE_LIN, host)) return rc;
    unpack_lin_records(host, N, (int)np, Hmat, g, stats);
    return TCSFM_OK;
}

int tcsfm_loss_surface(tcsfm_handle h, const tcsfm_opts *o, const float *tgt, const float *src, const float *depth_t,
                       const float *depth_s, const float *K, int P, const float *poses, double *cost_out) {
    if (int rc = op_enter(h, o, P, tgt && src && depth_t && depth_s && poses && K && cost_out, "tcsfm_loss_surface: NULL argument")) return rc;
    Staging st(h, o);
    if (int rc = stage_K(st, K, 1)) return rc;
    tcsfm_opts oo = *o;
    oo.refine = TCSFM_REFINE_POSE;
    const PairArgs d = stage_pairs(st, {tgt, src, depth_t, depth_s, poses, K}, true, false, "poses", 1, 1, P);
    PoseCall c = pose_call_of(h, &oo, P, 0, 0, d, nullptr);
    st.host_out("cost_out", cost_out, (size_t)P * sizeof(double));
    std::vector<double> host;
    if (int rc = evaluate(st, "tcsfm_loss_surface", c, 1, MODE_COST, host)) return rc;
    const int rec = 6 * 6 + 6 + 4;
    for (int i = 0; i < P; i++) cost_out[i] = host[(size_t)i * rec + 42];
    return TCSFM_OK;
}

int tcsfm_scale_recovery(tcsfm_handle h, const tcsfm_opts *o, int N, const float *depth, const float *K, float real_cam_height,
                         int pad_to_batch, float *scale_out, float *median_out, float *height_out, float *mask_out) {
    if (int rc = op_enter(h, o, N, depth && K && scale_out, "tcsfm_scale_recovery: NULL argument")) return rc;
    if (h->H < 5 || h->W < 5) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery: image too small");
    Staging st(h, o);
    if (int rc = stage_K(st, K, N)) return rc;
    const size_t hw = (size_t)h->H * h->W;
    if (int rc = reserve_scale(h)) return rc;
    const float *d_depth = st.in("depth", depth, N * hw), *d_K = st.in("K", K, (size_t)N * 9);
    float *d_scale = st.out("scale_out", scale_out, (size_t)1), *d_med = st.out("median_out", median_out, (size_t)1), *d_h = st.out("height_out", height_out, N * hw), *d_m = st.out("mask_out", mask_out, N * hw);
    if (st.ready("tcsfm_scale_recovery")) return st.rc;
    HIPCHK(h, hipMemsetAsync(h->scale_hist, 0, 260 * sizeof(unsigned), h->stream));
    launch_ground(h, h->stream, N, d_depth, d_K, 9, d_h, d_m, h->scale_keys);
    // the reference pads the batch to config['minibatch'] with copies of image 0 (dnet_layers.py:307-311): weight image 0
    const int w0 = 1 + (pad_to_batch > N ? pad_to_batch - N : 0);
    unsigned *hist = h->scale_hist, *state = h->scale_hist + 256;
    const int nb = median_hist_blocks(hw);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_sel_hist, dim3(nb, N), dim3(256), 0, h->stream, (const unsigned *)h->scale_keys, (int)hw, w0,
                           (const unsigned *)state, shift, hist);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(64), 0, h->stream, hist, state, shift, real_cam_height, d_scale, d_med);
    }
    HIPCHK(h, hipGetLastError());
    return st.finish();
}

int tcsfm_scale_recovery_frames(tcsfm_handle h, const tcsfm_opts *o, int N, const void *depth, const void *K, float real_cam_height,
                                void *scale_out, void *median_out, int *count_out) {
    if (int rc = op_enter(h, o, N, depth && K && scale_out, "tcsfm_scale_recovery_frames: NULL argument")) return rc;
    if (h->H < 5 || h->W < 5) return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery_frames: image too small");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_scale_recovery_frames: host_ptrs must be 0 (device pointers); a host caller has the sequence calls (tcsfm_sequence_scale)");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("depth", depth, (size_t)N * hw * sizeof(float)); a.in("K", K, (size_t)N * 9 * sizeof(float));
    a.out("scale_out", scale_out, (size_t)N * sizeof(float)); a.out("median_out", median_out, (size_t)N * sizeof(float));
    a.out("count_out", count_out, (size_t)N * sizeof(int));
    if (int rc = check_overlap(h, "tcsfm_scale_recovery_frames", a)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc = pending_error(h)) return rc;
    if (int rc = check_intrinsics(h, o, (const float *)K, N)) return rc;
    if (int rc = reserve_scale(h)) return rc;
    launch_frame_scales(h, h->stream, N, (const float *)depth, (const float *)K, 9, h->scale_keys, real_cam_height, (float *)scale_out,
                        (float *)median_out, count_out);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int tcsfm_smooth_loss(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, double *loss_out) {
    if (int rc = op_enter(h, o, N, disp && img && loss_out, "tcsfm_smooth_loss: NULL argument")) return rc;
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    const float *d_disp = st.in("disp", disp, N * hw), *d_img = st.in("img", img, N * 3 * hw);
    const SmoothFront front(st, N);
    st.host_out("loss_out", loss_out, sizeof(double));
    if (st.ready("tcsfm_smooth_loss")) return st.rc;
    front.launch(h, N, d_disp, d_img);
    HIPCHK(h, hipGetLastError());
    std::vector<float> hp(front.s.n_partial);
    HIPCHK(h, hipMemcpyAsync(hp.data(), front.partial(), hp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double sx = 0.0, sy = 0.0;
    for (size_t i = 0; i < hp.size(); i += 2) { sx += hp[i]; sy += hp[i + 1]; }
    *loss_out = sx / ((double)N * h->H * (h->W - 1)) + sy / ((double)N * (h->H - 1) * h->W);
    return TCSFM_OK;
}

int tcsfm_smooth_loss_device(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, float *loss_out,
                             double *stats_out) {
    if (int rc = op_enter(h, o, N, disp && img && loss_out && stats_out, "tcsfm_smooth_loss_device: NULL argument")) return rc;
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_device: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    const float *d_disp = st.in("disp", disp, N * hw), *d_img = st.in("img", img, N * 3 * hw);
    float *d_loss = st.out("loss_out", loss_out, (size_t)1);
    double *d_stats = st.out("stats_out", stats_out, (size_t)N * 3);
    const SmoothFront front(st, N);
    if (st.ready("tcsfm_smooth_loss_device")) return st.rc;
    front.launch(h, N, d_disp, d_img);
    hipLaunchKernelGGL(k_smooth_reduce, dim3(1), dim3(256), 0, h->stream, (const float *)front.partial(), (const double *)front.mean(), N, front.s.nb, h->H, h->W,
                       d_stats, d_loss);
    HIPCHK(h, hipGetLastError());
    return st.finish();          // (device pointers: no copy, no synchronisation)
}

int tcsfm_smooth_loss_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, const double *stats,
                               const float *g_loss, float *g_disp) {
    if (int rc = op_enter(h, o, N, disp && img && stats && g_loss && g_disp, "tcsfm_smooth_loss_backward: NULL argument")) return rc;
    if (h->H < 2 || h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_smooth_loss_backward: image too small");
    Staging st(h, o);
    const size_t hw = (size_t)h->H * h->W;
    SmoothGradParams P;
    P.disp = st.in("disp", disp, N * hw); P.img = st.in("img", img, N * 3 * hw); P.stats = st.in("stats", stats, (size_t)N * 3); P.g_loss = st.in("g_loss", g_loss, (size_t)1);
    P.g_disp = st.out("g_disp", g_disp, N * hw);
    P.H = h->H; P.W = h->W; P.N = N;
    if (st.ready("tcsfm_smooth_loss_backward")) return st.rc;
    hipLaunchKernelGGL(k_smooth_bwd, pixel_grid(h, N), dim3(256), 0, h->stream, P);
    HIPCHK(h, hipGetLastError());
    return st.finish();
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
    const int nbx = window_loss_grid(P.hw, WL_UNITS).nbx;      // the grid: a function of the shape only
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
    hipLaunchKernelGGL(k_window_loss_bwd, dim3(window_loss_grid(G.in.hw, WL_UNITS).nb_bwd, B), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    return st.finish();
}
