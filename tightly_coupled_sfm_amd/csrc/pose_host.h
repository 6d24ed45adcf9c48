// Host side of the pose modes (include/tcsfm.h: tcsfm_refine, tcsfm_refine_window, the merged pose sequence of the queued calls,
// tcsfm_linearize, tcsfm_linearize_window, tcsfm_loss_surface): one driver (PoseDriver) in steps.  What a call stages and which steps its
// schedule has is call_plan.h's (no HIP there); here is what is launched, in which order, on the handle's stream.  Part of tcsfm_api.hip,
// the library's only translation unit: included after context.h (tcsfm_ctx, Staging, the argument checks, the profiling brackets), before dense_host.h, which
// uses the helpers below (run_pack, init_params, lin_params, solve_params, launch_lin, launch_solve, the trace helpers).
#pragma once
#include "call_plan.h"

static_assert(POSE_STEP_COST == MODE_COST && POSE_STEP_LIN == MODE_LIN, "the plan's step names are k_linearize's modes");

namespace {

// TCSFM_WINDOW_REFERENCE (window forms only): the coupling of the pairs' costs, see include/tcsfm.h
void apply_window_rule(const tcsfm_ctx *h, const tcsfm_opts *o, int win_B, int win_S, int N, LinParams &P, SolveParams &S) {
    if (!win_B || o->window_rule != TCSFM_WINDOW_REFERENCE) return;
    P.rule = 1;
    P.fwd_noauto = o->argmin ? 0 : win_B * win_S;      // optimizer.py:71-73: without argmin the forward term has no auto-mask
    S.rule = 1; S.grp_fwd = win_B * win_S; S.n_pairs = N;
    S.scale_fwd = o->argmin ? 1.0 : 0.25; S.scale_inv = 0.25;
    S.b_dc = (double)o->w_dc / ((double)win_B * win_S * (double)h->H * (double)h->W);   // :83-86: mean over all S*B maps
    if (o->w_pose_consist > 0.f) {       // :95-96: 0.1 (poses + poses_inv).abs().mean() over the S B x 6 entries
        S.w_pc = (double)o->w_pose_consist / (6.0 * win_B * win_S); S.pc_eps = (double)o->irls_eps; S.pose_lin = h->pose_lin;
    }
}

// k_linearize's SSIM gradient in its adjoint form (kernels.h, ADJ) or as the round-3 neighbour-visiting pass B: TCSFM_ADJOINT=0/1,
// read once per process (default: see adjoint_default below; both forms are exact, they differ in rounding only)
constexpr int kAdjointDefault = 0;
bool use_adjoint() {
    static const int v = [] { const char *e = getenv("TCSFM_ADJOINT"); return e ? (atoi(e) != 0) : (kAdjointDefault != 0); }();
    return v != 0;
}

template <int NP, bool DC, int MODE, bool ADJ>
void launch_lin_a(tcsfm_ctx *h, const LinParams &P, int N) {
    dim3 grid(h->nblk, N), block(TILE_NT);
    const bool sel = MODE != MODE_MAPS && P.sel_S > 1;   // window form with the min over sources: selection inside the kernel
    if (MODE != MODE_MAPS && P.trace != nullptr) {       // parity tests: the decision-recording build
        if (sel) hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, true, true, ADJ>), grid, block, 0, h->stream, P);
        else hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, false, true, ADJ>), grid, block, 0, h->stream, P);
    } else if (MODE != MODE_MAPS && !ADJ && P.tshare != 0) {       // window forms of the pose modes: the shared-pack instantiations (kernels.h TSH)
        if (sel) hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, true, false, false, false, MODE != MODE_MAPS>), grid, block, 0, h->stream, P);
        else hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, false, false, false, false, MODE != MODE_MAPS>), grid, block, 0, h->stream, P);
    } else if (sel)
        hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, true, false, ADJ>), grid, block, 0, h->stream, P);
    else
        hipLaunchKernelGGL((k_linearize<NP, DC, MODE, TILE_W, TILE_H, TILE_NT, false, false, ADJ>), grid, block, 0, h->stream, P);
}
template <int NP, bool DC, int MODE>
void launch_lin_t(tcsfm_ctx *h, const LinParams &P, int N) {
    if (MODE == MODE_LIN && use_adjoint()) launch_lin_a<NP, DC, MODE, MODE == MODE_LIN>(h, P, N);
    else launch_lin_a<NP, DC, MODE, false>(h, P, N);
}

void launch_lin(tcsfm_ctx *h, const LinParams &P_in, int N, int np, bool dc, int mode, int prof_class = 0) {
    LinParams P = P_in;
    if (prof_class == 0) take_stamp(h, P, (size_t)h->nblk * N); else P.stamp = nullptr;
    P.one_generation = (size_t)h->nblk * N <= 512;          // 256 CUs x 2 resident workgroups
    ProfScope prof(h, prof_class);
    if (np == 6) {
        if (mode == MODE_MAPS) launch_lin_t<6, false, MODE_MAPS>(h, P, N);
        else if (mode == MODE_COST) launch_lin_t<6, false, MODE_COST>(h, P, N);
        else if (dc) launch_lin_t<6, true, MODE_LIN>(h, P, N);
        else launch_lin_t<6, false, MODE_LIN>(h, P, N);
    } else {
        if (mode == MODE_MAPS) launch_lin_t<7, false, MODE_MAPS>(h, P, N);
        else if (mode == MODE_COST) launch_lin_t<7, false, MODE_COST>(h, P, N);
        else if (dc) launch_lin_t<7, true, MODE_LIN>(h, P, N);
        else launch_lin_t<7, false, MODE_LIN>(h, P, N);
    }
}

// TCSFM_SOLVE_LEAN=1: the 1024-thread form of the solve kernel for SE(3) calls without the pose-consistency term -- measured SLOWER than
// the 256-thread kernel (6.0 vs 5.3 us in-kernel, profiles/r05_solve_ab.txt): default off, kept for A/B runs
bool use_lean_solve() {
    static const int v = [] { const char *e = getenv("TCSFM_SOLVE_LEAN"); return e ? atoi(e) : 0; }();
    return v != 0;
}
// lean: k_solve_lean (the caller has checked that the call is on the SE(3) chart and carries no pose-consistency term)
void launch_solve_as(tcsfm_ctx *h, const SolveParams &S, int N, int np, bool lean) {
    ProfScope prof(h, 1);
    if (np == 6) { if (lean) hipLaunchKernelGGL((k_solve_lean<6>), dim3(N), dim3(1024), 0, h->stream, S); else hipLaunchKernelGGL((k_solve<6>), dim3(N), dim3(TC_SOLVE_NT), 0, h->stream, S); }
    else { if (lean) hipLaunchKernelGGL((k_solve_lean<7>), dim3(N), dim3(1024), 0, h->stream, S); else hipLaunchKernelGGL((k_solve<7>), dim3(N), dim3(TC_SOLVE_NT), 0, h->stream, S); }
}
void launch_solve(tcsfm_ctx *h, const SolveParams &S, int N, int np) {
    launch_solve_as(h, S, N, np, S.param == TCSFM_PARAM_SE3 && !(S.w_pc > 0.0) && use_lean_solve());      // (decided by the options of the call: every launch of a call takes the same kernel)
}

// decision trace (tcsfm_debug_trace) of linearisation `lin` of a call over N pairs: [lin][N][H*W] bits, [lin][N] decisions
void trace_at(const tcsfm_ctx *h, int lin, int N, LinParams &P, SolveParams &S) {
    const size_t hw = (size_t)h->H * h->W;
    P.trace = h->trace_bits ? h->trace_bits + (size_t)lin * N * hw : nullptr;
    S.trace_decide = h->trace_decide ? h->trace_decide + (size_t)lin * N : nullptr;
}
// ... whose buffers must hold every linearisation of the call's schedule (call_plan.h: pose_n_lin, the figure the schedule is made of)
int trace_check(tcsfm_ctx *h, const tcsfm_opts *o, int N) {
    const long long n_lin = pose_n_lin(o->solver, o->n_iters);
    if (h->trace_bits && n_lin * N * (long long)h->H * h->W > h->trace_bits_cap) return fail(h, TCSFM_E_ARG, "tcsfm_debug_trace: bits buffer too small for this call");
    if (h->trace_decide && n_lin * N > h->trace_decide_cap) return fail(h, TCSFM_E_ARG, "tcsfm_debug_trace: decide buffer too small for this call");
    return TCSFM_OK;
}
// tcsfm_linearize / tcsfm_linearize_window under a trace: ONE linearisation, bits [0][N][H*W]; no decision is taken, `decide` stays untouched
int trace_lin_once(tcsfm_ctx *h, int N, LinParams &P) {
    if (h->trace_bits && N * (long long)h->H * h->W > h->trace_bits_cap) return fail(h, TCSFM_E_ARG, "tcsfm_debug_trace: bits buffer too small for this call");
    P.trace = h->trace_bits;
    return TCSFM_OK;
}

int np_of(const tcsfm_opts *o) { return o->refine == TCSFM_REFINE_POSE_SCALE ? 7 : 6; }
int nacc_of(int np) { return np == 6 ? AccLayout<6>::NACC : AccLayout<7>::NACC; }

InitParams init_params(tcsfm_ctx *h, const tcsfm_opts *o, int N, const float *pose, const float *ls, const float *K, int shared) {
    InitParams I;
    I.pose = pose; I.log_scale = ls; I.K = K; I.st = h->state; I.pc = h->pconst; I.N = N; I.shared_image = shared;
    I.lambda0 = o->lambda0;
    I.K_mod = 0;
    I.err = h->err_word.dev;
    I.pose_lin = (o->window_rule == TCSFM_WINDOW_REFERENCE && o->w_pose_consist > 0.f) ? h->pose_lin : nullptr;
    return I;
}

// Group tickets must be zero when k_linearize starts: zeroed at create, re-zeroed by the reducers after every launch; only a call that
// failed midway can leave them dirty, and whoever is about to linearise cleans them here.
int zero_tickets(tcsfm_ctx *h) {
    HIPCHK(h, hipMemsetAsync(h->tickets, 0, (size_t)h->max_pairs * h->ngrp_alloc * sizeof(int), h->stream));
    return TCSFM_OK;
}
int clean_tickets(tcsfm_ctx *h) {
    if (!h->tickets_dirty) return TCSFM_OK;
    if (int rc = zero_tickets(h)) return rc;
    h->tickets_dirty = false;
    return TCSFM_OK;
}

// The pointer tables of n > 1 queued calls of B x S windows merged into ONE sequence: the kernels' table of inputs and, per call, the
// outputs (log-scales: pose + scale calls; depth maps: dense calls).  Filled in one place for both kinds.
struct MergedCalls {
    CoalTab ct;
    float *pose_out[TC_MAX_COAL], *ls_out[TC_MAX_COAL], *depth_out[TC_MAX_COAL];
    MergedCalls(const std::vector<CallArgs> &calls, int B, int S) {
        memset(&ct, 0, sizeof(ct));
        ct.ncall = (int)calls.size(); ct.cB = B; ct.cS = S;
        for (int i = 0; i < ct.ncall; i++) {
            const CallArgs &q = calls[i];
            ct.tgt[i] = q.tgt; ct.src[i] = q.src; ct.dt[i] = q.depth_t; ct.ds[i] = q.depth_s; ct.K[i] = q.K; ct.pose[i] = q.pose_in; ct.ls[i] = q.log_scale_in;
            pose_out[i] = q.pose_out; ls_out[i] = q.log_scale_out; depth_out[i] = q.depth_out;
        }
    }
};

// init == nullptr: pack only.  Otherwise the pair initialisation rides in the same launch (needs N == Nimg).
int run_pack(tcsfm_ctx *h, const tcsfm_opts *o, int Nimg, const float *tgt, const float *src, const float *dt, const float *ds,
             const InitParams *init = nullptr, int win_B = 0, int win_S = 0, float *depth_copy = nullptr, const WinOff *wo = nullptr,
             const CoalTab *ct = nullptr, float *depth_copy3 = nullptr, int *zero_ints = nullptr, int zero_n = 0, float *const *ct_depth3 = nullptr,
             bool tshare = false) {
    PackParams P;
    P.depth_out2 = depth_copy; P.depth_out3 = depth_copy3; P.zero_ints = zero_ints; P.zero_n = zero_n;
    P.tshare = tshare ? 1 : 0;
    if (tshare && !(ct || win_B > 0)) return fail(h, TCSFM_E_ARG, "internal: the shared-pack form needs a window-form pack");
    P.c_out3 = (ct && ct_depth3) ? 1 : 0;
    for (int i = 0; i < TC_MAX_COAL; i++) P.c_depth_out3[i] = (ct && ct_depth3 && i < ct->ncall) ? ct_depth3[i] : nullptr;
    if (wo) P.win_off = *wo; else P.win_off.on = 0;
    memset(&P.init, 0, sizeof(P.init));
    P.win_B = win_B; P.win_S = win_S;
    if (init) {
        if (int rc = clean_tickets(h)) return rc;
        P.init = *init;
    }
    P.tgt = tgt; P.src = src; P.depth_t = dt; P.depth_s = ds;
    P.tgtpack = h->tgtpack; P.srcpack = h->srcpack; P.depth_out = h->depth_work;
    P.H = h->H; P.W = h->W; P.N = Nimg;
    P.wl = o->w_l1 / 3.f; P.ws = o->w_ssim / 3.f;
    P.depth_is_disp = o->depth_is_disp;
    P.min_disp = o->depth_is_disp ? 1.f / o->max_depth : 0.f;
    P.max_disp = o->depth_is_disp ? 1.f / o->min_depth : 0.f;
    if (ct ? Nimg != 2 * ct->cS * ct->ncall * ct->cB : (win_B > 0 && Nimg != 2 * win_S * win_B))
        return fail(h, TCSFM_E_ARG, "internal: a window-form pack covers the 2 S B directed pairs of its windows");
    {
        ProfScope prof(h, 2);
        // window forms: one row of workgroups per FORWARD pair, which packs its inverse too (pack_body)
        const int rows = (ct || win_B > 0) ? Nimg / 2 : Nimg;
        const unsigned ptiles = (unsigned)(((h->W + PT_W - 1) / PT_W) * ((h->H + PT_H - 1) / PT_H));       // 64 x 4 pixel tiles (pack_body)
        if (ct) hipLaunchKernelGGL(k_pack_coal, dim3(ptiles, rows), dim3(256), 0, h->stream, P, *ct);
        else hipLaunchKernelGGL(k_pack, dim3(ptiles, rows), dim3(256), 0, h->stream, P);
    }
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int run_init(tcsfm_ctx *h, const tcsfm_opts *o, int N, const float *pose, const float *ls, const float *K, int shared) {
    if (int rc = zero_tickets(h)) return rc;      // (every time, whatever the mark says: this covers an aborted earlier call)
    InitParams I = init_params(h, o, N, pose, ls, K, shared);
    hipLaunchKernelGGL(k_init, dim3((N + 63) / 64), dim3(64), 0, h->stream, I);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

// Small tile grids (KITTI 640x192: 240 workgroups per pair) skip the in-launch group reduction: the solve kernel sums the
// workgroup records itself with all loads in flight (one batch of <= 32 per thread), which is cheaper than the
// publish / ticket / last-arriver tail of every linearisation.  Larger grids keep the two-level reduction.
int direct_records(const tcsfm_ctx *h) { return h->nblk <= 256; }

LinParams lin_params(tcsfm_ctx *h, const tcsfm_opts *o, int np) {
    LinParams P;
    memset(&P, 0, sizeof(P));
    P.tgtpack = h->tgtpack; P.srcpack = h->srcpack; P.depth_t = h->depth_work; P.pc = h->pconst; P.partials = h->partials; P.blockrec = h->blockrec; P.tickets = h->tickets;
    P.H = h->H; P.W = h->W; P.tiles_x = h->tiles_x; P.tiles_y = h->tiles_y; P.nacc = nacc_of(np); P.ngrp = h->ngrp; P.ngrp_pad = h->ngrp_pad;
    P.wl = o->w_l1 / 3.f; P.ws = o->w_ssim / 3.f; P.eps = o->irls_eps; P.automask = o->automask;
    P.direct = direct_records(h);
    return P;
}

SolveParams solve_params(tcsfm_ctx *h, const tcsfm_opts *o, int np, int shared) {
    SolveParams S;
    memset(&S, 0, sizeof(S));
    S.partials = h->partials; S.st = h->state; S.pc = h->pconst; S.stats = nullptr; S.lin_out = h->lin_out;
    S.ngrp = h->ngrp; S.nacc = nacc_of(np); S.np = np; S.has_dc = o->w_dc > 0.f;
    if (direct_records(h)) { S.partials = h->blockrec; S.ngrp = h->nblk; }
    S.n_iters = o->n_iters; S.solver = o->solver; S.param = o->param;
    S.b_dc = (double)o->w_dc / ((double)h->H * (double)h->W);
    S.lambda_up = o->lambda_up; S.lambda_down = o->lambda_down; S.lambda_min = o->lambda_min;
    S.prior_scale = np == 7 ? (double)o->prior_scale : 0.0;
    S.shared_image = shared;
    S.dbg = h->dbg_stamps;
    return S;
}

// frame-level pack cache of a sequence call (kernels.h k_frame_pack / k_pack_cached): the ring's packed frames, and where this call's windows start
struct FrameCache { const float4 *fpack; const float *fdepth; int slot0, tpos; };

// One pose call, inputs already on the device.  N directed pairs: the pair form (win_B == 0, one image set per pair; shared: ONE image
// set behind all N poses), a win_B x win_S window, or merged calls (m): m->ct.ncall queued calls of cB x cS windows run as ONE sequence
// over win_B = ncall cB targets, inputs and outputs go through the pointer tables.  Null outputs are not wanted.
struct PoseCall {
    tcsfm_ctx *h;
    const tcsfm_opts *o;
    int N, win_B, win_S;
    const float *tgt, *src, *dt, *ds, *K, *pose_in, *ls_in;
    float *pose_out = nullptr, *ls_out = nullptr, *stats = nullptr;
    const WinOff *wo = nullptr;
    const FrameCache *fc = nullptr;
    const MergedCalls *m = nullptr;
    int shared = 0;
};

// The steps of a pose call: one of the packs, couple(), then iterate() + finish_no_iters() (a refinement) or lin_once() + records() (one
// evaluation at the given poses).  The constructor fills the three parameter blocks; nothing is launched before a pack.
struct PoseDriver {
    const PoseCall &c;
    tcsfm_ctx *h;
    const tcsfm_opts *o;
    const PosePlan &pl;
    const int N, np;
    const size_t hw;
    InitParams I;
    LinParams P;
    SolveParams S;

    PoseDriver(const PoseCall &c_, const PosePlan &pl_)
        : c(c_), h(c_.h), o(c_.o), pl(pl_), N(c_.N), np(pl_.np), hw((size_t)c_.h->H * c_.h->W),
          I(init_params(c_.h, c_.o, c_.N, c_.pose_in, c_.ls_in, c_.K, c_.shared)), P(lin_params(c_.h, c_.o, pl_.np)), S(solve_params(c_.h, c_.o, pl_.np, c_.shared)) {
        I.K_mod = c.win_B;
        P.shared_image = c.shared;
        S.stats = c.stats;
    }

    // the pair form of the one-evaluation entries: nimg image sets packed, then the pairs' constants by k_init
    int pack_pairs(int nimg) {
        if (int rc = run_pack(h, o, nimg, c.tgt, c.src, c.dt, c.ds)) return rc;
        return run_init(h, o, N, c.pose_in, c.ls_in, c.K, c.shared);
    }
    // pair form, window or merged windows, the pair initialisation riding in the pack launch.  tshare: window forms pack every image ONCE
    // (LinParams::tshare, kernels.h)
    int pack(bool tshare) {
        if (int rc = run_pack(h, o, N, c.tgt, c.src, c.dt, c.ds, &I, c.win_B, c.win_S, nullptr, c.wo, c.m ? &c.m->ct : nullptr, nullptr, nullptr, 0, nullptr, tshare)) return rc;
        if (tshare) { P.tshare = 1; P.tshare_sb = N / 2; }
        return TCSFM_OK;
    }
    // sequence call: rgb + depth were packed once per frame when they landed; only the pair-specific part is formed here
    int pack_cached() {
        if (int rc = clean_tickets(h)) return rc;
        PackCachedParams C;
        C.fpack = c.fc->fpack; C.tgtpack = h->tgtpack; C.pair_src = h->pair_idx; C.pair_dep = h->pair_idx + h->max_pairs;
        C.H = h->H; C.W = h->W; C.N = N; C.win_B = c.win_B; C.win_S = c.win_S; C.slot0 = c.fc->slot0; C.tpos = c.fc->tpos; C.win_off = *c.wo;
        C.wl = o->w_l1 / 3.f; C.ws = o->w_ssim / 3.f; C.init = I;
        {
            ProfScope prof(h, 2);
            hipLaunchKernelGGL(k_pack_cached, dim3((unsigned)((hw + 255) / 256), pl.pack_rows), dim3(256), 0, h->stream, C);      // (a row per forward pair)
        }
        HIPCHK(h, hipGetLastError());
        P.srcpack = c.fc->fpack; P.depth_t = c.fc->fdepth; P.pair_src = C.pair_src; P.pair_dep = C.pair_dep;
        return TCSFM_OK;
    }
    // what ties the pairs of a call together: the min over a window's sources (evaluated inside k_linearize<SEL>), the window rule, and
    // the per-call outputs of merged calls
    void couple() {
        if (pl.n_sel) { P.sel_B = c.win_B; P.sel_S = c.win_S; }
        apply_window_rule(h, o, c.win_B, c.win_S, N, P, S);
        if (!c.m) return;
        S.c_ncall = c.m->ct.ncall; S.c_B = c.m->ct.cB; S.c_S = c.m->ct.cS;
        for (int i = 0; i < c.m->ct.ncall; i++) { S.c_pose_out[i] = c.m->pose_out[i]; S.c_ls_out[i] = c.m->ls_out[i]; }
    }
    // the plan's schedule: a linearisation and a solve per step; the emitting step writes the refined pose
    int iterate() {
        if (int rc = trace_check(h, o, N)) return rc;
        const bool dc = o->w_dc > 0.f;
        for (int i = 0; i < pl.n_lin; i++) {
            const PoseStep s = pl.step(i);
            trace_at(h, i, N, P, S);
            launch_lin(h, P, N, np, dc, s.lin);
            S.it = s.it; S.mode = s.solve_mode;
            S.pose_out = s.emit ? c.pose_out : nullptr; S.log_scale_out = s.emit ? c.ls_out : nullptr;
            launch_solve(h, S, N, np);
        }
        HIPCHK(h, hipGetLastError());
        return TCSFM_OK;
    }
    int finish_no_iters() {      // nothing to solve: round-trip the pose through SE(3)
        if (!pl.finish) return TCSFM_OK;
        FinishParams F;
        F.st = h->state; F.pose_out = c.pose_out; F.log_scale_out = c.ls_out; F.N = N;
        hipLaunchKernelGGL(k_finish, dim3((N + 63) / 64), dim3(64), 0, h->stream, F);
        HIPCHK(h, hipGetLastError());
        return TCSFM_OK;
    }
    // ONE evaluation at the given poses (mode: MODE_LIN, or MODE_COST, which records no trace); k_solve's mode 2 exports the records
    int lin_once(int mode) {
        if (mode == MODE_LIN)
            if (int rc = trace_lin_once(h, N, P)) return rc;
        launch_lin(h, P, N, np, o->w_dc > 0.f, mode);
        S.mode = 2;
        if (mode == MODE_COST) S.has_dc = 0;  // only the three scalar sums are live in cost mode
        launch_solve(h, S, N, np);
        HIPCHK(h, hipGetLastError());
        return TCSFM_OK;
    }
    // ... the per-pair records (H [np][np], g [np], 4 statistics) to the host; synchronises
    int records(std::vector<double> &host) {
        host.resize((size_t)N * (np * np + np + 4));
        HIPCHK(h, hipMemcpyAsync(host.data(), h->lin_out, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return TCSFM_OK;
    }
};

// ... into the caller's arrays (each optional)
void unpack_lin_records(const std::vector<double> &host, int N, int np, double *Hmat, double *g, double *stats) {
    const int rec = np * np + np + 4;
    for (int n = 0; n < N; n++) {
        const double *r = &host[(size_t)n * rec];
        if (Hmat) memcpy(Hmat + (size_t)n * np * np, r, sizeof(double) * np * np);
        if (g) memcpy(g + (size_t)n * np, r + np * np, sizeof(double) * np);
        if (stats) memcpy(stats + (size_t)n * 4, r + np * np + np, sizeof(double) * 4);
    }
}

PosePlan pose_plan_of(const tcsfm_opts *o, int N, int win_B, int win_S, const MergedCalls *m = nullptr) {
    return pose_plan(N, win_B, win_S, m ? m->ct.ncall : 0, m ? m->ct.cB : 0, m ? m->ct.cS : 0, o->solver, o->n_iters, o->refine, o->argmin);
}

// One evaluation of N pairs at given poses, results as host records: tcsfm_linearize (nimg == N), tcsfm_loss_surface (nimg == 1: one
// image set under every pose) and, window != 0, tcsfm_linearize_window (c.win_B x c.win_S).  c: staged by the entry point.
int pose_evaluate(PoseCall c, int nimg, int mode, std::vector<double> &host) {
    const PosePlan pl = pose_plan_of(c.o, c.N, c.win_B, c.win_S);
    c.shared = (!c.win_B && nimg == 1 && c.N > 1) ? 1 : 0;
    PoseDriver d(c, pl);
    if (int rc = c.win_B ? d.pack(false) : d.pack_pairs(nimg)) return rc;
    d.couple();
    if (int rc = d.lin_once(mode)) return rc;
    return d.records(host);
}

// The refinement behind tcsfm_refine (win_B == 0: one image set per pair), tcsfm_refine_window (win_B x win_S windows; wo / fc: a sequence
// call's source offsets and frame cache) and the merged sequence of queued calls (m: every array comes per call from the tables -- device
// pointers, validated at enqueue -- and `a` is the first call's).  Checks, staging, then the driver's steps.
int pose_refine(tcsfm_ctx *h, const tcsfm_opts *o, int N, int win_B, int win_S, const CallArgs &a, const WinOff *wo, const FrameCache *fc,
                const MergedCalls *m = nullptr) {
    int rc = check_common(h, o, N);
    if (rc) return rc;
    if (!a.tgt || !a.src || !a.depth_t || !a.depth_s || !a.pose_in || !a.pose_out || !a.K) return fail(h, TCSFM_E_ARG, "tcsfm_refine: NULL input");
    Staging st(h, o);
    if (st.rc) return st.rc;
    const PosePlan pl = pose_plan_of(o, N, win_B, win_S, m);
    if (!m && (rc = check_intrinsics(h, o, a.K, pl.nimg_t))) return rc;
    const size_t hw = (size_t)h->H * h->W;
    PoseCall c{h, o, N, win_B, win_S};
    c.tgt = st.in("tgt", a.tgt, pl.tgt(hw)); c.src = st.in("src", a.src, pl.src(hw)); c.dt = st.in("depth_t", a.depth_t, pl.depth_t(hw));
    c.ds = st.in("depth_s", a.depth_s, pl.depth_s(hw)); c.K = st.in("K", a.K, pl.K()); c.pose_in = st.in("pose_in", a.pose_in, pl.pose());
    const float *d_ls_in = st.in("log_scale_in", a.log_scale_in, pl.log_scale());
    c.ls_in = pl.np == 7 ? d_ls_in : nullptr;
    c.pose_out = st.out("pose_out", a.pose_out, pl.pose()); c.ls_out = st.out("log_scale_out", pl.np == 7 ? a.log_scale_out : nullptr, pl.log_scale());
    c.stats = st.out("stats_out", a.stats_out, pl.stats());
    c.wo = wo; c.fc = fc; c.m = m;
    if (st.ready(nullptr)) return st.rc;
    if (c.stats) HIPCHK(h, hipMemsetAsync(c.stats, 0, pl.stats() * sizeof(float), h->stream));
    PoseDriver d(c, pl);
    // window forms: every image packed ONCE (LinParams::tshare, kernels.h) -- TCSFM_TSHARE=0 keeps the round-4 layout (A/B hook)
    static const bool tshare_env = !(getenv("TCSFM_TSHARE") && atoi(getenv("TCSFM_TSHARE")) == 0);
    if ((rc = fc ? d.pack_cached() : d.pack(tshare_env && pl.window))) return rc;
    d.couple();
    if ((rc = d.iterate())) return rc;
    if ((rc = d.finish_no_iters())) return rc;
    return st.finish(o->host_ptrs == 1);   // host_ptrs == 2: pinned + asynchronous, the caller synchronises
}

}  // namespace
