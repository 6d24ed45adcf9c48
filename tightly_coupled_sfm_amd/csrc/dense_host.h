// Host side of the dense modes (include/tcsfm.h: tcsfm_refine_dense, tcsfm_refine_dense_window, tcsfm_linearize_dense_window*): three
// drivers behind dense_body -- the pair form (DensePair), the library's joint mode (DenseJoint) and the reference's loss (DenseRef).  The
// arithmetic -- capacities, tile grids, which part of which buffer a launch works on, the refusals -- is dense_plan.h's (no HIP there);
// here is what is launched, in which order, on which stream.  Part of tcsfm_api.hip, the library's only translation unit: included after
// pose_host.h, whose run_pack, lin_params, solve_params, launch_lin, launch_solve and trace helpers it uses.
//
// A driver is a per-call struct: reserve (every buffer the mode needs, every call: a no-op from the second identical call on, so nothing
// is allocated or freed under stream capture), pack, the parameter blocks, then linearise(lin) / solve(it) / update(it) per iteration.
#pragma once
#include "dense_plan.h"

namespace {

// lin_export of a reference-loss call: ONE linearisation at the given poses, nothing updated: host outputs of tcsfm_linearize_dense_window
struct DrefExport { double *scal, *g_pose; float *d_g_rho; const float *d_depth0; float *d_g_rho_src; /* [S B][H W] or null: tcsfm_linearize_dense_window_sources */ };

// One dense call, inputs already on the device.  B targets of S sources each; the pair form outside a window: S = 0 and B pairs.  Merged
// calls (ct): ncall queued calls of cB targets each run as ONE sequence over B = ncall cB targets, inputs and outputs go through the
// pointer tables.
struct DenseCall {
    tcsfm_ctx *h;
    const tcsfm_opts *o;
    int B, S;
    const float *tgt, *src, *dt, *ds, *K, *pose_in;
    float *pose_out, *depth_out, *stats;
    const WinOff *wo;
    const CoalTab *ct;
    float *const *ct_pose, *const *ct_depth;
    bool out_on_input;             // depth_out lies on depth_t or depth_s (honoured, include/tcsfm.h; refine_overlap finds it)
    const DrefExport *ex;
};

#define DENSE_RESERVE(buf, id)                                                                       \
    RESERVE(h, D.buf, cp.cap[id])

// What the three drivers share: the call, the plan and the pieces each of them would otherwise write out again.
struct DenseDriver {
    const DenseCall &c;
    tcsfm_ctx *h;
    const tcsfm_opts *o;
    DenseScratch &D;
    const DenseCaps &cp;           // the handle's, computed once at create
    DensePlan pl;
    tcsfm_opts oo;                 // the call's options as the pose-mode helpers take them (run_pack, lin_params, solve_params)
    size_t hw;
    int B, S, SB, N;
    bool lm, tr;
    dim3 px(int rows) const { return dim3((unsigned)((hw + 255) / 256), rows); }      // one thread per pixel of `rows` maps

    DenseDriver(const DenseCall &c_, int mode, unsigned flags)
        : c(c_), h(c_.h), o(c_.o), D(c_.h->dense), cp(c_.h->caps),
          pl(dense_plan(c_.h->caps, mode, c_.h->H, c_.h->W, c_.h->max_pairs, c_.B, c_.S, flags)), oo(*c_.o), hw((size_t)c_.h->H * c_.h->W), B(c_.B), S(c_.S),
          SB(pl.SB), N(pl.N), lm(c_.o->solver == TCSFM_SOLVER_LM), tr(c_.h->trace_bits != nullptr) {
        oo.refine = TCSFM_REFINE_POSE;
        oo.window_rule = TCSFM_WINDOW_PAIR;          // (the pose-mode coupling; the joint kernels take the rule through JointParams)
    }
    int refused() const { return pl.refusal ? fail(h, TCSFM_E_ARG, pl.refusal) : TCSFM_OK; }

    // the inverse pairs' view of a linearisation's inputs: S B pairs further on
    LinParams inverse_view(LinParams P) const {
        P.tgtpack += pl.inv(DB_TGTPACK); P.srcpack += pl.inv(DB_SRCPACK); P.depth_t += pl.inv(DB_DEPTH_WORK); P.pc += pl.inv(DB_PCONST);
        return P;
    }
    LinParams joint_grid(LinParams P) const {          // ... on the joint kernels' own tile grid
        P.tiles_x = pl.jtiles_x; P.tiles_y = pl.jtiles_y; P.ngrp = pl.jngrp; P.direct = 1;
        return P;
    }
    float *stats_inv() const { return c.stats ? c.stats + pl.inv(DB_STATS) * (o->n_iters + 1) * TCSFM_NSTAT : nullptr; }
    // decision trace (tcsfm_debug_trace) of linearisation `lin` from pair `first` on: [lin][N][H*W] bits, [lin][N] decisions
    unsigned short *trace_bits_at(int lin, size_t first) const { return tr ? h->trace_bits + ((size_t)lin * N + first) * hw : nullptr; }
    int *trace_decide_at(int lin, size_t first) const { return h->trace_decide ? h->trace_decide + (size_t)lin * N + first : nullptr; }
    // the selection masks of the forward pairs at the current poses and depths (the selection itself: ext_selected, inside the dense kernels)
    void select_pass(int n_sel) {
        LinParams M = lin_params(h, &oo, 6);
        M.o_diff = D.sel_maps.p; M.o_valid = D.sel_maps.p + pl.inv(DB_SEL_MAPS);
        launch_lin(h, M, n_sel, 6, false, MODE_MAPS, 2);
    }
    // merged calls: every call's own outputs, through the coalesce table
    template <class P> void coal_pose(P &p) const {
        if (!c.ct) return;
        p.c_ncall = c.ct->ncall; p.c_B = c.ct->cB; p.c_S = c.ct->cS;
        for (int i = 0; i < c.ct->ncall; i++) p.c_pose_out[i] = c.ct_pose[i];
    }
    template <class P> void coal_depth(P &p) const {
        if (!c.ct) return;
        p.c_ncall = c.ct->ncall; p.c_B = c.ct->cB;
        for (int i = 0; i < c.ct->ncall; i++) p.c_depth_out[i] = c.ct_depth[i];
    }
    void finish_no_iters(hipStream_t st) {     // nothing to solve: round-trip the poses through SE(3)
        if (o->n_iters != 0) return;
        FinishParams F;
        F.st = h->state; F.pose_out = c.pose_out; F.log_scale_out = nullptr; F.N = N;
        hipLaunchKernelGGL(k_finish, dim3((N + 63) / 64), dim3(64), 0, st, F);
    }
    int copy_out(hipStream_t st) {             // the work buffer's maps to the caller
        HIPCHK(h, hipMemcpyAsync(c.depth_out, h->depth_work, N * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
        return TCSFM_OK;
    }
    int reserve_pair_form(bool with_lm, bool with_sel) {      // per-pixel records, prior centres and steps of the pair-form dense kernels
        if (with_sel) DENSE_RESERVE(sel_maps, DB_SEL_MAPS);
        DENSE_RESERVE(dense_rec, DB_DENSE_REC); DENSE_RESERVE(depth0, DB_DEPTH0); DENSE_RESERVE(delta, DB_DELTA);
        if (with_lm) { DENSE_RESERVE(dense_rec_acc, DB_DENSE_REC_ACC); DENSE_RESERVE(depth_acc, DB_DEPTH_ACC); DENSE_RESERVE(lm_accept, DB_LM_ACCEPT); }
        return TCSFM_OK;
    }
    int reserve_joint() {                      // per-pixel records, workgroup records and per-target state of the joint kernels
        DENSE_RESERVE(jrec, DB_JREC); DENSE_RESERVE(jblockrec, DB_JBLOCKREC); DENSE_RESERVE(jstate, DB_JSTATE); DENSE_RESERVE(jdelta, DB_JDELTA);
        return TCSFM_OK;
    }
};

// ---- the library's JOINT mode of a window (include/tcsfm.h, tcsfm_refine_dense_window): the S forward pairs of every target share one
// depth map and are solved together (k_dense_joint / k_solve_joint / k_dense_joint_update); the inverse pairs run the pair-form dense
// kernels on offset views of the same scratch.
template <int NS>
struct DenseJoint : DenseDriver {
    // the joint kernel runs on its own tile grid, as under the reference's loss (third session of round 5): 256-thread workgroups, for S = 2 the
    // LEAN form of the kernel (161 VGPRs: three workgroups per CU instead of one 512-thread workgroup at 212-232)
    static constexpr int JTW = kJointTileW, JTH = kJointTileH, JNT = JTW * JTH;
    int n_sel;
    LinParams Pj, Pi;
    JointParams J;
    JointSolveParams Sj;
    JointUpdateParams Uj;
    SolveParams Si;
    DenseParams Dn;
    DenseUpdateParams Ui;
    DenseLmParams Ul;
    hipStream_t fs, is;            // the forward group's stream (the handle's) and the inverse pairs'

    explicit DenseJoint(const DenseCall &c_)
        : DenseDriver(c_, DENSE_JOINT, (c_.o->argmin ? DF_ARGMIN : 0) | (c_.o->solver == TCSFM_SOLVER_LM ? DF_LM : 0)) { n_sel = o->argmin ? SB : 0; }
    int reserve() {
        if (int rc = reserve_pair_form(lm, n_sel != 0)) return rc;
        if (int rc = reserve_joint()) return rc;
        if (lm) { DENSE_RESERVE(jrec_acc, DB_JREC_ACC); DENSE_RESERVE(jdepth_acc, DB_JDEPTH_ACC); }
        return TCSFM_OK;
    }
    int pack() {
        InitParams I = init_params(h, &oo, N, c.pose_in, nullptr, c.K, 0);
        I.K_mod = B;
        return run_pack(h, &oo, N, c.tgt, c.src, c.dt, c.ds, &I, B, S, D.depth0.p, c.wo);
    }
    void params_forward() {        // the forward group: joint
        Pj = joint_grid(lin_params(h, &oo, 6));
        if (n_sel) { Pj.ext_diff = D.sel_maps.p; Pj.ext_valid = D.sel_maps.p + pl.inv(DB_SEL_MAPS); Pj.n_ext = n_sel; Pj.ext_B = B; Pj.ext_S = S; }
        memset(&J, 0, sizeof(J));
        J.jrec = D.jrec.p; J.depth0 = D.depth0.p; J.jblockrec = D.jblockrec.p; J.lambda_depth = o->lambda_depth; J.w_prior = o->prior_depth;
        J.B = B; J.S = S; J.argmin = o->argmin ? 1 : 0;
        J.automask = 0;                             // own masks only without argmin, where the reference's forward term has no auto-mask (:71-73)
        memset(&Sj, 0, sizeof(Sj));
        Sj.jblockrec = D.jblockrec.p; Sj.js = D.jstate.p; Sj.st = h->state; Sj.pc = h->pconst; Sj.stats = c.stats; Sj.nblk = pl.jnblk; Sj.B = B;
        Sj.n_iters = o->n_iters; Sj.solver = o->solver; Sj.lambda_up = o->lambda_up; Sj.lambda_down = o->lambda_down; Sj.lambda_min = o->lambda_min;
        Sj.lambda0 = o->lambda0; Sj.delta_out = D.jdelta.p; Sj.accept_out = lm ? D.lm_accept.p : nullptr;
        memset(&Uj, 0, sizeof(Uj));
        Uj.jrec = D.jrec.p; Uj.jrec_acc = lm ? D.jrec_acc.p : nullptr; Uj.depth_acc = lm ? D.jdepth_acc.p : nullptr; Uj.delta = D.jdelta.p;
        Uj.accept = lm ? D.lm_accept.p : nullptr; Uj.depth = h->depth_work; Uj.depth_out = nullptr; Uj.hw = (int)hw; Uj.B = B; Uj.S = S; Uj.mode = 0;
        Uj.rho_lo = 1.f / o->max_depth; Uj.rho_hi = 1.f / o->min_depth;
    }
    void params_inverse() {        // the inverse pairs: the pair-form dense kernels on views offset by S B pairs
        Pi = inverse_view(lin_params(h, &oo, 6));
        Pi.tiles_x = pl.dtiles_x; Pi.tiles_y = pl.dtiles_y; Pi.ngrp = pl.dngrp; Pi.direct = 1;
        Pi.blockrec += pl.inv(DB_BLOCKREC);
        Si = solve_params(h, &oo, 6, 0);
        Si.partials = Pi.blockrec; Si.ngrp = pl.dnblk; Si.st = h->state + pl.inv(DB_STATE); Si.pc = h->pconst + pl.inv(DB_PCONST);
        Si.stats = stats_inv();
        Si.delta_out = D.delta.p + pl.inv(DB_DELTA); Si.accept_out = lm ? D.lm_accept.p + pl.inv(DB_LM_ACCEPT) : nullptr;
        float *depth_inv = h->depth_work + pl.inv(DB_DEPTH_WORK);
        Dn.dense_rec = D.dense_rec.p + pl.inv(DB_DENSE_REC); Dn.depth0 = D.depth0.p + pl.inv(DB_DEPTH0); Dn.lambda_depth = o->lambda_depth; Dn.w_prior = o->prior_depth;
        Dn.prev_rec = nullptr; Dn.prev_delta = D.delta.p; Dn.depth_next = nullptr; Dn.rho_lo = Uj.rho_lo; Dn.rho_hi = Uj.rho_hi;
        memset(&Ui, 0, sizeof(Ui));          // (no coalesce table: c_ncall = 0)
        Ui.dense_rec = Dn.dense_rec; Ui.delta = Si.delta_out; Ui.depth = depth_inv; Ui.depth_out = depth_inv; Ui.hw = (int)hw;
        Ui.rho_lo = Uj.rho_lo; Ui.rho_hi = Uj.rho_hi;
        Ul.rec_try = Dn.dense_rec; Ul.rec_acc = lm ? D.dense_rec_acc.p + pl.inv(DB_DENSE_REC_ACC) : nullptr; Ul.depth_acc = lm ? D.depth_acc.p + pl.inv(DB_DEPTH_ACC) : nullptr;
        Ul.depth = depth_inv; Ul.delta = Si.delta_out; Ul.accept = Si.accept_out; Ul.hw = (int)hw; Ul.rho_lo = Uj.rho_lo; Ul.rho_hi = Uj.rho_hi;
    }
    // The inverse pairs' refinement never meets the forward group's (different pairs, different scratch views): it runs on a second
    // stream beside it -- fork after the pack, join before the results are copied out -- so a call costs max(forward chain, inverse
    // chain) per iteration instead of their sum (80 -> ~50 us per iteration for the KITTI window at 640x192).  Under graph capture both
    // chains go on the handle's stream instead: a replayed graph with parallel branches needs more hardware queues than a process may
    // be given, and the chains never touch each other's data, so the results are the same bits.
    int fork() {
        if (!h->aux_stream) {
            HIPCHK(h, h->aux_stream.create());
            HIPCHK(h, h->aux_fork.create());
            HIPCHK(h, h->aux_join.create());
        }
        fs = h->stream; is = h->capturing ? h->stream : h->aux_stream;
        if (int rc = trace_check(h, o, N)) return rc;
        if (is != fs) {
            HIPCHK(h, hipEventRecord(h->aux_fork, fs));
            HIPCHK(h, hipStreamWaitEvent(is, h->aux_fork, 0));
        }
        return TCSFM_OK;
    }
    void linearise_inverse(int lin) {
        Pi.trace = trace_bits_at(lin, SB);
        Si.trace_decide = trace_decide_at(lin, SB);
        Pi.stamp = nullptr;
        const dim3 grid(pl.dnblk, SB), block(kDenseNT);
        if (tr) hipLaunchKernelGGL((k_dense_linearize<kDenseTileW, kDenseTileH, kDenseNT, true>), grid, block, 0, is, Pi, Dn);
        else hipLaunchKernelGGL((k_dense_linearize<kDenseTileW, kDenseTileH, kDenseNT>), grid, block, 0, is, Pi, Dn);
    }
    void solve_inverse(int it, int mode, bool writes_pose) {
        Si.it = it; Si.mode = mode; Si.pose_out = writes_pose ? c.pose_out + (size_t)SB * 6 : nullptr; Si.log_scale_out = nullptr;
        hipLaunchKernelGGL((k_solve<6>), dim3(SB), dim3(TC_SOLVE_NT), 0, is, Si);
    }
    void inverse_chain() {         // the inverse pairs, all iterations, on the second stream
        const int nit = o->n_iters;
        for (int it = 0; it < nit; it++) {
            linearise_inverse(it);
            solve_inverse(it, 0, !lm && it == nit - 1);
            if (lm) hipLaunchKernelGGL(k_dense_update_lm, px(SB), dim3(256), 0, is, Ul);
            else hipLaunchKernelGGL(k_dense_update, px(SB), dim3(256), 0, is, Ui);
        }
        if (lm && nit > 0) {
            linearise_inverse(nit);
            solve_inverse(nit, 1, true);
            hipLaunchKernelGGL(k_dense_final_lm, px(SB), dim3(256), 0, is, (const int *)Ul.accept, (const float *)Ul.depth_acc, Ul.depth, (int)hw);
        }
    }
    void linearise_forward(int lin) {
        Pj.trace = trace_bits_at(lin, 0);
        Sj.trace_decide = trace_decide_at(lin, 0);
        if (n_sel) select_pass(n_sel);       // at the current poses and the current SHARED depth
        take_stamp(h, Pj, (size_t)pl.jnblk * B);
        ProfScope prof(h, 0);
        if (tr) hipLaunchKernelGGL((k_dense_joint<NS, JTW, JTH, JNT, true>), dim3(pl.jnblk, B), dim3(JNT), 0, fs, Pj, J);
        else hipLaunchKernelGGL((k_dense_joint<NS, JTW, JTH, JNT>), dim3(pl.jnblk, B), dim3(JNT), 0, fs, Pj, J);
    }
    void solve_forward(int it, int mode, bool writes_pose) {
        Sj.it = it; Sj.mode = mode; Sj.pose_out = writes_pose ? c.pose_out : nullptr;
        hipLaunchKernelGGL((k_solve_joint<NS>), dim3(B), dim3(JSOLVE_NT), 0, fs, Sj);
    }
    void forward_chain() {         // the forward group, jointly, on the handle's stream
        const int nit = o->n_iters;
        for (int it = 0; it < nit; it++) {
            linearise_forward(it);
            solve_forward(it, 0, !lm && it == nit - 1);
            hipLaunchKernelGGL((k_dense_joint_update<NS>), px(B), dim3(256), 0, fs, Uj);
        }
        if (lm && nit > 0) {
            linearise_forward(nit);
            solve_forward(nit, 1, true);
            Uj.mode = 1;
            hipLaunchKernelGGL((k_dense_joint_update<NS>), px(B), dim3(256), 0, fs, Uj);
        }
    }
    int run() {
        int rc;
        if ((rc = refused()) || (rc = reserve()) || (rc = pack())) return rc;
        params_forward();
        params_inverse();
        if ((rc = fork())) return rc;
        inverse_chain();
        if (is != fs) HIPCHK(h, hipEventRecord(h->aux_join, is));
        forward_chain();
        if (is != fs) HIPCHK(h, hipStreamWaitEvent(fs, h->aux_join, 0));
        HIPCHK(h, hipGetLastError());
        finish_no_iters(h->stream);
        return copy_out(h->stream);
    }
};

// the fixed-point scatter sums of the reference-loss dense mode are zero between calls (their consumer clears them); after a fresh
// allocation, an export or a call that failed midway they are cleared here
int dref_clean(tcsfm_ctx *h) {
    if (!h->dref_dirty) return TCSFM_OK;
    DenseScratch &D = h->dense;
    if (D.dref_ext.p) HIPCHK(h, hipMemsetAsync(D.dref_ext.p, 0, D.dref_ext.cap * sizeof(long long), h->stream));
    if (D.dref_ext_src.p) HIPCHK(h, hipMemsetAsync(D.dref_ext_src.p, 0, D.dref_ext_src.cap * sizeof(long long), h->stream));
    if (D.jtick.p) HIPCHK(h, hipMemsetAsync(D.jtick.p, 0, D.jtick.cap * sizeof(int), h->stream));      // (a call that failed midway may have left tickets behind)
    h->dref_dirty = false;
    return TCSFM_OK;
}

// ---- dense window mode on the REFERENCE's loss (include/tcsfm.h, dense_ref_kernel.h): plain refinement, merged calls, free source maps,
// the quarter-resolution unknown, and the export of one linearisation.
template <int NS>
struct DenseRef : DenseDriver {
    using JL = JointLayout<NS>;
    // The joint kernel's own tile grid (round 5): 32 x 8 tiles of 256 threads by default.  At 256 VGPRs the kernel holds 8 waves per CU either
    // way; as TWO independent 4-wave workgroups their barriers and load phases no longer coincide (one workgroup's gathers run under the
    // other's arithmetic), which a single 8-wave workgroup cannot do -- at the price of a larger halo share (TC_JOINT_TILE_H=16: the round-4 grid).
    static constexpr int DTW = kJointTileW, DTH = kJointTileH, DNT = DTW * DTH;
    // The loss couples the windows of ONE call (batch normalisers, means over the call's maps): every merged call is a normaliser group of
    // its own (norm_B = cB targets), the per-map weights take the CALL's batch size Bc.
    int Bc, ngroups, norm_B;
    int nblk, nqblk, nq;           // workgroup records per target of the joint kernel; the quarter-resolution cell groups and cells
    bool sel, qres, free_src, pc, smooth, direct_out;
    const DrefExport *ex;
    hipStream_t st;
    float *maps_diff, *maps_valid;
    LinParams Pi, Pj, Pj2, F;
    SolveParams Si;
    JointParams J, J2;
    DrefSmoothParams Ds;
    JointSolveParams Sj, Sj2;
    JointUpdateParams Uj, Uj2;
    QresParams Q, Q2;

    static unsigned flags_of(const DenseCall &c) {
        const bool ex = c.ex != nullptr;
        return (c.o->argmin ? DF_ARGMIN : 0) | (!ex && c.o->depth_param == TCSFM_DEPTH_QUARTER ? DF_QRES : 0) | (!ex && c.o->free_source_depths != 0 ? DF_FREE_SRC : 0) |
               (ex ? DF_EXPORT : 0) | (ex && c.ex->d_g_rho_src ? DF_EXPORT_SRC : 0) | (c.ct ? DF_MERGED : 0);
    }
    explicit DenseRef(const DenseCall &c_) : DenseDriver(c_, DENSE_REF, flags_of(c_)), ex(c_.ex), st(c_.h->stream) {
        Bc = c.ct ? c.ct->cB : B; ngroups = c.ct ? c.ct->ncall : 1; norm_B = c.ct ? c.ct->cB : 0;
        nblk = pl.jnblk; nqblk = pl.nqblk; nq = pl.nq;
        sel = o->argmin && S > 1;
        // the reference's parametrisation (optimizer.py:194-198, 235-239): quarter-resolution unknown, x4 bilinear upsampling (dense_ref_kernel.h)
        qres = !ex && o->depth_param == TCSFM_DEPTH_QUARTER;
        // opts.free_source_depths: the inverse pairs as S B groups of one source (the joint kernel / solve / update on views offset by S B pairs)
        free_src = !ex && o->free_source_depths != 0;
        pc = o->w_pose_consist > 0.f && !ex;      // optimizer.py:95-96 as a term of this mode (the export of one linearisation leaves it out)
        smooth = o->w_smooth > 0.f && h->H > 1 && h->W > 1;
        oo.w_pose_consist = 0.f;                  // (the couplings are set explicitly: `pc`)
        // The pack leaves -- plain refinement with fixed source maps -- the inputs in the caller's depth output: its inverse slots (the
        // source maps) are final, the forward slots are overwritten by the last back-substitution ... unless the caller's depth_out lies on
        // depth_t or depth_s (out_on_input): output slot s B + b and input slot s B + b hold different maps and other workgroups of the pack
        // are still reading, so such a call leaves depth_out alone until the final copy from the work buffer, as the modes without a direct
        // output do (a merged sequence carries no such call: the queued form runs it at once)
        direct_out = !ex && !free_src && o->n_iters > 0 && (c.depth_out != nullptr || c.ct != nullptr) && !c.out_on_input;
    }
    int reserve() {
        // (with the pair-form and accepted-state records it never reads: where the buffers of a handle land moves its kernels' times by a percent)
        DENSE_RESERVE(sel_maps, DB_SEL_MAPS); DENSE_RESERVE(dense_rec, DB_DENSE_REC); DENSE_RESERVE(depth0, DB_DEPTH0); DENSE_RESERVE(delta, DB_DELTA);
        DENSE_RESERVE(jrec, DB_JREC); DENSE_RESERVE(jrec_acc, DB_JREC_ACC); DENSE_RESERVE(jdepth_acc, DB_JDEPTH_ACC); DENSE_RESERVE(jblockrec, DB_JBLOCKREC);
        DENSE_RESERVE(jstate, DB_JSTATE); DENSE_RESERVE(jdelta, DB_JDELTA); DENSE_RESERVE(jpart, DB_JPART);
        if (int rc = reserve_zeroed(D.jtick, cp.cap[DB_JTICK])) return rc;
        DENSE_RESERVE(dref_norms, DB_DREF_NORMS);
        if (int rc = reserve_sums(D.dref_ext, cp.cap[DB_DREF_EXT])) return rc;
        DENSE_RESERVE(dref_export, DB_DREF_EXPORT); DENSE_RESERVE(dref_smooth, DB_DREF_SMOOTH);
        if (qres) { DENSE_RESERVE(qres_rho, DB_QRES_RHO); DENSE_RESERVE(qres_rec, DB_QRES_REC); }
        if (free_src) {
            DENSE_RESERVE(jrec_src, DB_JREC_SRC); DENSE_RESERVE(jstate_src, DB_JSTATE_SRC); DENSE_RESERVE(jdelta_src, DB_JDELTA_SRC);
            if (int rc = reserve_sums(D.dref_ext_src, cp.cap[DB_DREF_EXT_SRC])) return rc;
            if (qres) { DENSE_RESERVE(qres_rho_src, DB_QRES_RHO_SRC); DENSE_RESERVE(qres_rec_src, DB_QRES_REC_SRC); }
        }
        return TCSFM_OK;
    }
    // what happens once after a fresh allocation keys on the buffer's own capacity having been 0: the tickets start at zero ...
    int reserve_zeroed(DevBuf<int> &b, size_t n) {
        if (b.cap) return TCSFM_OK;
        RESERVE(h, b, n);
        if (hipMemset(b.p, 0, n * sizeof(int)) != hipSuccess) { (void)b.release(); return fail(h, TCSFM_E_HIP, "hipMemset of the joint solve's tickets failed"); }
        return TCSFM_OK;
    }
    int reserve_sums(DevBuf<long long> &b, size_t n) {      // ... and fresh scatter sums are cleared before their first use (dref_clean)
        if (!b.cap) h->dref_dirty = true;
        RESERVE(h, b, n);
        return TCSFM_OK;
    }
    int pack() {       // the pack also zeroes the batch counters
        InitParams I = init_params(h, &oo, N, c.pose_in, nullptr, c.K, 0);
        I.K_mod = B;
        if (pc) I.pose_lin = h->pose_lin;            // buffer 0 of [2][N][12]: every pair's transform at the first linearisation
        if (int rc = run_pack(h, &oo, N, c.tgt, c.src, c.dt, c.ds, &I, c.ct ? 0 : B, S, D.depth0.p, c.wo, c.ct, direct_out && !c.ct ? c.depth_out : nullptr,
                              D.dref_norms.p, 2 * TC_MAX_COAL, c.ct ? c.ct_depth : nullptr)) return rc;
        if (ex && ex->d_depth0)       // the prior's centre given explicitly (slots of the forward pairs (0, b): index b)
            HIPCHK(h, hipMemcpyAsync(D.depth0.p, ex->d_depth0, (size_t)B * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
        return trace_check(h, o, N);
    }
    void params_inverse() {        // the inverse pairs: pose kernels on views offset by S B pairs, window rule REFERENCE (all of them are the rule's inverse group)
        Pi = inverse_view(lin_params(h, &oo, 6));
        Pi.blockrec += pl.inv(DB_BLOCKREC); Pi.tickets += pl.inv(DB_TICKETS); Pi.partials += pl.inv(DB_PARTIALS);
        Si = solve_params(h, &oo, 6, 0);
        Si.partials = direct_records(h) ? Pi.blockrec : Pi.partials;
        Si.st = h->state + pl.inv(DB_STATE); Si.pc = h->pconst + pl.inv(DB_PCONST); Si.lin_out = h->lin_out + pl.inv(DB_LIN_OUT);
        Si.rule = 1; Si.grp_fwd = 0; Si.n_pairs = SB; Si.scale_fwd = 1.0; Si.scale_inv = 0.25;
        Si.b_dc = (double)o->w_dc / ((double)(S * Bc) * (double)hw);
        Si.stats = stats_inv();
        Si.dbg = nullptr;          // (diagnostic stamps: the joint kernel's phases in this mode, not the pair solve's)
    }
    void params_forward() {        // the forward group: the joint kernel under the reference's rule
        Pj = joint_grid(lin_params(h, &oo, 6));
        if (sel) { Pj.ext_diff = maps_diff; Pj.ext_valid = maps_valid; Pj.n_ext = SB; Pj.ext_B = B; Pj.ext_S = S; }
        memset(&J, 0, sizeof(J));
        J.jrec = D.jrec.p; J.depth0 = D.depth0.p; J.jblockrec = D.jblockrec.p; J.w_prior = 0.f;
        J.lambda_depth = ex ? 1e20f : o->lambda_depth;      // (export: depth block frozen, the reduced right-hand side IS the pose gradient)
        J.B = B; J.S = S; J.argmin = o->argmin ? 1 : 0;
        J.automask = o->argmin ? o->automask : 0;     // own masks: with one source the min is the source itself; without argmin no auto-mask (:71-73)
        J.norms = D.dref_norms.p; J.norm_B = norm_B; J.ext2 = D.dref_ext.p; J.c_f = o->argmin ? 1.f : 0.25f;
        J.dbg = h->dbg_stamps;
        J.b_dc = o->w_dc / ((float)(S * Bc) * (float)hw); J.w_init_px = o->prior_init / ((float)Bc * (float)hw);
        J.sig_lo = 1.f / o->max_depth; J.sig_ir = 1.f / (1.f / o->min_depth - 1.f / o->max_depth);
        memset(&Ds, 0, sizeof(Ds));
        if (smooth) {       // optimizer.py:92-93: l_smooth_weight x [mean over B H (W-1) x-edges + mean over B (H-1) W y-edges]
            J.smooth = D.dref_smooth.p;
            J.w_smooth_x = o->w_smooth / ((float)Bc * (float)h->H * (float)(h->W - 1)); J.w_smooth_y = o->w_smooth / ((float)Bc * (float)(h->H - 1) * (float)h->W);
            Ds.depth = h->depth_work; Ds.tgtpack = h->tgtpack; Ds.out = D.dref_smooth.p; Ds.H = h->H; Ds.W = h->W;
            Ds.sig_lo = J.sig_lo; Ds.sig_ir = J.sig_ir; Ds.wx = J.w_smooth_x; Ds.wy = J.w_smooth_y;
        }
        memset(&Sj, 0, sizeof(Sj));
        {   // TCSFM_DEBUG_STAMPS=2: the phases of target 0's joint SOLVE instead (scripts/diag/solve_front_stamps.py)
            static const int which = [] { const char *e = getenv("TCSFM_DEBUG_STAMPS"); return e ? atoi(e) : 0; }();
            if (which == 2) { Sj.dbg = h->dbg_stamps; J.dbg = nullptr; }
        }
        Sj.jblockrec = D.jblockrec.p; Sj.js = D.jstate.p; Sj.st = h->state; Sj.pc = h->pconst; Sj.stats = c.stats; Sj.nblk = nblk; Sj.B = B;
        Sj.n_iters = o->n_iters; Sj.solver = TCSFM_SOLVER_GN; Sj.lambda_up = o->lambda_up; Sj.lambda_down = o->lambda_down; Sj.lambda_min = o->lambda_min;
        Sj.lambda0 = o->lambda0; Sj.delta_out = D.jdelta.p; Sj.accept_out = nullptr;
        Sj.norms = D.dref_norms.p; Sj.norm_B = norm_B; Sj.c_f = J.c_f;
        coal_pose(Sj);
        coal_pose(Si);
        if (c.ct) { Si.c_n0 = SB; for (int i = 0; i < c.ct->ncall; i++) Si.c_ls_out[i] = nullptr; }
        memset(&Uj, 0, sizeof(Uj));
        Uj.jrec = D.jrec.p; Uj.delta = D.jdelta.p; Uj.depth = h->depth_work; Uj.hw = (int)hw; Uj.B = B; Uj.S = S; Uj.mode = 0;
        Uj.rho_lo = 1.f / o->max_depth; Uj.rho_hi = 1.f / o->min_depth;
        Uj.srcpack_inv = h->srcpack + pl.inv(DB_SRCPACK); Uj.W = h->W; Uj.H = h->H;
    }
    // the quarter-resolution cells of the targets' maps and, with free source maps, of the source maps: the start is the quarter-resolution
    // projection of the input map, upsampled again (optimizer.py:194-196, 235); the prior's centre stays the full-resolution input
    // (`self.target_disparity`, :89-90)
    void params_qres() {
        memset(&Q, 0, sizeof(Q));
        if (qres) {
            J.qres = 1; J.rec_stride = pl.recs; Sj.nblk = pl.recs;
            Q.jrec = D.jrec.p; Q.qrec = D.qres_rec.p; Q.rho_q = D.qres_rho.p; Q.jblockrec = D.jblockrec.p; Q.delta = D.jdelta.p; Q.depth = h->depth_work;
            Q.srcpack_inv = Uj.srcpack_inv; Q.H = h->H; Q.W = h->W; Q.B = B; Q.S = S; Q.rec_stride = pl.recs; Q.rec_first = nblk;
            Q.rho_lo = Uj.rho_lo; Q.rho_hi = Uj.rho_hi;
            hipLaunchKernelGGL(k_qres_init, dim3((unsigned)((nq + 255) / 256), B), dim3(256), 0, st, Q);
            hipLaunchKernelGGL(k_qres_upsample, px(B), dim3(256), 0, st, Q);
            Q.norms_zero = D.dref_norms.p; Q.norms_n = 2 * ngroups;
        }
        Q2 = Q;
        if (qres && free_src) {      // the source maps in the same parametrisation: their quarter-resolution projection is the start (optimizer.py:194-196)
            Q2.jrec = D.jrec_src.p; Q2.qrec = D.qres_rec_src.p; Q2.rho_q = D.qres_rho_src.p; Q2.delta = D.jdelta_src.p;
            Q2.depth = h->depth_work + pl.inv(DB_DEPTH_WORK); Q2.srcpack_inv = h->srcpack; Q2.B = SB; Q2.S = 1; Q2.norms_zero = nullptr;
            hipLaunchKernelGGL(k_qres_init, dim3((unsigned)((nq + 255) / 256), SB), dim3(256), 0, st, Q2);
            hipLaunchKernelGGL(k_qres_upsample, px(SB), dim3(256), 0, st, Q2);
        }
    }
    // The source maps as S B groups of one source: every inverse pair as a group WITHOUT argmin is the reference's inverse term (0.25 / K_i,
    // own weights, valid x auto-mask, its depth-consistency term), its local unknowns the pair's pose and the source map it back-projects.
    // Serves the free-source mode and the export-with-sources path, which differ in the record buffer and the scatter-sum buffer.
    void source_groups(LinParams &P2, JointParams &G2, float *jrec, long long *ext2) {
        P2 = joint_grid(inverse_view(lin_params(h, &oo, 6)));
        G2 = J;
        G2.jrec = jrec; G2.depth0 = nullptr; G2.B = SB; G2.S = 1; G2.argmin = 0; G2.automask = o->automask;
        G2.norms = D.dref_norms.p + 1;                // the group's normaliser is K_i, its factor 0.25 (optimizer.py:79)
        G2.c_f = 0.25f; G2.w_init_px = 0.f; G2.smooth = nullptr; G2.w_smooth_x = G2.w_smooth_y = 0.f; G2.qres = 0; G2.rec_stride = 0;
        G2.ext2 = ext2; G2.ext_norm = D.dref_norms.p; G2.ext_c = J.c_f;
    }
    void params_free_sources() {   // ... their records behind the forward groups' in jblockrec: one solve launch and one update launch serve both
        Sj2 = Sj;
        Uj2 = Uj;
        source_groups(Pj2, J2, D.jrec_src.p, D.dref_ext_src.p);
        J2.jblockrec = D.jblockrec.p + pl.jrec2_off; Sj2.jblockrec = D.jblockrec.p + pl.jrec2_off; Q2.jblockrec = D.jblockrec.p + pl.jrec2_off;
        if (qres) { J2.qres = 1; J2.rec_stride = pl.recs; }
        Sj2.js = D.jstate_src.p; Sj2.st = h->state + pl.inv(DB_STATE); Sj2.pc = h->pconst + pl.inv(DB_PCONST); Sj2.B = SB; Sj2.nblk = pl.recs;
        Sj2.stats = stats_inv();
        Sj2.delta_out = D.jdelta_src.p; Sj2.norms = D.dref_norms.p + 1; Sj2.c_f = 0.25;
        Uj2.jrec = D.jrec_src.p; Uj2.delta = D.jdelta_src.p; Uj2.depth = h->depth_work + pl.inv(DB_DEPTH_WORK); Uj2.B = SB; Uj2.S = 1;
        Uj2.norms_zero = nullptr;                     // (the forward update zeroes the counters: it runs after both solves)
        Uj2.srcpack_inv = h->srcpack;                 // forward pair m samples source map m: the depth channel of ITS pack
    }
    // Round 5: with the source maps fixed a linearisation OPENS with one launch over all 2 S B pairs (k_linearize<FRONT>: the forward pairs'
    // selection and K_f, the inverse pairs' systems, K_i and their adjoint scatter) in place of the residual-map, count, scatter and
    // inverse-linearisation launches.  (second session: the free-source-map mode opens with the same launch -- every row light there, the
    // forward rows scattering the adjoint of their samples of the source maps -- and its two joint groups share ONE solve launch and ONE
    // update launch)
    void params_front() {
        F = lin_params(h, &oo, 6);
        F.front_fwd = SB; F.front_Bt = B; F.norm_B = norm_B; F.norms = D.dref_norms.p; F.ext2 = D.dref_ext.p;
        F.front_light = free_src ? 1 : 0; F.ext2_src = D.dref_ext_src.p;
        F.fwd_noauto = o->argmin ? 0 : SB;                       // optimizer.py:71-73: without argmin the forward term has no auto-mask
        F.one_generation = (size_t)pl.nblk * (SB + (sel ? B : SB)) <= 512;
        if (sel) { F.sel_B = B; F.sel_S = S; F.sel_out = maps_valid; Pj.ext_diff = nullptr; Pj.ext_valid = nullptr; Pj.n_ext = 0; Pj.sel_in = maps_valid; }
        Si.norms = D.dref_norms.p; Si.norm_Bt = B; Si.norm_B = norm_B;
    }
    void launch_front(int lin) {
        F.trace = trace_bits_at(lin, 0);
        F.stamp = nullptr;
        ProfScope prof(h, 2);
        const dim3 grid(pl.nblk, SB + (sel ? B : SB)), block(TILE_NT);     // inverse pairs, then the forward rows (under the selection: one per target)
        if (tr) {
            if (sel) hipLaunchKernelGGL((k_linearize<6, true, MODE_LIN, TILE_W, TILE_H, TILE_NT, true, true, false, true>), grid, block, 0, st, F);
            else hipLaunchKernelGGL((k_linearize<6, true, MODE_LIN, TILE_W, TILE_H, TILE_NT, false, true, false, true>), grid, block, 0, st, F);
        } else if (sel) hipLaunchKernelGGL((k_linearize<6, true, MODE_LIN, TILE_W, TILE_H, TILE_NT, true, false, false, true>), grid, block, 0, st, F);
        else hipLaunchKernelGGL((k_linearize<6, true, MODE_LIN, TILE_W, TILE_H, TILE_NT, false, false, false, true>), grid, block, 0, st, F);
    }
    void linearise(int lin) {
        Pi.trace = trace_bits_at(lin, SB);
        Si.trace_decide = trace_decide_at(lin, SB);
        launch_front(lin);
        Pj.trace = trace_bits_at(lin, 0);
        Sj.trace_decide = trace_decide_at(lin, 0);
        if (smooth) hipLaunchKernelGGL(k_dref_smooth, dim3(B), dim3(1024), 0, st, Ds);
        const bool both = free_src && !smooth;       // free source maps: the forward groups and the inverse pairs' groups of one source in ONE launch
        take_stamp(h, Pj, (size_t)nblk * (both ? B + SB : B));
        ProfScope prof(h, 0);
        if (both) {
            Pj2.trace = trace_bits_at(lin, SB);
            Pj2.stamp = Pj.stamp;                    // (stamps are indexed by the launch's grid)
            if (tr) hipLaunchKernelGGL((k_dense_joint2<NS, DTW, DTH, DNT, true>), dim3(nblk, B + SB), dim3(DNT), 0, st, Pj, J, Pj2, J2);
            else hipLaunchKernelGGL((k_dense_joint2<NS, DTW, DTH, DNT, false>), dim3(nblk, B + SB), dim3(DNT), 0, st, Pj, J, Pj2, J2);
            if (qres) hipLaunchKernelGGL((k_qres_schur2<NS>), dim3(nqblk, B + SB), dim3(256), 0, st, Q, Q2);      // both groups' cells
            return;
        }
        // (l_smooth is compiled into its own instantiations: without it -- the reference's drivers -- the S = 2 kernel is the LEAN form, three workgroups per CU)
        if (smooth) {
            if (tr) hipLaunchKernelGGL((k_dense_joint<NS, DTW, DTH, DNT, true, true, true>), dim3(nblk, B), dim3(DNT), 0, st, Pj, J);
            else hipLaunchKernelGGL((k_dense_joint<NS, DTW, DTH, DNT, false, true, true>), dim3(nblk, B), dim3(DNT), 0, st, Pj, J);
        } else if (tr) hipLaunchKernelGGL((k_dense_joint<NS, DTW, DTH, DNT, true, true, false>), dim3(nblk, B), dim3(DNT), 0, st, Pj, J);
        else hipLaunchKernelGGL((k_dense_joint<NS, DTW, DTH, DNT, false, true, false>), dim3(nblk, B), dim3(DNT), 0, st, Pj, J);
        if (qres && !free_src) hipLaunchKernelGGL((k_qres_schur<NS>), dim3(nqblk, B), dim3(256), 0, st, Q);
        if (free_src) {
            // Independent of the forward groups' launch above (own records behind theirs in jblockrec): one solve launch serves both.
            Pj2.trace = trace_bits_at(lin, SB);
            if (tr) hipLaunchKernelGGL((k_dense_joint<1, DTW, DTH, DNT, true, true, false>), dim3(nblk, SB), dim3(DNT), 0, st, Pj2, J2);
            else hipLaunchKernelGGL((k_dense_joint<1, DTW, DTH, DNT, false, true, false>), dim3(nblk, SB), dim3(DNT), 0, st, Pj2, J2);
            if (qres) hipLaunchKernelGGL((k_qres_schur2<NS>), dim3(nqblk, B + SB), dim3(256), 0, st, Q, Q2);      // both groups' cells
        }
    }
    // The gradient w.r.t. the SOURCE inverse-depth maps (held fixed by the refinement; leaves of the reference's optimize_depth_pred).
    // Their role mirrors the target map's: local in the inverse pair -- source_groups -- and sampled by the forward pair:
    // k_dref_scatter_src, in units of the forward factor a_f.  Oracle: dref_source_depth_gradient.
    int export_sources() {
        HIPCHK(h, hipMemsetAsync(D.dref_ext.p, 0, (size_t)SB * hw * 2 * sizeof(long long), st));
        LinParams M = lin_params(h, &oo, 6);              // residual maps of all pairs
        M.o_diff = maps_diff; M.o_valid = maps_valid;
        launch_lin(h, M, N, 6, false, MODE_MAPS, 2);      // (the forward pairs' residual maps: what k_dref_scatter_src weighs the samples with)
        LinParams Pp = lin_params(h, &oo, 6);             // the scatter of the forward pairs' samples of the source maps
        Pp.ext_diff = maps_diff; Pp.ext_valid = maps_valid; Pp.n_ext = SB; Pp.ext_B = B; Pp.ext_S = S;
        DrefPrepassParams Dp;
        Dp.diff = maps_diff; Dp.valid = maps_valid; Dp.norms = D.dref_norms.p; Dp.ext = D.dref_ext.p; Dp.B = B; Dp.S = S;
        Dp.argmin = o->argmin ? 1 : 0; Dp.automask = o->automask; Dp.eps = o->irls_eps;
        Dp.b_dc = o->w_dc / ((float)(S * Bc) * (float)hw);
        Dp.plain_dif = 0;
        hipLaunchKernelGGL(k_dref_scatter_src, px(SB), dim3(256), 0, st, Pp, Dp, D.dref_ext.p, J.c_f);
        LinParams P2;
        JointParams G2;
        source_groups(P2, G2, D.jrec_acc.p, D.dref_ext.p);
        hipLaunchKernelGGL((k_dense_joint<1, DTW, DTH, DNT, false, true, false>), dim3(nblk, SB), dim3(DNT), 0, st, P2, G2);
        hipLaunchKernelGGL(k_dref_export_grho_src, px(SB), dim3(256), 0, st, (const float *)D.jrec_acc.p, (int)JointLayout<1>::JREC, (const int *)D.dref_norms.p, ex->d_g_rho_src, (int)hw);
        return TCSFM_OK;
    }
    int export_once() {            // one linearisation, exported
        linearise(0);
        Si.mode = 2; Si.it = 0;
        launch_solve(h, Si, SB, 6);
        Sj.it = 0; Sj.mode = 0; Sj.export_out = D.dref_export.p;
        hipLaunchKernelGGL((k_solve_joint<NS>), dim3(B), dim3(JSOLVE_NT), 0, st, Sj);
        hipLaunchKernelGGL(k_dref_export_grho, px(B), dim3(256), 0, st, (const float *)D.jrec.p, (int)JL::JREC, (const double *)D.dref_export.p, 2 + 6 * JMAXS, ex->d_g_rho, (int)hw);
        if (ex->d_g_rho_src)
            if (int rc = export_sources()) return rc;
        HIPCHK(h, hipGetLastError());
        constexpr int kLin6 = 6 * 6 + 6 + 4;          // k_solve<6> mode 2: H [36], g [6], cost, cost_photo, cost_dc, n_mask
        std::vector<double> lin((size_t)SB * kLin6), jx((size_t)B * (2 + 6 * JMAXS));
        int norms[4];
        HIPCHK(h, hipMemcpyAsync(lin.data(), Si.lin_out, lin.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(jx.data(), D.dref_export.p, jx.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(norms, D.dref_norms.p, sizeof(norms), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        double fwd = 0, inv_p = 0, inv_d = 0;
        for (int b = 0; b < B; b++) {
            fwd += jx[(size_t)b * (2 + 6 * JMAXS)];
            for (int s_ = 0; s_ < S; s_++)
                for (int j = 0; j < 6; j++) ex->g_pose[(size_t)(s_ * B + b) * 6 + j] = jx[(size_t)b * (2 + 6 * JMAXS) + 2 + 6 * s_ + j];
        }
        for (int m = 0; m < SB; m++) {
            const double *q = &lin[(size_t)m * kLin6];
            for (int j = 0; j < 6; j++) ex->g_pose[(size_t)(SB + m) * 6 + j] = q[36 + j];
            inv_p += q[36 + 6 + 1]; inv_d += q[36 + 6 + 2];
        }
        double pc_total = 0.0;
        if (o->w_pose_consist > 0.f) {       // l_pose_consist of the exported linearisation: a closed form of the input poses (se3_math.h)
            std::vector<float> ph((size_t)N * 6);
            HIPCHK(h, hipMemcpy(ph.data(), c.pose_in, ph.size() * sizeof(float), hipMemcpyDeviceToHost));
            pc_total = pose_consist_linearised(ph.data(), SB, (double)o->w_pose_consist, (double)o->irls_eps, ex->g_pose);
        }
        ex->scal[0] = fwd + inv_p + inv_d + pc_total; ex->scal[1] = fwd; ex->scal[2] = inv_p; ex->scal[3] = inv_d;
        ex->scal[4] = norms[0]; ex->scal[5] = norms[1]; ex->scal[6] = jx[1]; ex->scal[7] = pc_total;
        return TCSFM_OK;
    }
    // The targets' record sums are split over several workgroups (JointSolveParams::nsplit: the last arriver solves) when a target has MANY records
    // -- the quarter-resolution unknown's tile + cell-group records.  Measured (scripts/dense_ref_timing.py, TCSFM_JOINT_SPLIT=1 switches it off):
    // 600-960 records: -2 ... -8 % per call; 150-480 records: the ticket costs what the faster fetch buys (+0 ... +2 %): not split -- except the S >= 2
    // targets' 480 records of 97+ floats, which two workgroups sum in one batch of loads each (third session: -0.8 % per B=1 KITTI window, -2.8 % at
    // minibatch 6; with one source the 32-float records are one batch already and splitting costs 2-4 %: profiles/r05_joint_split_sweep.txt)
    // (after the S = 1 solve took 32 record subsets its 600-900 quarter-resolution records are best summed by ONE workgroup -- 185 -> 175 us per 240x320
    // call -- and the S >= 2 targets' by four: profiles/r05_joint_split_sweep.txt)
    void params_solve() {
        auto split_of = [](int recs, int ns) { return ns == 1 ? 1 : (recs >= 512 ? 4 : (recs >= 400 ? 2 : 1)); };
        static const int split_env = getenv("TCSFM_JOINT_SPLIT") ? atoi(getenv("TCSFM_JOINT_SPLIT")) : -1;       // (A/B hook: 1 = off)
        Sj.nsplit = split_env > 0 ? std::min(split_env, kJointSplitMax) : split_of(Sj.nblk, NS); Sj.jpart = D.jpart.p; Sj.jtick = D.jtick.p;
        if (free_src) {
            Sj2.nsplit = split_env > 0 ? std::min(split_env, kJointSplitMax) : split_of(Sj2.nblk, 1);
            Sj2.jpart = D.jpart.p + pl.inv(DB_JPART); Sj2.jtick = D.jtick.p + pl.inv(DB_JTICK);
        }
        if (pc) {     // c = weight / (6 S B) of the CALL (merged calls never carry the term); forward pairs at [0, SB), inverse pairs at [SB, 2 SB) of a buffer
            const double w = (double)o->w_pose_consist / (6.0 * SB);
            Sj.w_pc = w; Sj.pc_eps = (double)o->irls_eps; Sj.pose_lin = h->pose_lin; Sj.pc_np = N; Sj.pc_self0 = 0; Sj.pc_part0 = SB;
            if (free_src) Sj2.w_pc = w, Sj2.pc_eps = (double)o->irls_eps, Sj2.pose_lin = h->pose_lin, Sj2.pc_np = N, Sj2.pc_self0 = SB, Sj2.pc_part0 = 0;
            Si.w_pc = w; Si.pc_eps = (double)o->irls_eps; Si.pose_lin = h->pose_lin; Si.pc_np = N; Si.pc_self0 = SB; Si.pc_part0 = 0;
        }
    }
    void solve(int it) {
        const bool last = it == o->n_iters - 1;
        Si.it = it; Si.mode = 0; Si.pose_out = last ? c.pose_out + (size_t)SB * 6 : nullptr; Si.log_scale_out = nullptr;
        Sj.it = it; Sj.mode = 0; Sj.pose_out = last ? c.pose_out : nullptr;
        ProfScope prof(h, 1);
        if (free_src) {   // the forward groups' 6S x 6S systems and the inverse groups' (pose + source map) 6 x 6 systems: one launch
            Sj2.it = it; Sj2.mode = 0; Sj2.pose_out = last ? c.pose_out + (size_t)SB * 6 : nullptr;
            Sj2.trace_decide = trace_decide_at(it, SB);
            if (pc) hipLaunchKernelGGL((k_solve_joint2<NS, true>), dim3(B * Sj.nsplit + SB * Sj2.nsplit), dim3(JSOLVE_NT), 0, st, Sj, Sj2);
            else hipLaunchKernelGGL((k_solve_joint2<NS>), dim3(B * Sj.nsplit + SB * Sj2.nsplit), dim3(JSOLVE_NT), 0, st, Sj, Sj2);
        } else {          // the target groups' and the inverse pairs' systems: independent, one launch
            if (pc) hipLaunchKernelGGL((k_solve_front<NS, true>), dim3(B * Sj.nsplit + SB), dim3(JSOLVE_NT), 0, st, Sj, Si);
            else hipLaunchKernelGGL((k_solve_front<NS>), dim3(B * Sj.nsplit + SB), dim3(JSOLVE_NT), 0, st, Sj, Si);
        }
    }
    void update(int it) {
        if (direct_out && it == o->n_iters - 1) {      // the last back-substitution also writes the caller's map (coalesced calls: every call's own)
            Uj.depth_out = c.depth_out; Q.depth_out = c.depth_out;
            coal_depth(Uj);
            coal_depth(Q);
        }
        const unsigned qsu_tiles = (unsigned)(((h->W + QSU_TW - 1) / QSU_TW) * ((h->H + QSU_TH - 1) / QSU_TH));
        if (qres) {       // cell step + x4 upsampling in one launch; the cell values ping-pong between the two halves of qres_rho
            const size_t half = pl.inv(DB_QRES_RHO);
            Q.rho_q = D.qres_rho.p + (it & 1) * half; Q.rho_q_next = D.qres_rho.p + ((it + 1) & 1) * half;
            if (free_src) {       // ... and the source maps' cells in the same launch (their upsampling refreshes the packs the forward pairs sample)
                const size_t half2 = pl.inv(DB_QRES_RHO_SRC);
                Q2.rho_q = D.qres_rho_src.p + (it & 1) * half2; Q2.rho_q_next = D.qres_rho_src.p + ((it + 1) & 1) * half2;
                hipLaunchKernelGGL((k_qres_step_up2<NS>), dim3(qsu_tiles, B + SB), dim3(QSU_TW * QSU_TH), 0, st, Q, Q2);
            } else hipLaunchKernelGGL((k_qres_step_up<NS>), dim3(qsu_tiles, B), dim3(QSU_TW * QSU_TH), 0, st, Q);
        } else if (free_src)      // the targets' maps and the source maps (the inverse pairs' own depth slots AND the depth channel of the packs the
                                  // forward pairs sample) in one launch
            hipLaunchKernelGGL((k_dense_joint_update2<NS>), px(B + SB), dim3(256), 0, st, Uj, Uj2);
        else hipLaunchKernelGGL((k_dense_joint_update<NS>), px(B), dim3(256), 0, st, Uj);
    }
    int finish() {
        HIPCHK(h, hipGetLastError());
        finish_no_iters(st);
        if (!direct_out)
            if (int rc = copy_out(st)) return rc;
        h->dref_dirty = o->n_iters == 0;      // (every linearisation's sums were consumed and cleared; with no iteration the pack's zeroed counters are all there is)
        return TCSFM_OK;
    }
    int run() {
        int rc;
        if (c.ct && (ex || o->free_source_depths != 0 || o->n_iters < 1 || c.stats || h->trace_bits))
            return fail(h, TCSFM_E_ARG, "internal: merged reference-loss calls are plain refinements with fixed source maps");
        if ((rc = refused()) || (rc = reserve()) || (rc = pack())) return rc;
        maps_diff = D.sel_maps.p; maps_valid = D.sel_maps.p + pl.inv(DB_SEL_MAPS);
        params_inverse();
        params_forward();
        params_qres();
        // (one stream: running the inverse pairs' linearise + solve on a second stream beside the forward group's, forked behind the scatter and
        // joined after the depth update, was measured SLOWER -- 261 vs 232 us per 240x320 window, 383 vs 361 at 192x640 S=2: the event hops cost
        // more than the ~18 us of overlap they buy)
        // the counters and the scatter sums are zero when a linearisation starts: zeroed here once per call, and by their consumers afterwards
        // (k_dense_joint clears every sum it reads, k_dense_joint_update the counters) -- two memset launches per iteration cost 10 us
        if ((rc = dref_clean(h))) return rc;
        h->dref_dirty = true;          // (until this call has issued its last consumer)
        Uj.norms_zero = D.dref_norms.p; Uj.norms_n = 2 * ngroups;
        if (free_src) params_free_sources();
        params_front();
        if (ex) return export_once();
        params_solve();
        for (int it = 0; it < o->n_iters; it++) {
            linearise(it);
            solve(it);
            update(it);
        }
        return finish();
    }
};

// ---- the PAIR form: every pair has its own copy of its target's depth map (tcsfm_refine_dense, and windows without the joint mode)
struct DensePair : DenseDriver {
    int n_sel;
    bool fuse;
    LinParams P;
    SolveParams Sv;
    DenseParams Dn;
    DenseUpdateParams U;
    DenseLmParams Ul;
    float *Dbuf[2], *Rbuf[2];

    explicit DensePair(const DenseCall &c_)
        : DenseDriver(c_, DENSE_PAIR, (c_.o->argmin ? DF_ARGMIN : 0) | (c_.o->solver == TCSFM_SOLVER_LM ? DF_LM : 0) | (c_.ct ? DF_MERGED : 0)) {
        n_sel = (S > 1 && o->argmin) ? SB : 0;
        // Gauss-Newton in the pair form: the back-substitution of iteration k is fused into the linearisation of iteration k+1 (depth
        // maps and per-pixel records ping-pong between two buffers); LM rolls maps back and the min over sources needs the current map
        // materialised before the linearisation, so those keep the separate update launch
        fuse = !lm && !n_sel && o->n_iters > 0;
    }
    int reserve() {
        if (int rc = reserve_pair_form(lm, n_sel != 0)) return rc;
        if (fuse) { DENSE_RESERVE(dense_rec2, DB_DENSE_REC2); DENSE_RESERVE(depth_alt, DB_DEPTH_ALT); }
        return TCSFM_OK;
    }
    int pack() {       // every pair gets its OWN copy of its target's depth; the pack also leaves the prior centre depth0
        InitParams I = init_params(h, &oo, N, c.pose_in, nullptr, c.K, 0);
        I.K_mod = S ? B : 0;
        return run_pack(h, &oo, N, c.tgt, c.src, c.dt, c.ds, &I, S ? B : 0, S, D.depth0.p, c.wo, c.ct);
    }
    void params() {
        P = lin_params(h, &oo, 6);
        P.tiles_x = pl.dtiles_x; P.tiles_y = pl.dtiles_y; P.ngrp = pl.dngrp;
        Sv = solve_params(h, &oo, 6, 0);
        P.direct = pl.dnblk <= 512;
        Sv.partials = P.direct ? h->blockrec : h->partials; Sv.ngrp = P.direct ? pl.dnblk : P.ngrp;
        Sv.stats = c.stats; Sv.delta_out = D.delta.p;
        coal_pose(Sv);
        Dn.dense_rec = D.dense_rec.p; Dn.depth0 = D.depth0.p; Dn.lambda_depth = o->lambda_depth; Dn.w_prior = o->prior_depth;
        Dn.prev_rec = nullptr; Dn.prev_delta = D.delta.p; Dn.depth_next = nullptr;
        Dn.rho_lo = 1.f / o->max_depth; Dn.rho_hi = 1.f / o->min_depth;
        memset(&U, 0, sizeof(U));
        U.dense_rec = D.dense_rec.p; U.delta = D.delta.p; U.depth = h->depth_work; U.depth_out = h->depth_work; U.hw = (int)hw;
        U.rho_lo = Dn.rho_lo; U.rho_hi = Dn.rho_hi;
        Dbuf[0] = h->depth_work; Dbuf[1] = D.depth_alt.p; Rbuf[0] = D.dense_rec.p; Rbuf[1] = D.dense_rec2.p;
        // min over the sources (window form): selection masks of the forward pairs from their residual maps at the current poses
        // AND current depth copies, rebuilt before every linearisation (same two launches as in the pose mode)
        if (n_sel) { P.ext_diff = D.sel_maps.p; P.ext_valid = D.sel_maps.p + pl.inv(DB_SEL_MAPS); P.n_ext = n_sel; P.ext_B = B; P.ext_S = S; }
        Ul.rec_try = D.dense_rec.p; Ul.rec_acc = D.dense_rec_acc.p; Ul.depth_acc = D.depth_acc.p; Ul.depth = h->depth_work; Ul.delta = D.delta.p;
        Ul.accept = D.lm_accept.p; Ul.hw = (int)hw; Ul.rho_lo = U.rho_lo; Ul.rho_hi = U.rho_hi;
        Sv.accept_out = lm ? D.lm_accept.p : nullptr;
    }
    void linearise(int lin) {
        trace_at(h, lin, N, P, Sv);
        if (fuse) {   // reads depth_{it-1} + the records / step of iteration it-1, leaves depth_it and the records of iteration it
            P.depth_t = Dbuf[lin & 1]; Dn.depth_next = Dbuf[(lin + 1) & 1];
            Dn.dense_rec = Rbuf[lin & 1]; Dn.prev_rec = lin > 0 ? Rbuf[(lin - 1) & 1] : nullptr;
        }
        if (n_sel) select_pass(n_sel);
        take_stamp(h, P, (size_t)pl.dnblk * N);
        ProfScope prof(h, 0);
        const dim3 grid(pl.dnblk, N), block(kDenseNT);
        if (P.trace != nullptr) hipLaunchKernelGGL((k_dense_linearize<kDenseTileW, kDenseTileH, kDenseNT, true>), grid, block, 0, h->stream, P, Dn);
        else hipLaunchKernelGGL((k_dense_linearize<kDenseTileW, kDenseTileH, kDenseNT>), grid, block, 0, h->stream, P, Dn);
    }
    void solve(int it, int mode, bool writes_pose) {
        Sv.it = it; Sv.mode = mode;
        Sv.pose_out = writes_pose ? c.pose_out : nullptr; Sv.log_scale_out = nullptr;
        launch_solve(h, Sv, N, 6);
    }
    void update() {
        if (lm) hipLaunchKernelGGL(k_dense_update_lm, px(N), dim3(256), 0, h->stream, Ul);
        else if (!fuse) hipLaunchKernelGGL(k_dense_update, px(N), dim3(256), 0, h->stream, U);
    }
    int run() {
        int rc;
        if ((rc = refused()) || (rc = reserve()) || (rc = pack())) return rc;
        params();
        if ((rc = trace_check(h, o, N))) return rc;
        const int nit = o->n_iters;
        for (int it = 0; it < nit; it++) {
            linearise(it);
            solve(it, 0, !lm && it == nit - 1);
            update();
        }
        if (fuse) {   // the last back-substitution writes the caller's depth map directly
            U.dense_rec = Rbuf[(nit - 1) & 1]; U.depth = Dbuf[nit & 1]; U.depth_out = c.depth_out;
            coal_depth(U);
            if (c.ct) U.c_S = c.ct->cS;
            hipLaunchKernelGGL(k_dense_update, px(N), dim3(256), 0, h->stream, U);
        }
        if (lm && nit > 0) {   // evaluate the last trial once more; keep it only if it lowered the cost (pose and depth map)
            linearise(nit);
            solve(nit, 1, true);
            hipLaunchKernelGGL(k_dense_final_lm, px(N), dim3(256), 0, h->stream, (const int *)D.lm_accept.p, (const float *)D.depth_acc.p, h->depth_work, (int)hw);
        }
        HIPCHK(h, hipGetLastError());
        finish_no_iters(h->stream);
        return fuse ? TCSFM_OK : copy_out(h->stream);
    }
};

// the driver of a call: the reference's loss at S = 1 .. JMAXS, the library's joint mode at S = 2 .. JMAXS_OWN, the pair form otherwise
int dense_ref_run(const DenseCall &c) {
    switch (c.S) {
    case 1: return DenseRef<1>(c).run();
    case 2: return DenseRef<2>(c).run();
    case 3: return DenseRef<3>(c).run();
    default: return DenseRef<4>(c).run();
    }
}
int dense_joint_run(const DenseCall &c) { return c.S == 2 ? DenseJoint<2>(c).run() : DenseJoint<3>(c).run(); }
int dense_pair_run(const DenseCall &c) { return DensePair(c).run(); }
#undef DENSE_RESERVE

}  // namespace

static int drain_queued(tcsfm_ctx *h);      // (call_host.h)

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
