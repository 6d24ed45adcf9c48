// Host side of the solve test hooks (include/tcsfm.h: tcsfm_debug_solve, tcsfm_debug_solve_joint): ONE launch of a production solve kernel on
// host arrays the caller gives.  Here: the device copies both entries work on (DebugBufs), the argument checks of the joint entry (plain C++,
// no HIP: debug_joint_refusal) and the joint entry itself.  Part of tcsfm_api.hip, the library's only translation unit: included after
// context.h (fail, HIPCHK, DeviceGuard, pending_error; DevBuf and the guard-band helpers of device_owned.h) and drain_queued.  Production launches and kernels are not touched: the
// entry instantiates k_solve_joint<NS>, k_solve_front<NS, PC> and k_solve_joint2<NS, PC> at NS = 1 .. JMAXS, as dense_host.h does.
#pragma once

namespace {

// the device copies of a debug entry: allocations of the entry's own (guarded like every other), freed when it returns
struct DebugBufs {
    std::vector<DevBuf<char>> bufs;
    std::vector<void *> dev;      // their pointers, for tcguard::damaged_among
    struct Back { void *host; void *dev; size_t bytes; };
    std::vector<Back> back;
    // host == nullptr: nullptr.  Otherwise a device copy of `bytes` bytes; out: copied back after the launch
    hipError_t up(const void *host, size_t bytes, bool out, void **res) {
        *res = nullptr;
        if (!host || bytes == 0) return hipSuccess;
        bufs.emplace_back();
        hipError_t e = DEV_RESERVE(bufs.back(), bytes);
        if (e != hipSuccess) return e;
        void *d = bufs.back().p;
        dev.push_back(d);
        e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        if (out) back.push_back({const_cast<void *>(host), d, bytes});
        *res = d;
        return hipSuccess;
    }
};

inline int debug_joint_nacc(int ns) {
    return ns == 1 ? JointLayout<1>::NACC : (ns == 2 ? JointLayout<2>::NACC : (ns == 3 ? JointLayout<3>::NACC : JointLayout<4>::NACC));
}

// one group's checks: nullptr when the launch may index everything it will, else the message of the first check that fails.
// ns: the group's sources per target; pc: the variant has the pose-consistency code compiled in
inline const char *debug_joint_group_refusal(const tcsfm_debug_joint_group &g, int ns, int n_alloc, bool pc, int pc_np) {
    if (g.B < 1 || g.B > 4096 || g.b_alloc < g.B || g.b_alloc > 8192) return "need 1 <= B <= b_alloc";
    if (g.nblk < 1 || g.nblk > (1 << 20)) return "nblk must be at least 1";
    if (g.nsplit < 1 || g.nsplit > kJointSplitMax) return "nsplit out of range (1 .. 8)";
    if (!g.records || !g.js) return "records and js are required";
    if (g.n0 < 0 || (long long)g.n0 + (long long)ns * g.B > n_alloc) return "a pair index is outside the per-pair arrays (n0 + NS B > n_alloc)";
    if (g.nsplit > 1) {
        if (!g.jpart || !g.jtick) return "nsplit > 1 needs jpart and jtick";
        for (int b = 0; b < g.B; b++)
            if (g.jtick[b] != 0) return "a non-zero jtick (the tickets are zero between launches)";
    }
    if (g.norms) {
        if (g.norm_n < 1 || g.norm_B < 0) return "bad norms geometry";
        if ((g.norm_B > 0 ? (g.B - 1) / g.norm_B : 0) >= g.norm_n) return "norms is shorter than a target's group index needs";
    }
    if (pc) {
        if (g.pc_self0 < 0 || g.pc_part0 < 0) return "negative pose_lin geometry";
        if ((long long)g.pc_self0 + (long long)ns * g.B > pc_np) return "a pair's own slot is outside pose_lin";
        if ((long long)g.pc_part0 + (long long)ns * g.B > pc_np) return "a partner index is outside pose_lin";
    }
    return nullptr;
}

inline const char *debug_joint_refusal(const tcsfm_opts *o, const tcsfm_debug_solve_joint_args *a) {
    if (!o || !a) return "NULL argument";
    if (a->variant < 0 || a->variant > 4) return "variant must be 0 .. 4";
    if (a->NS < 1 || a->NS > JMAXS) return "NS must be 1 .. 4";
    if (a->mode < 0 || a->mode > 1) return "mode must be 0 or 1";
    if (o->solver != TCSFM_SOLVER_GN && o->solver != TCSFM_SOLVER_LM) return "unknown solver";
    if (a->mode == 1 && o->solver == TCSFM_SOLVER_GN) return "mode 1 is the final LM check: the solver must be LM";
    if (o->n_iters < 0 || o->n_iters > 1024 || a->it < 0 || a->it > o->n_iters) return "need 0 <= it <= n_iters";
    if (!a->state || !a->pconst) return "state and pconst are required";
    if (a->n_alloc < 1 || a->n_alloc > 32768) return "n_alloc must be at least 1";
    const bool two = a->variant >= 3, pc = a->variant == 2 || a->variant == 4;
    const bool pc_asked = a->w_pc > 0.0 || a->w_pc != a->w_pc;
    if (!pc && pc_asked) return "variants 0, 1 and 3 have no pose-consistency term";
    if (pc && (!a->pose_lin || a->pc_np < 1 || a->pc_np > 65536)) return "variants 2 and 4 read and write pose_lin: pose_lin and pc_np are required";
    if (const char *m = debug_joint_group_refusal(a->a, a->NS, a->n_alloc, pc, a->pc_np)) return m;
    if (two) {
        if (const char *m = debug_joint_group_refusal(a->b, 1, a->n_alloc, pc, a->pc_np)) return m;
        const long long a0 = a->a.n0, a1 = a0 + (long long)a->NS * a->a.B, b0 = a->b.n0, b1 = b0 + a->b.B;
        if (a0 < b1 && b0 < a1) return "the two groups' pairs overlap";
        if (pc) {
            const long long sa0 = a->a.pc_self0, sa1 = sa0 + (long long)a->NS * a->a.B, sb0 = a->b.pc_self0, sb1 = sb0 + a->b.B;
            if (sa0 < sb1 && sb0 < sa1) return "the two groups' own pose_lin slots overlap";
        }
    }
    if (a->c_ncall < 0 || a->c_ncall > TC_MAX_COAL) return "c_ncall out of range";
    if (a->c_ncall > 0) {
        if (two) return "coalesced outputs: variants 0 to 2 only (merged calls never carry free source maps)";
        if (a->c_B < 1 || a->c_S < 1 || a->c_B > 4096 || a->c_S > 4096) return "bad coalesce geometry";
        for (int n = 0; n < a->NS * a->a.B; n++) {
            const CoalIdx ci = coal_index(a->c_ncall, a->c_B, a->c_S, n);
            if (ci.call < 0 || ci.call >= a->c_ncall || !a->c_pose_out[ci.call] || ci.li < 0 || ci.li >= a->c_len[ci.call])
                return "a coalesced pair's output slot is outside the given per-call arrays";
        }
    }
    return nullptr;
}

template <int NS>
void debug_joint_launch(int variant, hipStream_t st, const JointSolveParams &Pa, const JointSolveParams &Pb) {
    const int Ga = Pa.nsplit > 1 ? Pa.nsplit : 1, Gb = Pb.nsplit > 1 ? Pb.nsplit : 1;
    if (variant == 0) hipLaunchKernelGGL((k_solve_joint<NS>), dim3(Pa.B * Ga), dim3(JSOLVE_NT), 0, st, Pa);
    else if (variant <= 2) {
        SolveParams Pi;
        memset(&Pi, 0, sizeof(Pi));       // grid = B G: no workgroup takes the pair role
        if (variant == 2) hipLaunchKernelGGL((k_solve_front<NS, true>), dim3(Pa.B * Ga), dim3(JSOLVE_NT), 0, st, Pa, Pi);
        else hipLaunchKernelGGL((k_solve_front<NS>), dim3(Pa.B * Ga), dim3(JSOLVE_NT), 0, st, Pa, Pi);
    } else if (variant == 4) hipLaunchKernelGGL((k_solve_joint2<NS, true>), dim3(Pa.B * Ga + Pb.B * Gb), dim3(JSOLVE_NT), 0, st, Pa, Pb);
    else hipLaunchKernelGGL((k_solve_joint2<NS>), dim3(Pa.B * Ga + Pb.B * Gb), dim3(JSOLVE_NT), 0, st, Pa, Pb);
}

int debug_solve_joint_run(tcsfm_ctx *h, const tcsfm_opts *o, tcsfm_debug_solve_joint_args *a) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (const char *why = debug_joint_refusal(o, a)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_debug_solve_joint: ") + why).c_str());
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    DebugBufs B;
    const size_t na = (size_t)a->n_alloc;
    const bool two = a->variant >= 3, pc = a->variant == 2 || a->variant == 4;
    void *p = nullptr;
#define DJ_UP(dst, type, host, bytes, out) HIPCHK(h, B.up((host), (bytes), (out), &p)); dst = (type)p
    PairState *st = nullptr;
    PairConst *pcn = nullptr;
    float *stats = nullptr, *pose_out = nullptr;
    int *trace_decide = nullptr;
    double *pose_lin = nullptr;
    DJ_UP(st, PairState *, a->state, na * sizeof(PairState), true);
    DJ_UP(pcn, PairConst *, a->pconst, na * sizeof(PairConst), true);
    DJ_UP(stats, float *, a->stats, na * (o->n_iters + 1) * TCSFM_NSTAT * sizeof(float), true);
    DJ_UP(pose_out, float *, a->pose_out, na * 6 * sizeof(float), true);
    DJ_UP(trace_decide, int *, a->trace_decide, na * sizeof(int), true);
    DJ_UP(pose_lin, double *, a->pose_lin, (size_t)2 * (a->pc_np > 0 ? a->pc_np : 0) * 12 * sizeof(double), true);
    JointSolveParams P[2];
    memset(P, 0, sizeof(P));
    for (int k = 0; k < (two ? 2 : 1); k++) {
        const tcsfm_debug_joint_group &g = k ? a->b : a->a;
        JointSolveParams &S = P[k];
        const size_t nb = (size_t)g.b_alloc, nacc = (size_t)debug_joint_nacc(k ? 1 : a->NS);
        DJ_UP(S.jblockrec, const float *, g.records, nb * g.nblk * nacc * sizeof(float), false);
        DJ_UP(S.js, JointState *, g.js, nb * sizeof(JointState), true);
        DJ_UP(S.norms, const int *, g.norms, (size_t)g.norm_n * 2 * sizeof(int), false);
        DJ_UP(S.delta_out, double *, g.delta_out, nb * 6 * JMAXS * sizeof(double), true);
        DJ_UP(S.accept_out, int *, g.accept_out, nb * sizeof(int), true);
        DJ_UP(S.export_out, double *, g.export_out, nb * (2 + 6 * JMAXS) * sizeof(double), true);
        DJ_UP(S.jpart, double *, g.jpart, nb * g.nsplit * nacc * sizeof(double), true);
        DJ_UP(S.jtick, int *, g.jtick, nb * sizeof(int), true);
        S.st = st + g.n0; S.pc = pcn + g.n0;
        S.stats = stats ? stats + (size_t)g.n0 * (o->n_iters + 1) * TCSFM_NSTAT : nullptr;
        S.pose_out = pose_out ? pose_out + (size_t)g.n0 * 6 : nullptr;
        S.trace_decide = trace_decide ? trace_decide + g.n0 : nullptr;
        S.nblk = g.nblk; S.B = g.B; S.it = a->it; S.n_iters = o->n_iters; S.solver = o->solver; S.mode = a->mode;
        S.lambda_up = o->lambda_up; S.lambda_down = o->lambda_down; S.lambda_min = o->lambda_min; S.lambda0 = o->lambda0;
        S.norm_B = g.norm_B; S.c_f = g.c_f; S.nsplit = g.nsplit;
        if (pc) { S.w_pc = a->w_pc; S.pc_eps = a->pc_eps; S.pose_lin = pose_lin; S.pc_np = a->pc_np; S.pc_self0 = g.pc_self0; S.pc_part0 = g.pc_part0; }
    }
    if (a->c_ncall > 0) {
        P[0].c_ncall = a->c_ncall; P[0].c_B = a->c_B; P[0].c_S = a->c_S;
        for (int i = 0; i < a->c_ncall; i++) { DJ_UP(P[0].c_pose_out[i], float *, a->c_pose_out[i], (size_t)a->c_len[i] * 6 * sizeof(float), true); }
    }
#undef DJ_UP
    switch (a->NS) {
    case 1: debug_joint_launch<1>(a->variant, h->stream, P[0], P[1]); break;
    case 2: debug_joint_launch<2>(a->variant, h->stream, P[0], P[1]); break;
    case 3: debug_joint_launch<3>(a->variant, h->stream, P[0], P[1]); break;
    default: debug_joint_launch<4>(a->variant, h->stream, P[0], P[1]); break;
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (const auto &b : B.back) HIPCHK(h, hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    // the entry's allocations are freed when it returns, so tcsfm_debug_check_guards never sees them: their bands are checked here
    const int hit = tcguard::damaged_among(B.dev);
    if (hit < 0) return fail(h, TCSFM_E_HIP, "tcsfm_debug_solve_joint: could not read the guard bands back");
    if (hit > 0) return fail(h, TCSFM_E_HIP, "tcsfm_debug_solve_joint: the launch wrote outside the entry's device arrays (guard bands damaged, details on stderr)");
    return TCSFM_OK;
}

}  // namespace

int tcsfm_debug_solve_layout(int *sizeof_pair_state, int *sizeof_pair_const) {
    if (sizeof_pair_state) *sizeof_pair_state = (int)sizeof(PairState);
    if (sizeof_pair_const) *sizeof_pair_const = (int)sizeof(PairConst);
    return TCSFM_OK;
}

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
