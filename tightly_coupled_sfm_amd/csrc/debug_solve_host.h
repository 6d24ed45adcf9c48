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
