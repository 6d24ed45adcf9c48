// The scratch plan of a dense call (dense_host.h), host only: how large every buffer of the dense modes is, which tile grids a call
// launches on, and which part of which buffer each of its launches works on.  Integer arithmetic, no HIP, no environment:
// tests/asan/dense_plan_host.cpp builds it alone and walks a grid of handles and calls.
//
// The contract.  A CAPACITY (dense_caps) depends on the handle -- H, W, max_pairs -- and on nothing else: a captured call graph
// (tcsfm_set_graph_replay) bakes the scratch pointers in, so a buffer is allocated once, at that capacity, and is never re-sized while
// the handle lives.  A VIEW (dense_plan) is what one call takes of a buffer, as offset and extent in ELEMENTS of the buffer's type; every
// view of an accepted plan lies inside its buffer's capacity, and the views a call writes from launches that may run side by side are
// disjoint.  Where the capacities cannot hold a call the plan carries a refusal and the call launches nothing.
#pragma once
#include <stddef.h>
#include "layout.h"

namespace tc {

// Every buffer a dense call takes a view of: the handle's create-time buffers first, then the dense scratch (DenseScratch, dense_host.h).
enum DenseBuf {
    DB_TGTPACK, DB_SRCPACK, DB_DEPTH_WORK, DB_PCONST, DB_STATE, DB_BLOCKREC, DB_TICKETS, DB_PARTIALS, DB_LIN_OUT,      // create-time
    DB_STATS,            // the caller's statistics: in blocks of one pair's (n_iters + 1) x TCSFM_NSTAT floats; capacity N blocks, the call's own
    DB_SEL_MAPS,         // dense window modes: the forward pairs' diff | valid maps, [2][max_pairs][H*W]
    DB_DENSE_REC, DB_DEPTH0, DB_DELTA,                 // per-pixel records, prior centres and steps of the pair-form dense kernels
    DB_DENSE_REC2, DB_DEPTH_ALT,                       // ... second record / depth buffers of the fused back-substitution (ping-pong)
    DB_DENSE_REC_ACC, DB_DEPTH_ACC, DB_LM_ACCEPT,      // dense LM: accepted per-pixel records / depth maps, accept flags
    // joint dense modes (one depth map per target shared by its S forward pairs): per-pixel records, workgroup records, per-target state
    DB_JREC, DB_JREC_ACC, DB_JDEPTH_ACC, DB_JBLOCKREC, DB_JSTATE, DB_JDELTA,
    DB_JPART, DB_JTICK,  // split record sums of the joint solve (JointSolveParams::nsplit): [2][8][accumulator rows] fp64, [2][targets] tickets
    // dense mode on the reference's loss (dense_ref_kernel.h): mask counts, fixed-point scatter sums, linearisation export, l_smooth means
    DB_DREF_NORMS, DB_DREF_EXT, DB_DREF_EXPORT, DB_DREF_SMOOTH,
    DB_QRES_RHO, DB_QRES_REC,      // TCSFM_DEPTH_QUARTER: [2][targets][H/4 * W/4] cell unknowns (ping-pong), [targets][cells][JREC] cell records
    // free source depth maps (opts.free_source_depths): the inverse pairs as groups of one source
    DB_JREC_SRC, DB_JSTATE_SRC, DB_JDELTA_SRC, DB_DREF_EXT_SRC, DB_QRES_RHO_SRC, DB_QRES_REC_SRC,
    DB_COUNT
};

struct DenseCaps {
    size_t cap[DB_COUNT];          // elements (DB_STATS: 0, the array is the caller's)
    int nblk, ngrp;                // the pose path's tile grid (32 x TC_TILE_H) and its reduction groups
    int nblk_alloc, ngrp_alloc, ngrp_pad;      // records / groups per pair the create-time buffers hold
    int jrec_alloc;                // workgroup records per target jblockrec holds: joint_records_per_target
};

inline int tiles_of(int H, int W, int tw, int th) { return ((W + tw - 1) / tw) * ((H + th - 1) / th); }
inline int joint_tiles(int H, int W) { return tiles_of(H, W, kJointTileW, kJointTileH); }
// k_qres_*'s cell groups: their records follow the joint kernel's tiles' in a target's row of jblockrec
inline int qres_groups(int H, int W) { return ((H / 4) * (W / 4) + QRES_CELLS_PER_WG - 1) / QRES_CELLS_PER_WG; }
// workgroup records of one target, the most any call can write: the joint tiles, then the quarter-resolution unknown's cell groups.  (Not the
// pose path's 16 x 16 tile count: that is the smaller one whenever ceil(W / 16) is odd and ceil(H / 8) even -- 16 x 48, 28 x 48, 192 x 624.)
inline int joint_records_per_target(int H, int W) { return joint_tiles(H, W) + qres_groups(H, W); }

static_assert(JMAXS == 4, "joint_max_over_S lists the layouts S = 1 .. 4");
constexpr size_t joint_jrec(int S) { return S == 1 ? JointLayout<1>::JREC : S == 2 ? JointLayout<2>::JREC : S == 3 ? JointLayout<3>::JREC : JointLayout<4>::JREC; }
constexpr size_t joint_nacc(int S) { return S == 1 ? JointLayout<1>::NACC : S == 2 ? JointLayout<2>::NACC : S == 3 ? JointLayout<3>::NACC : JointLayout<4>::NACC; }
// what 0: floats per pixel of jrec / jrec_acc / qres_rec; 1: accumulator rows of one half of jpart (and the forward groups' share of a
// jblockrec row); 2: one jblockrec row = forward groups + the free-source mode's inverse groups
constexpr size_t joint_max_over_S(size_t n, int what) {
    size_t m = 0;
    for (int S = 1; S <= JMAXS; S++) {
        const size_t t = S == 1 ? (n + 1) / 2 : n / (2 * S);          // targets of a call with S sources (2 B S <= max_pairs)
        const size_t v = t * (what == 0 ? joint_jrec(S) : what == 1 ? joint_nacc(S) : joint_nacc(S) + S * joint_nacc(1));
        m = v > m ? v : m;
    }
    return m;
}
inline size_t joint_rec_floats(size_t n) { return joint_max_over_S(n, 0); }
inline size_t joint_acc_floats(size_t n) { return joint_max_over_S(n, 1); }
inline size_t joint_blockrec_floats(size_t n) { return joint_max_over_S(n, 2); }

// Capacities of a handle.  The per-PIXEL records (jrec, jrec_acc, the quarter-resolution cell records) and the per-target record arrays
// (workgroup records, split partial sums) are sized for the largest layout any call can need: a call of S sources has at most
// max_pairs / (2 S) targets of JREC(S) floats per pixel and NACC(S) per record, so the capacity is the maximum over S = 1 .. JMAXS of
// (targets at S) x JREC(S) -- 8 x max_pairs / 2 at S = 1 and S = 2, 28 x max_pairs / 8 at S = 4 -- not JREC(JMAXS) x the most targets (the
// per-pixel records of a handle are smaller than the S <= 3 layouts had them: 20 x max_pairs / 4).  The workgroup records also hold,
// behind the forward groups', the free-source mode's S B inverse groups of one source.  The per-TARGET arrays (state, step, accepted
// depth) are sized for the most targets any call can have: (max_pairs + 1) / 2, reached at S = 1 (they were once sized for S >= 2 and the
// S = 1 reference-loss mode indexed past them).
inline DenseCaps dense_caps(int H, int W, int max_pairs) {
    DenseCaps c;
    const size_t hw = (size_t)H * W, n = (size_t)max_pairs;
    const size_t nt = (n + 1) / 2, ng = n / 2;                     // targets at most (S = 1); inverse groups of one source at most
    const size_t nq = (size_t)(H / 4) * (W / 4);
    const size_t nrec = joint_rec_floats(n), nacc = joint_acc_floats(n);
    c.nblk = tiles_of(H, W, TILE_W, TILE_H);
    c.ngrp = (c.nblk + RG - 1) / RG;
    c.nblk_alloc = ((W + 15) / 16) * ((H + 15) / 16);   // the finest tiling of the pose path and the pair-form dense kernels (16 x 16); the
                                                         // joint kernels' 32 x 8 tiles size their own scratch (joint_records_per_target)
    if (c.nblk_alloc < c.nblk) c.nblk_alloc = c.nblk;
    c.ngrp_alloc = (c.nblk_alloc + RG - 1) / RG;
    c.ngrp_pad = (c.ngrp_alloc + 63) / 64 * 64;
    c.jrec_alloc = joint_records_per_target(H, W);
    size_t *k = c.cap;
    k[DB_TGTPACK] = n * hw; k[DB_SRCPACK] = n * (size_t)(H + 2) * (W + 2); k[DB_DEPTH_WORK] = n * hw;      // (the source pack is zero-bordered)
    k[DB_PCONST] = n; k[DB_STATE] = n; k[DB_LIN_OUT] = n * kLinOut;
    k[DB_BLOCKREC] = n * c.nblk_alloc * kMaxAcc; k[DB_TICKETS] = n * c.ngrp_alloc; k[DB_PARTIALS] = n * c.ngrp_pad * kMaxAcc;
    k[DB_STATS] = 0;
    k[DB_SEL_MAPS] = 2 * n * hw;
    k[DB_DENSE_REC] = n * hw * 8; k[DB_DEPTH0] = n * hw; k[DB_DELTA] = n * 8;
    k[DB_DENSE_REC2] = n * hw * 8; k[DB_DEPTH_ALT] = n * hw;
    k[DB_DENSE_REC_ACC] = n * hw * 8; k[DB_DEPTH_ACC] = n * hw; k[DB_LM_ACCEPT] = n;
    k[DB_JREC] = hw * nrec; k[DB_JREC_ACC] = hw * nrec; k[DB_JDEPTH_ACC] = nt * hw;
    k[DB_JBLOCKREC] = (size_t)c.jrec_alloc * joint_blockrec_floats(n);      // (tile records + the quarter-resolution mode's cell-group records)
    k[DB_JSTATE] = nt; k[DB_JDELTA] = nt * 6 * JMAXS;
    k[DB_JPART] = 2 * kJointSplitMax * nacc;                       // (forward groups, then the free-source mode's inverse groups)
    k[DB_JTICK] = 2 * nt;
    k[DB_DREF_NORMS] = 2 * TC_MAX_COAL;                            // (one (K_f, K_i) pair per normaliser group)
    k[DB_DREF_EXT] = nt * hw * 2;                                  // (targets <= max_pairs / 2; two sums per pixel)
    k[DB_DREF_EXPORT] = nt * (2 + 6 * JMAXS); k[DB_DREF_SMOOTH] = nt * 2;
    k[DB_QRES_RHO] = 2 * nt * nq;                                  // (two buffers: k_qres_step_up ping-pongs)
    k[DB_QRES_REC] = nq * nrec;
    k[DB_JREC_SRC] = ng * hw * JointLayout<1>::JREC; k[DB_JSTATE_SRC] = ng; k[DB_JDELTA_SRC] = ng * 6 * JMAXS; k[DB_DREF_EXT_SRC] = ng * hw * 2;
    k[DB_QRES_RHO_SRC] = 2 * ng * nq;                              // (two buffers: k_qres_step_up ping-pongs)
    k[DB_QRES_REC_SRC] = ng * nq * JointLayout<1>::JREC;
    return c;
}

enum DenseMode { DENSE_PAIR = 0, DENSE_JOINT = 1, DENSE_REF = 2 };      // the pair form, the library's joint mode, the reference's loss
enum DenseFlags {
    DF_ARGMIN = 1,       // min over the sources (selection maps)
    DF_LM = 2,           // Levenberg-Marquardt (not under the reference's loss)
    DF_QRES = 4,         // TCSFM_DEPTH_QUARTER
    DF_FREE_SRC = 8,     // opts.free_source_depths
    DF_EXPORT = 16,      // tcsfm_linearize_dense_window: one linearisation, exported
    DF_EXPORT_SRC = 32,  // ... with the gradient w.r.t. the source maps (tcsfm_linearize_dense_window_sources)
    DF_MERGED = 64       // B covers the targets of several queued calls
};

struct DenseView { size_t off = 0, len = 0; };      // elements; len = 0: the call takes no such view

// Every view of a call, with its extent: what tests/asan/dense_plan_host.cpp checks.  Of a buffer indexed by pair, a[] is the forward
// pairs' part and b[] the inverse pairs', S B pairs further on; of jblockrec, jpart and jtick a[] is the forward groups' part and b[] the
// free-source mode's inverse groups' (behind jrec2_off / in the second half); of sel_maps a[] is the diff half and b[] the valid half; of
// qres_rho and qres_rho_src a[] and b[] are the two ping-pong halves (iteration `it` reads half it & 1 and writes the other).  a[x] and
// b[x] may be written by launches that run side by side: they are disjoint.  c[] is what the export-with-sources path re-uses AFTER the
// solve has consumed the forward groups' records: the source groups' per-pixel records (jrec_acc), workgroup records (the front of
// jblockrec) and scatter sums (dref_ext).
struct DenseViews { DenseView a[DB_COUNT], b[DB_COUNT], c[DB_COUNT]; };

// What a driver needs of a call: the grids, the records per target and where every second view starts (a first view starts at 0).
struct DensePlan {
    const char *refusal = nullptr;
    int B = 0, S = 0, SB = 0, N = 0;                 // targets, sources, forward pairs, pairs
    int tiles_x = 0, tiles_y = 0, nblk = 0, ngrp = 0;          // pose grid, 32 x TC_TILE_H
    int dtiles_x = 0, dtiles_y = 0, dnblk = 0, dngrp = 0;      // pair-form dense grid, 32 x 16
    int jtiles_x = 0, jtiles_y = 0, jnblk = 0, jngrp = 0;      // joint grid, 32 x TC_JOINT_TILE_H
    int nq = 0, nqblk = 0;                           // quarter-resolution cells of a map; their cell groups (0 unless the call is one)
    int recs = 0;                                    // workgroup records per target: jnblk + nqblk
    size_t jrec2_off = 0;                            // = off[DB_JBLOCKREC] where the call has inverse groups
    size_t off[DB_COUNT] = {};                       // DenseViews::b[x].off
    size_t inv(DenseBuf x) const { return off[x]; }
};

// The plan of a call of B targets with S sources each (merged calls: all their targets; the pair form outside a window: S = 0 and B
// pairs) on a handle of H x W and max_pairs whose capacities are cp.  The caller has checked 2 B S <= max_pairs (B <= max_pairs) and the
// flags' admissibility.  views: also every view with its extent (the drivers pass none).
inline DensePlan dense_plan(const DenseCaps &cp, int mode, int H, int W, int max_pairs, int B, int S, unsigned flags, DenseViews *views = nullptr) {
    DensePlan p;
    const size_t hw = (size_t)H * W, hwb = (size_t)(H + 2) * (W + 2), n = (size_t)max_pairs, nt = (n + 1) / 2, ng = n / 2;
    const bool sel = (flags & DF_ARGMIN) && S > 1, lm = (flags & DF_LM) != 0, qres = (flags & DF_QRES) != 0, free_src = (flags & DF_FREE_SRC) != 0;
    p.B = B; p.S = S; p.SB = S ? S * B : B; p.N = S ? 2 * S * B : B;
    const size_t SB = (size_t)p.SB, N = (size_t)p.N;
    p.tiles_x = (W + TILE_W - 1) / TILE_W; p.tiles_y = (H + TILE_H - 1) / TILE_H; p.nblk = p.tiles_x * p.tiles_y; p.ngrp = (p.nblk + RG - 1) / RG;
    p.dtiles_x = (W + kDenseTileW - 1) / kDenseTileW; p.dtiles_y = (H + kDenseTileH - 1) / kDenseTileH; p.dnblk = p.dtiles_x * p.dtiles_y; p.dngrp = (p.dnblk + RG - 1) / RG;
    p.jtiles_x = (W + kJointTileW - 1) / kJointTileW; p.jtiles_y = (H + kJointTileH - 1) / kJointTileH; p.jnblk = p.jtiles_x * p.jtiles_y; p.jngrp = (p.jnblk + RG - 1) / RG;
    p.nq = (H / 4) * (W / 4); p.nqblk = qres ? qres_groups(H, W) : 0;
    p.recs = p.jnblk + p.nqblk;
    auto view = [&p, views](int which, DenseBuf x, size_t off, size_t len) {
        if (which == 1) p.off[x] = off;
        if (views) (which == 0 ? views->a : which == 1 ? views->b : views->c)[x] = {off, len};
    };
    // a[x] = rows [0, na) and b[x] = rows [na, na + nb) of `stride` elements
    auto rows = [&view](DenseBuf x, size_t na, size_t nb, size_t stride) { view(0, x, 0, na * stride); if (nb) view(1, x, na * stride, nb * stride); };
    if (mode == DENSE_PAIR) {
        if (p.dnblk > cp.nblk_alloc || p.dngrp > cp.ngrp_alloc) { p.refusal = "internal: dense tile grid exceeds scratch"; return p; }
        const size_t nacc6 = AccLayout<6>::NACC;
        rows(DB_TGTPACK, N, 0, hw); rows(DB_SRCPACK, N, 0, hwb); rows(DB_DEPTH_WORK, N, 0, hw); rows(DB_PCONST, N, 0, 1); rows(DB_STATE, N, 0, 1);
        rows(DB_BLOCKREC, N, 0, p.dnblk * nacc6); rows(DB_TICKETS, N, 0, p.dngrp); rows(DB_PARTIALS, N, 0, p.dngrp * nacc6); rows(DB_STATS, N, 0, 1);
        rows(DB_DENSE_REC, N, 0, hw * 8); rows(DB_DEPTH0, N, 0, hw); rows(DB_DELTA, N, 0, 8);
        if (lm) { rows(DB_DENSE_REC_ACC, N, 0, hw * 8); rows(DB_DEPTH_ACC, N, 0, hw); rows(DB_LM_ACCEPT, N, 0, 1); }
        if (!lm && !sel) { rows(DB_DENSE_REC2, N, 0, hw * 8); rows(DB_DEPTH_ALT, N, 0, hw); }      // the fused back-substitution's ping-pong
        if (sel) { view(0, DB_SEL_MAPS, 0, SB * hw); view(1, DB_SEL_MAPS, n * hw, SB * hw); }
        return p;
    }
    // capacity of the joint scratch for a call with B targets of S sources each (explicit: the sizes above are derived, not per call)
    const size_t jrec_f = joint_jrec(S), nacc_f = joint_nacc(S), nacc1 = joint_nacc(1), nacc6 = AccLayout<6>::NACC;
    auto joint_fits = [&]() {
        return (size_t)B <= nt && (size_t)B * jrec_f <= joint_rec_floats(n) && (size_t)B * nacc_f <= joint_acc_floats(n) && p.recs <= cp.jrec_alloc &&
               (size_t)B * p.recs * nacc_f <= cp.cap[DB_JBLOCKREC];
    };
    // both window modes: the packs, constants and states of the forward pairs, then of the inverse pairs
    rows(DB_TGTPACK, SB, SB, hw); rows(DB_SRCPACK, SB, SB, hwb); rows(DB_DEPTH_WORK, SB, SB, hw); rows(DB_PCONST, SB, SB, 1); rows(DB_STATE, SB, SB, 1);
    rows(DB_STATS, SB, SB, 1); rows(DB_DEPTH0, SB, SB, hw);
    rows(DB_JREC, B, 0, hw * jrec_f); rows(DB_JBLOCKREC, B, 0, p.recs * nacc_f); rows(DB_JSTATE, B, 0, 1); rows(DB_JDELTA, B, 0, 6 * JMAXS);
    if (mode == DENSE_JOINT) {
        if (p.dnblk > cp.nblk_alloc) { p.refusal = "internal: dense tile grid exceeds scratch"; return p; }
        if (!joint_fits()) { p.refusal = "internal: the joint dense scratch does not hold this many targets"; return p; }
        // the inverse pairs: the pair-form dense kernels on views offset by S B pairs
        rows(DB_BLOCKREC, SB, SB, p.dnblk * nacc6); rows(DB_DELTA, SB, SB, 8); rows(DB_DENSE_REC, SB, SB, hw * 8);
        if (lm) {
            rows(DB_DENSE_REC_ACC, SB, SB, hw * 8); rows(DB_DEPTH_ACC, SB, SB, hw);
            view(0, DB_LM_ACCEPT, 0, (size_t)B); view(1, DB_LM_ACCEPT, SB, SB);       // (the forward groups' flags are per target)
            rows(DB_JREC_ACC, B, 0, hw * jrec_f); rows(DB_JDEPTH_ACC, B, 0, hw);
        }
        if (sel) { view(0, DB_SEL_MAPS, 0, SB * hw); view(1, DB_SEL_MAPS, n * hw, SB * hw); }
        return p;
    }
    // ---- the reference's loss
    if (!joint_fits()) { p.refusal = "internal: the joint dense scratch does not hold this many targets"; return p; }
    // (the inverse groups' workgroup records follow the forward groups' in jblockrec: both joint launches of a linearisation run before the solve)
    p.jrec2_off = (size_t)B * p.recs * nacc_f;
    if (free_src && p.jrec2_off + SB * p.recs * nacc1 > cp.cap[DB_JBLOCKREC]) { p.refusal = "internal: the inverse groups' records exceed the scratch"; return p; }
    // the inverse pairs' systems: the pose kernels on views offset by S B pairs
    rows(DB_BLOCKREC, SB, SB, p.nblk * nacc6); rows(DB_TICKETS, SB, SB, p.ngrp); rows(DB_PARTIALS, SB, SB, p.ngrp * nacc6); rows(DB_LIN_OUT, SB, SB, kLinOut);
    view(0, DB_SEL_MAPS, 0, N * hw); view(1, DB_SEL_MAPS, n * hw, N * hw);
    rows(DB_DREF_NORMS, 2 * TC_MAX_COAL, 0, 1); rows(DB_DREF_EXT, B, 0, hw * 2); rows(DB_DREF_EXPORT, B, 0, 2 + 6 * JMAXS); rows(DB_DREF_SMOOTH, B, 0, 2);
    view(0, DB_JPART, 0, (size_t)kJointSplitMax * B * nacc_f); view(0, DB_JTICK, 0, (size_t)B);
    if (qres) {
        view(0, DB_QRES_RHO, 0, (size_t)B * p.nq); view(1, DB_QRES_RHO, nt * p.nq, (size_t)B * p.nq);
        rows(DB_QRES_REC, B, 0, p.nq * jrec_f);
    }
    if (free_src) {
        view(1, DB_JBLOCKREC, p.jrec2_off, SB * p.recs * nacc1);
        view(1, DB_JPART, kJointSplitMax * joint_acc_floats(n), kJointSplitMax * SB * nacc1); view(1, DB_JTICK, nt, SB);
        rows(DB_JREC_SRC, SB, 0, hw * joint_jrec(1)); rows(DB_JSTATE_SRC, SB, 0, 1); rows(DB_JDELTA_SRC, SB, 0, 6 * JMAXS); rows(DB_DREF_EXT_SRC, SB, 0, hw * 2);
        if (qres) {
            view(0, DB_QRES_RHO_SRC, 0, SB * p.nq); view(1, DB_QRES_RHO_SRC, ng * p.nq, SB * p.nq);
            rows(DB_QRES_REC_SRC, SB, 0, p.nq * joint_jrec(1));
        }
    }
    if (flags & DF_EXPORT_SRC) {
        view(2, DB_JREC_ACC, 0, SB * hw * joint_jrec(1)); view(2, DB_JBLOCKREC, 0, SB * p.jnblk * nacc1); view(2, DB_DREF_EXT, 0, SB * hw * 2);
    }
    return p;
}

inline DensePlan dense_plan(int mode, int H, int W, int max_pairs, int B, int S, unsigned flags, DenseViews *views = nullptr) {
    return dense_plan(dense_caps(H, W, max_pairs), mode, H, W, max_pairs, B, S, flags, views);
}

}  // namespace tc
