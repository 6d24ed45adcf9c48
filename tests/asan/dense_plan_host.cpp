// Stand-alone sanitizer program for the scratch plan of the dense modes (csrc/dense_plan.h) and the host closed form of the
// pose-consistency term (csrc/se3_math.h).  Its own main, no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I tightly_coupled_sfm_amd/csrc tests/asan/dense_plan_host.cpp -o dense_plan_host && ./dense_plan_host
//
// (the runtimes are linked statically: the program then runs as it is wherever the process's library list does not start with them)
// Every admissible call of a grid of handles is planned and checked: (a) every view of an accepted plan lies inside its buffer's
// capacity, (b) the views one call writes from launches that may run side by side are disjoint, (c) a capacity takes no call argument,
// (d) a plan is refused exactly where the three checks of the drivers this header replaced refuse -- restated below from their formulas,
// with the record sizes as literals, in the grid (where none refuses) and at probes outside the contract (where all three do) -- and (e) a table pins capacities and offsets of a few handles, worked out by hand.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <type_traits>
#include "dense_plan.h"
#include "se3_math.h"

using namespace tc;

// (c) the capacities are a function of the handle alone
static_assert(std::is_same<decltype(&dense_caps), DenseCaps (*)(int, int, int)>::value, "dense_caps(H, W, max_pairs)");

// ---- (d) the checks as the drivers made them.  Record sizes: JREC(S) = 8, 16, 20, 28 floats per pixel; NACC(S) = 32, 97, 198, 335.
static const size_t kJrec[5] = {0, 8, 16, 20, 28}, kNacc[5] = {0, 32, 97, 198, 335};
static size_t old_max_over_S(size_t n, int what) {
    size_t m = 0;
    for (int S = 1; S <= 4; S++) {
        const size_t t = S == 1 ? (n + 1) / 2 : n / (2 * S);
        const size_t v = t * (what == 0 ? kJrec[S] : what == 1 ? kNacc[S] : kNacc[S] + S * kNacc[1]);
        m = v > m ? v : m;
    }
    return m;
}
static int cdiv(int a, int b) { return (a + b - 1) / b; }
static const char *old_refusal(int mode, int H, int W, int n, int B, int S, bool qres, bool free_src, int tiles_less = 0, size_t blockrec_less = 0) {
    const int nblk_pose = cdiv(W, 32) * cdiv(H, TC_TILE_H), n16 = cdiv(W, 16) * cdiv(H, 16);
    const int nblk_alloc = (n16 < nblk_pose ? nblk_pose : n16) - tiles_less, ngrp_alloc = cdiv(nblk_alloc, 16);
    const int dnblk = cdiv(W, 32) * cdiv(H, 16), jnblk = cdiv(W, 32) * cdiv(H, TC_JOINT_TILE_H);
    const int nqg = cdiv((H / 4) * (W / 4), 16), jrec_alloc = jnblk + nqg;
    if (mode == DENSE_PAIR) return (dnblk > nblk_alloc || cdiv(dnblk, 16) > ngrp_alloc) ? "internal: dense tile grid exceeds scratch" : nullptr;
    if (mode == DENSE_JOINT && dnblk > nblk_alloc) return "internal: dense tile grid exceeds scratch";
    const size_t nt = ((size_t)n + 1) / 2, cap = (size_t)jrec_alloc * old_max_over_S(n, 2) - blockrec_less;
    const int recs = jnblk + (qres ? nqg : 0);
    const bool fits = (size_t)B <= nt && (size_t)B * kJrec[S] <= old_max_over_S(n, 0) && (size_t)B * kNacc[S] <= old_max_over_S(n, 1) && recs <= jrec_alloc &&
                      (size_t)B * recs * kNacc[S] <= cap;
    if (!fits) return "internal: the joint dense scratch does not hold this many targets";
    if (mode == DENSE_REF && free_src && (size_t)B * recs * kNacc[S] + (size_t)S * B * recs * kNacc[1] > cap)
        return "internal: the inverse groups' records exceed the scratch";
    return nullptr;
}

static bool inside(const DenseView &v, size_t cap) { return v.len == 0 || (v.off <= cap && v.len <= cap - v.off); }
static bool disjoint(const DenseView &u, const DenseView &v) { return u.len == 0 || v.len == 0 || u.off + u.len <= v.off || v.off + v.len <= u.off; }

static long accepted = 0, refused = 0, probed = 0;
static int bad = 0;

static void check(int mode, int H, int W, int n, int B, int S, unsigned flags) {
    const DenseCaps cp = dense_caps(H, W, n);
    DenseViews v;
    const DensePlan p = dense_plan(mode, H, W, n, B, S, flags, &v);
    const bool qres = flags & DF_QRES, free_src = flags & DF_FREE_SRC;
    const char *want = old_refusal(mode, H, W, n, B, S, qres, free_src);
    if ((want == nullptr) != (p.refusal == nullptr) || (want && strcmp(want, p.refusal))) {       // (d)
        if (bad++ < 20) printf("mode %d %dx%d max_pairs %d B %d S %d flags %u: refusal '%s', the drivers' '%s'\n", mode, H, W, n, B, S, flags, p.refusal ? p.refusal : "", want ? want : "");
        return;
    }
    if (p.refusal) { refused++; return; }
    accepted++;
    for (int x = 0; x < DB_COUNT; x++) {
        const size_t cap = x == DB_STATS ? (size_t)p.N : cp.cap[x];
        if (!inside(v.a[x], cap) || !inside(v.b[x], cap) || !inside(v.c[x], cap)) {               // (a)
            if (bad++ < 20) printf("mode %d %dx%d max_pairs %d B %d S %d flags %u: a view of buffer %d leaves its capacity %zu\n", mode, H, W, n, B, S, flags, x, cap);
        }
        if (!disjoint(v.a[x], v.b[x])) {                                                          // (b)
            if (bad++ < 20) printf("mode %d %dx%d max_pairs %d B %d S %d flags %u: the two views of buffer %d overlap\n", mode, H, W, n, B, S, flags, x);
        }
    }
    // (b) by name: what must be there to be disjoint
    bool named = true;
    if (mode != DENSE_PAIR) for (int x : {DB_TGTPACK, DB_SRCPACK, DB_DEPTH_WORK, DB_PCONST, DB_STATE, DB_BLOCKREC, DB_STATS, DB_DEPTH0}) named = named && v.a[x].len && v.b[x].len;
    if (mode == DENSE_JOINT) for (int x : {DB_DELTA, DB_DENSE_REC}) named = named && v.a[x].len && v.b[x].len;
    if (mode == DENSE_JOINT && (flags & DF_LM)) for (int x : {DB_LM_ACCEPT, DB_DENSE_REC_ACC, DB_DEPTH_ACC}) named = named && v.a[x].len && v.b[x].len;
    if (mode == DENSE_REF) for (int x : {DB_TICKETS, DB_PARTIALS, DB_LIN_OUT, DB_SEL_MAPS}) named = named && v.a[x].len && v.b[x].len;
    if (mode == DENSE_REF && free_src) {
        for (int x : {DB_JBLOCKREC, DB_JPART, DB_JTICK}) named = named && v.a[x].len && v.b[x].len;
        named = named && v.b[DB_JBLOCKREC].off == p.jrec2_off && p.jrec2_off == v.a[DB_JBLOCKREC].len;
    }
    if (qres) named = named && v.a[DB_QRES_RHO].len && v.b[DB_QRES_RHO].len && (!free_src || (v.a[DB_QRES_RHO_SRC].len && v.b[DB_QRES_RHO_SRC].len));
    if (!named) { if (bad++ < 20) printf("mode %d %dx%d max_pairs %d B %d S %d flags %u: a view is missing\n", mode, H, W, n, B, S, flags); }
    for (int x = 0; x < DB_COUNT; x++) if (p.off[x] != v.b[x].off) { if (bad++ < 20) printf("plan offset of buffer %d\n", x); }      // what the drivers read
    if (p.SB != (S ? S * B : B) || p.N != (S ? 2 * S * B : B) || p.recs != p.jnblk + p.nqblk || p.jnblk != joint_tiles(H, W)) { if (bad++ < 20) printf("plan fields\n"); }
}

// ---- (e) capacities and offsets worked out by hand from the formulas
struct CapRow { int H, W, n; int nblk, nblk_alloc, ngrp_alloc, ngrp_pad, jrec_alloc; size_t jrec, jblockrec, jpart, jtick, jdepth_acc, dref_ext, qres_rho, qres_rec, jrec_src, qres_rec_src, sel_maps, dense_rec, blockrec; };
struct OffRow { int H, W, n, B, S; unsigned flags; int recs; size_t jrec2_off, jpart_b, jtick_b, qres_b, qres_src_b, tgtpack_b, srcpack_b, blockrec_b, partials_b, sel_b; };

static void pose_consistency() {
    // one window pair: p_fwd = (0.1, 0, ..), p_inv = (0.2, 0, ..), weight 6 -> c = 1; r = 0.3 in the first coordinate of both pairs: value 0.3,
    // gradient c r / |r| = 1 in pose coordinates, carried by A^-T = [[-I, 0], [Tx', -I]] (no rotation): -1 in the first coordinate
    const float poses[12] = {0.1f, 0, 0, 0, 0, 0, 0.2f, 0, 0, 0, 0, 0};
    double g[12] = {0};
    const double v = pose_consist_linearised(poses, 1, 6.0, 1e-3, g);
    bool ok = fabs(v - ((double)0.1f + (double)0.2f)) < 1e-15;
    for (int i = 0; i < 12; i++) ok = ok && fabs(g[i] - (i % 6 == 0 ? -1.0 : 0.0)) < 1e-15;
    // two window pairs with rotations whose inverses are their exact opposites: no residual, no gradient
    const float q[24] = {0.1f, -0.2f, 0.05f, 0.3f, 0.2f, -0.1f, 0, 0, 0, 0.01f, 0, 0, -0.1f, 0.2f, -0.05f, -0.3f, -0.2f, 0.1f, 0, 0, 0, -0.01f, 0, 0};
    double g2[24] = {0};
    const double v2 = pose_consist_linearised(q, 2, 0.1, 1e-3, g2);
    ok = ok && v2 == 0.0;
    for (int i = 0; i < 24; i++) ok = ok && g2[i] == 0.0;
    if (!ok) { printf("pose_consist_linearised\n"); bad++; }
}

int main() {
    const CapRow caps[] = {
        {192, 640, 24, 240, 480, 30, 64, 960, 11796480, 1333440, 16080, 24, 1474560, 2949120, 184320, 737280, 11796480, 737280, 5898240, 23592960, 840960},
        {16, 48, 8, 2, 3, 1, 64, 7, 24576, 3241, 5360, 8, 3072, 6144, 384, 1536, 24576, 1536, 12288, 49152, 1752},
        {28, 48, 9, 4, 6, 1, 64, 14, 53760, 6482, 5360, 10, 6720, 13440, 840, 3360, 43008, 2688, 24192, 96768, 3942},
        {240, 320, 33, 150, 300, 19, 64, 600, 10444800, 1111200, 21440, 34, 1305600, 2611200, 163200, 652800, 9830400, 614400, 5068800, 20275200, 722700},
    };
    for (const CapRow &r : caps) {
        const DenseCaps c = dense_caps(r.H, r.W, r.n);
        const bool same = c.nblk == r.nblk && c.nblk_alloc == r.nblk_alloc && c.ngrp_alloc == r.ngrp_alloc && c.ngrp_pad == r.ngrp_pad && c.jrec_alloc == r.jrec_alloc &&
                          c.cap[DB_JREC] == r.jrec && c.cap[DB_JREC_ACC] == r.jrec && c.cap[DB_JBLOCKREC] == r.jblockrec && c.cap[DB_JPART] == r.jpart && c.cap[DB_JTICK] == r.jtick &&
                          c.cap[DB_JDEPTH_ACC] == r.jdepth_acc && c.cap[DB_DREF_EXT] == r.dref_ext && c.cap[DB_QRES_RHO] == r.qres_rho && c.cap[DB_QRES_REC] == r.qres_rec &&
                          c.cap[DB_JREC_SRC] == r.jrec_src && c.cap[DB_QRES_REC_SRC] == r.qres_rec_src && c.cap[DB_SEL_MAPS] == r.sel_maps && c.cap[DB_DENSE_REC] == r.dense_rec &&
                          c.cap[DB_BLOCKREC] == r.blockrec && c.cap[DB_DREF_NORMS] == 32 && c.cap[DB_DELTA] == (size_t)r.n * 8;
        if (!same) { printf("capacities of %dx%d max_pairs %d\n", r.H, r.W, r.n); bad++; }
    }
    const OffRow offs[] = {
        {192, 640, 24, 6, 2, DF_ARGMIN | DF_QRES | DF_FREE_SRC, 960, 558720, 8040, 12, 92160, 92160, 1474560, 1494576, 164160, 10260, 2949120},
        {192, 640, 24, 3, 4, 0, 480, 482400, 0, 0, 0, 0, 1474560, 1494576, 164160, 10260, 2949120},
        {16, 48, 8, 1, 4, DF_QRES | DF_FREE_SRC, 7, 2345, 2680, 4, 192, 192, 3072, 3600, 456, 228, 6144},
        {16, 48, 8, 2, 2, DF_ARGMIN | DF_FREE_SRC, 4, 776, 2680, 4, 0, 0, 3072, 3600, 456, 228, 6144},
    };
    for (const OffRow &r : offs) {
        DenseViews v;
        const DensePlan p = dense_plan(DENSE_REF, r.H, r.W, r.n, r.B, r.S, r.flags, &v);
        const bool fs = r.flags & DF_FREE_SRC, q = r.flags & DF_QRES;
        const bool same = !p.refusal && p.recs == r.recs && p.jrec2_off == r.jrec2_off && (!fs || (v.b[DB_JBLOCKREC].off == r.jrec2_off && v.b[DB_JPART].off == r.jpart_b && v.b[DB_JTICK].off == r.jtick_b)) &&
                          (!q || v.b[DB_QRES_RHO].off == r.qres_b) && (!(q && fs) || v.b[DB_QRES_RHO_SRC].off == r.qres_src_b) && v.b[DB_TGTPACK].off == r.tgtpack_b &&
                          v.b[DB_SRCPACK].off == r.srcpack_b && v.b[DB_BLOCKREC].off == r.blockrec_b && v.b[DB_PARTIALS].off == r.partials_b && v.b[DB_SEL_MAPS].off == r.sel_b &&
                          v.b[DB_STATE].off == (size_t)r.S * r.B && v.b[DB_LIN_OUT].off == (size_t)r.S * r.B * 60;
        if (!same) { printf("offsets of %dx%d max_pairs %d B %d S %d flags %u\n", r.H, r.W, r.n, r.B, r.S, r.flags); bad++; }
    }
    {   // the library's joint mode and the pair form at 16 x 48, max_pairs 8, B = 2, S = 2: S B = 4 pairs further on, 2 tiles of 32 x 16 per pair
        DenseViews jv, qv;
        const DensePlan j = dense_plan(DENSE_JOINT, 16, 48, 8, 2, 2, DF_LM, &jv);
        const DensePlan q = dense_plan(DENSE_PAIR, 16, 48, 8, 2, 2, DF_ARGMIN, &qv);
        const bool same = !j.refusal && j.dnblk == 2 && jv.b[DB_BLOCKREC].off == 4 * 2 * 57 && jv.b[DB_DELTA].off == 32 && jv.b[DB_DENSE_REC].off == 4 * 768 * 8 && jv.b[DB_LM_ACCEPT].off == 4 &&
                          jv.a[DB_LM_ACCEPT].len == 2 && jv.b[DB_DEPTH_ACC].off == 4 * 768 && jv.a[DB_JBLOCKREC].len == 2 * 4 * 97 && !q.refusal && qv.a[DB_BLOCKREC].len == 8 * 2 * 57 &&
                          qv.b[DB_SEL_MAPS].off == 8 * 768 && qv.a[DB_SEL_MAPS].len == 4 * 768 && qv.a[DB_DENSE_REC2].len == 0;
        if (!same) { printf("offsets of the joint mode / the pair form at 16x48\n"); bad++; }
    }
    {   // (d) outside the contract, where the three refusals fire: more targets than the handle has; a handle whose record buffers are
        // smaller than dense_caps makes them (by one tile / by one float under an exactly full jblockrec row: 16 x 48, max_pairs 8, B = 1, S = 4)
        struct Probe { int mode, H, W, n, B, S; unsigned flags; int tiles_less; size_t blockrec_less; const char *text; };
        const Probe probes[] = {
            {DENSE_REF, 16, 48, 8, 5, 1, 0, 0, 0, "internal: the joint dense scratch does not hold this many targets"},
            {DENSE_JOINT, 16, 48, 8, 3, 2, DF_LM, 0, 0, "internal: the joint dense scratch does not hold this many targets"},
            {DENSE_REF, 192, 640, 24, 4, 4, DF_QRES, 0, 0, "internal: the joint dense scratch does not hold this many targets"},
            {DENSE_REF, 16, 48, 8, 1, 4, DF_QRES | DF_FREE_SRC, 0, 1, "internal: the inverse groups' records exceed the scratch"},
            {DENSE_REF, 16, 48, 8, 1, 4, DF_QRES | DF_FREE_SRC, 0, 0, nullptr},
            {DENSE_REF, 16, 48, 8, 1, 4, DF_QRES, 0, 897, "internal: the joint dense scratch does not hold this many targets"},
            {DENSE_PAIR, 16, 48, 8, 8, 0, 0, 2, 0, "internal: dense tile grid exceeds scratch"},
            {DENSE_PAIR, 192, 640, 24, 2, 2, DF_LM, 241, 0, "internal: dense tile grid exceeds scratch"},
            {DENSE_JOINT, 16, 48, 8, 2, 2, 0, 2, 0, "internal: dense tile grid exceeds scratch"},
            {DENSE_JOINT, 16, 48, 8, 2, 2, 0, 1, 0, nullptr},
        };
        for (const Probe &q : probes) {
            DenseCaps cp = dense_caps(q.H, q.W, q.n);
            cp.nblk_alloc -= q.tiles_less; cp.ngrp_alloc = (cp.nblk_alloc + 15) / 16; cp.cap[DB_JBLOCKREC] -= q.blockrec_less;
            const DensePlan p = dense_plan(cp, q.mode, q.H, q.W, q.n, q.B, q.S, q.flags);
            const char *old = old_refusal(q.mode, q.H, q.W, q.n, q.B, q.S, q.flags & DF_QRES, q.flags & DF_FREE_SRC, q.tiles_less, q.blockrec_less);
            const bool same = q.text ? (p.refusal && old && !strcmp(p.refusal, q.text) && !strcmp(old, q.text)) : (!p.refusal && !old);
            if (!same) { printf("probe mode %d %dx%d max_pairs %d B %d S %d: '%s', the drivers' '%s', expected '%s'\n", q.mode, q.H, q.W, q.n, q.B, q.S, p.refusal ? p.refusal : "", old ? old : "", q.text ? q.text : ""); bad++; }
            else if (q.text) probed++;
        }
    }
    // ---- the grid
    const int Hs[] = {4, 8, 16, 28, 48, 192, 240}, Ws[] = {4, 16, 48, 320, 624, 640};
    for (int H : Hs) for (int W : Ws) for (int n = 1; n <= 33; n++) {
        const bool q4 = H % 4 == 0 && W % 4 == 0;
        for (int N = 1; N <= n; N++)                               // the pair form outside a window: N pairs
            for (unsigned lm : {0u, (unsigned)DF_LM}) check(DENSE_PAIR, H, W, n, N, 0, lm);
        for (int S = 1; S <= 4; S++) for (int B = 1; 2 * B * S <= n; B++) {
            for (unsigned am : {0u, (unsigned)DF_ARGMIN}) {
                for (unsigned lm : {0u, (unsigned)DF_LM}) {
                    check(DENSE_PAIR, H, W, n, B, S, am | lm);
                    if (S >= 2 && S <= JMAXS_OWN) check(DENSE_JOINT, H, W, n, B, S, am | lm);
                }
                for (unsigned qr : {0u, (unsigned)DF_QRES}) {
                    if (qr && !q4) continue;
                    for (unsigned fs : {0u, (unsigned)DF_FREE_SRC}) check(DENSE_REF, H, W, n, B, S, am | qr | fs);
                    if (B >= 2) check(DENSE_REF, H, W, n, B, S, am | qr | DF_MERGED);      // merged calls: plain refinements with fixed source maps
                }
                check(DENSE_REF, H, W, n, B, S, am | DF_EXPORT);
                check(DENSE_REF, H, W, n, B, S, am | DF_EXPORT | DF_EXPORT_SRC);
            }
            if (B >= 2) check(DENSE_PAIR, H, W, n, B, S, DF_MERGED);                       // ... per-pair Gauss-Newton calls without the selection
        }
    }
    pose_consistency();
    if (accepted != 530460 || refused != 0) { printf("grid: %ld accepted, %ld refused; 530460 and 0 expected\n", accepted, refused); bad++; }
    printf(bad ? "FAILED\n" : "dense_plan_host ok: %ld plans accepted, %ld refused in the grid, %ld refusals probed outside it\n", accepted, refused, probed);
    return bad ? 1 : 0;
}
