// The decisions of the drop-in operators (operators_host.h), host only: which launches, memsets and reservations a backward entry makes
// when cotangents or outputs are NULL, and the launch and scratch geometry of every operator.  Booleans and integer arithmetic, no HIP, no
// environment, no handle: tests/asan/operator_plan_host.cpp builds it alone and plays every NULL / wanted combination against a truth
// table written from what each output needs, and the geometry at its edges.  The drivers read these decisions and make none of their own.
//
// The invariants.
//  1. Warp backward.  d_depth_s receives flow through g_proj_depth ALONE (the scatter chain: gmax, scatter, fix-out); without it a wanted
//     d_depth_s is zeroed by a memset and nothing else runs on its behalf.  d_depth_t and d_pose come from k_warp_bwd, d_pose through the
//     pose tail behind it and the workgroup records it reserves.  Pair constants are formed exactly when a kernel runs.  Nothing wanted:
//     nothing reserved, zeroed or launched.
//  2. Warp backward.  lg_hw is the smallest l with 2^l >= hw (the fixed-point scale of the scatter sums).
//  3. Photometric-maps backward.  g_rec flows from g_diff alone, g_proj_depth and g_comp_depth from g_weight alone.  A wanted output whose
//     cotangent is absent is zeroed by a memset, never written by the launch; the launch happens exactly when some output has its cotangent.
//  4. Composed photometric backward.  The float64 forward warp runs exactly when an output is wanted and g_diff or g_weight is given, and
//     writes img_rec for g_diff, the two depth planes for g_weight.  The warp backward's g_rec is the assembly's plane under g_diff (it
//     already holds g_img_rec's share), else the caller's g_img_rec; its g_proj_depth and g_comp_depth are the assembly's under g_weight,
//     else absent.
//  5. Geometry.  A plane of hw pixels takes ceil(hw / 256) blocks of 256 threads; the median's histogram passes take min(that, 64).
//  6. Geometry.  disp_to_depth's backward gives every aligned group of four elements one thread and every tail element one; without
//     16-byte alignment every element is a tail element.
//  7. Geometry.  The window loss works on units: hw / 4 groups of four pixels and hw % 4 tail pixels.  The forward takes `units_per_thread`
//     units per thread, the backward one.
//  8. Geometry.  The smooth loss's scratch is N float64 means, then N x nb x 2 float32 partial sums, nb the plane's block count.
//  9. Geometry.  A tile grid covers W x H with ceil(W / tw) x ceil(H / th) tiles.
#pragma once
#include <stddef.h>

namespace tc {

// ---- launch and scratch geometry
inline unsigned pixel_blocks(size_t hw) { return (unsigned)((hw + 255) / 256); }                               // invariant 5
inline int median_hist_blocks(size_t hw) { return pixel_blocks(hw) < 64 ? (int)pixel_blocks(hw) : 64; }
inline int lg_ceil(size_t hw) {                                                                                // invariant 2
    int lg = 0;
    while (((size_t)1 << lg) < hw) lg++;
    return lg;
}

struct DispBwdSplit { long long n4, threads; };                                                                // invariant 6
inline DispBwdSplit disp_bwd_split(long long n, bool aligned16) {
    const long long n4 = aligned16 ? n / 4 : 0;
    return {n4, n4 + (n - 4 * n4)};
}

struct WindowLossGrid { int nu, nbx, nb_bwd; };      // units per target; blocks per target of the forward / of the backward       invariant 7
inline WindowLossGrid window_loss_grid(int hw, int units_per_thread) {
    const int nu = (hw >> 2) + (hw & 3), per = 256 * units_per_thread;
    return {nu, (nu + per - 1) / per, (nu + 255) / 256};
}

struct SmoothScratch { int nb; size_t partial_off, n_partial, bytes; };      // offsets and counts in floats (the means lie at 0)   invariant 8
inline SmoothScratch smooth_scratch(int N, size_t hw) {
    const int nb = (int)pixel_blocks(hw);
    const size_t n_partial = (size_t)N * nb * 2;
    return {nb, (size_t)N * 2, n_partial, ((size_t)N * 2 + n_partial) * sizeof(float)};
}

struct TileGrid { unsigned x, y; };                                                                            // invariant 9
inline TileGrid tile_grid(int W, int H, int tw, int th) { return {(unsigned)((W + tw - 1) / tw), (unsigned)((H + th - 1) / th)}; }

// ---- warp backward (invariants 1, 2)
struct WarpBwdPlan {
    bool reserve_rec;        // the pose gradient's workgroup records
    bool reserve_scatter;    // the fixed-point scatter sums and the per-item max |g_proj_depth|
    bool zero_ds;            // d_depth_s is merely zeroed
    bool scatter;            // k_warp_gmax, k_warp_scatter, k_warp_fix_out
    bool bwd;                // k_warp_bwd
    bool tail;               // k_warp_pose_tail
    bool pair_consts;        // a kernel runs: the call's pair constants are needed
    int lg_hw;
};
inline WarpBwdPlan warp_bwd_plan(bool g_proj_depth, bool want_dt, bool want_ds, bool want_pose, size_t hw) {
    WarpBwdPlan p;
    p.scatter = p.reserve_scatter = want_ds && g_proj_depth;
    p.zero_ds = want_ds && !g_proj_depth;
    p.bwd = want_dt || want_pose;
    p.tail = p.reserve_rec = want_pose;
    p.pair_consts = p.scatter || p.bwd;
    p.lg_hw = lg_ceil(hw);
    return p;
}

// ---- photometric-maps backward (invariant 3)
struct PhotoMapsBwdPlan { bool rec_on, dep_on, zero_rec, zero_pd, zero_cd, launch; };
inline PhotoMapsBwdPlan photo_maps_bwd_plan(bool g_diff, bool g_weight, bool want_rec, bool want_pd, bool want_cd) {
    PhotoMapsBwdPlan p;
    p.rec_on = want_rec && g_diff;
    p.dep_on = (want_pd || want_cd) && g_weight;
    p.zero_rec = want_rec && !p.rec_on; p.zero_pd = want_pd && !p.dep_on; p.zero_cd = want_cd && !p.dep_on;
    p.launch = p.rec_on || p.dep_on;
    return p;
}

// ---- composed photometric backward (invariant 4)
enum { COT_NONE = 0, COT_CALLER = 1, COT_ASSEMBLED = 2 };      // where a cotangent of the warp backward comes from
struct PhotoBwdPlan {
    bool fwd64, fwd_rec, fwd_depth;      // the float64 forward warp and the planes it writes
    int g_rec, g_pd, g_cd;               // COT_*
};
inline PhotoBwdPlan photo_bwd_plan(bool g_diff, bool g_weight, bool g_img_rec, bool any_wanted) {
    PhotoBwdPlan p;
    p.fwd64 = any_wanted && (g_diff || g_weight);
    p.fwd_rec = p.fwd64 && g_diff; p.fwd_depth = p.fwd64 && g_weight;
    p.g_rec = !any_wanted ? COT_NONE : (g_diff ? COT_ASSEMBLED : (g_img_rec ? COT_CALLER : COT_NONE));
    p.g_pd = p.g_cd = any_wanted && g_weight ? COT_ASSEMBLED : COT_NONE;
    return p;
}

}  // namespace tc
