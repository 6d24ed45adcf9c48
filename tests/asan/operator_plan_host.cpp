// Stand-alone sanitizer program for the decisions of the drop-in operators (csrc/operator_plan.h).  Its own main, no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I tightly_coupled_sfm_amd/csrc tests/asan/operator_plan_host.cpp -o operator_plan_host && ./operator_plan_host
//
// (the runtimes are linked statically: the program then runs as it is wherever the process's library list does not start with them)
//   The three backward plans over every NULL / wanted combination of their inputs -- 16, 32 and 16 cases -- against truth tables written from
//     what each output needs, not from the plan: d_depth_s receives flow through g_proj_depth alone and is zeroed without it, d_depth_t
//     needs k_warp_bwd, d_pose needs k_warp_bwd, its records and the tail; g_rec flows from g_diff, the depth cotangents from g_weight.
//   The geometry at its edges: block counts and lg_hw around the powers of two, the disp_to_depth backward split for n = 1 .. 9 aligned and
//     not, the window-loss grids for hw & 3 = 0 .. 3, the tile grid around one tile, the smooth-loss scratch.
//   -DPLANT=1 | 2 | 3 plants one wrong decision behind the plan (a d_depth_s that is never zeroed, depth cotangents computed without
//     g_weight, a block count rounded down): the program must then fail -- tests/test_operator_plan_cpu.py builds all four.
#include <stdio.h>
#include <string.h>
#include "operator_plan.h"

using namespace tc;

#ifndef PLANT
#define PLANT 0
#endif

static int bad = 0;
#define CHECK(cond, ...)                                                                             \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (bad++ < 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                            \
    } while (0)

// ---- the plan as the drivers read it, with the planted faults
static WarpBwdPlan warp_plan(bool gpd, bool dt, bool ds, bool pose, size_t hw) {
    WarpBwdPlan p = warp_bwd_plan(gpd, dt, ds, pose, hw);
    if (PLANT == 1) p.zero_ds = false;
    return p;
}
static PhotoMapsBwdPlan maps_plan(bool gdiff, bool gweight, bool rec, bool pd, bool cd) {
    PhotoMapsBwdPlan p = photo_maps_bwd_plan(gdiff, gweight, rec, pd, cd);
    if (PLANT == 2 && (pd || cd)) { p.dep_on = true; p.launch = true; }
    return p;
}
static unsigned blocks(size_t hw) { return PLANT == 3 ? (unsigned)(hw / 256) : pixel_blocks(hw); }

// ---- warp backward: case = g_proj_depth << 3 | d_depth_t << 2 | d_depth_s << 1 | d_pose; columns: records reserved, scatter buffers
// reserved, d_depth_s zeroed, scatter chain, k_warp_bwd, pose tail, pair constants
static const char *const kWarpTruth[16] = {
    // no g_proj_depth: nothing flows into the source depth -- a wanted d_depth_s is zeroed, and that needs no kernel
    "0000000", "1000111", "0010000", "1010111", "0000101", "1000111", "0010101", "1010111",
    // g_proj_depth given: d_depth_s takes the scatter chain, alone or beside k_warp_bwd
    "0000000", "1000111", "0101001", "1101111", "0000101", "1000111", "0101101", "1101111",
};

static void check_warp() {
    for (int c = 0; c < 16; c++) {
        const bool gpd = c & 8, dt = c & 4, ds = c & 2, pose = c & 1;
        const WarpBwdPlan p = warp_plan(gpd, dt, ds, pose, 561);
        const char got[8] = {(char)('0' + p.reserve_rec), (char)('0' + p.reserve_scatter), (char)('0' + p.zero_ds), (char)('0' + p.scatter),
                             (char)('0' + p.bwd), (char)('0' + p.tail), (char)('0' + p.pair_consts), 0};
        CHECK(strcmp(got, kWarpTruth[c]) == 0, "warp backward case %d: %s, truth %s", c, got, kWarpTruth[c]);
        // every wanted output is written exactly once: d_depth_s by the memset or by the chain, never both
        CHECK(!ds || (p.zero_ds != p.scatter), "case %d: d_depth_s written %d times", c, p.zero_ds + p.scatter);
        CHECK(ds || (!p.zero_ds && !p.scatter), "case %d: d_depth_s written though not wanted", c);
        CHECK(p.tail <= p.bwd && p.tail == p.reserve_rec && p.scatter == p.reserve_scatter, "case %d: a launch without its input or its buffer", c);
        CHECK(p.pair_consts == (p.scatter || p.bwd || p.tail), "case %d: pair constants", c);
    }
}

// ---- photometric-maps backward: case = g_diff << 4 | g_weight << 3 | g_rec << 2 | g_proj_depth << 1 | g_comp_depth
enum { ABSENT, ZEROED, COMPUTED };
static int state_of(bool wanted, bool cotangent) { return !wanted ? ABSENT : (cotangent ? COMPUTED : ZEROED); }

static void check_maps() {
    for (int c = 0; c < 32; c++) {
        const bool gdiff = c & 16, gweight = c & 8, rec = c & 4, pd = c & 2, cd = c & 1;
        const PhotoMapsBwdPlan p = maps_plan(gdiff, gweight, rec, pd, cd);
        // what each output needs: g_rec flows from g_diff alone, the two depth cotangents from g_weight alone
        const int s_rec = state_of(rec, gdiff), s_pd = state_of(pd, gweight), s_cd = state_of(cd, gweight);
        // what the driver does with the plan: the launch writes g_rec under rec_on and the wanted depth outputs under dep_on
        const int d_rec = p.zero_rec ? ZEROED : (p.launch && p.rec_on && rec ? COMPUTED : ABSENT);
        const int d_pd = p.zero_pd ? ZEROED : (p.launch && p.dep_on && pd ? COMPUTED : ABSENT);
        const int d_cd = p.zero_cd ? ZEROED : (p.launch && p.dep_on && cd ? COMPUTED : ABSENT);
        CHECK(d_rec == s_rec && d_pd == s_pd && d_cd == s_cd, "maps backward case %d: outputs %d %d %d, truth %d %d %d", c, d_rec, d_pd, d_cd, s_rec, s_pd, s_cd);
        CHECK(p.launch == (s_rec == COMPUTED || s_pd == COMPUTED || s_cd == COMPUTED), "case %d: launch %d", c, p.launch);
        CHECK(!(p.rec_on && !gdiff) && !(p.dep_on && !gweight), "case %d: a cotangent read that was not given", c);
        CHECK(!(p.zero_rec && p.rec_on) && !((p.zero_pd || p.zero_cd) && p.dep_on), "case %d: an output zeroed and computed", c);
    }
    // a few rows by hand
    const PhotoMapsBwdPlan a = maps_plan(true, false, true, true, false);      // g_weight absent: g_proj_depth zeroed, g_rec computed
    CHECK(a.rec_on && !a.dep_on && !a.zero_rec && a.zero_pd && !a.zero_cd && a.launch, "row a");
    const PhotoMapsBwdPlan b = maps_plan(false, false, true, true, true);      // no cotangent: three memsets, no launch
    CHECK(!b.rec_on && !b.dep_on && b.zero_rec && b.zero_pd && b.zero_cd && !b.launch, "row b");
    const PhotoMapsBwdPlan d = maps_plan(true, true, false, false, true);      // only g_comp_depth wanted
    CHECK(!d.rec_on && d.dep_on && !d.zero_rec && !d.zero_pd && !d.zero_cd && d.launch, "row d");
}

// ---- composed photometric backward: case = g_diff << 3 | g_weight << 2 | g_img_rec << 1 | an output wanted; columns: forward warp runs,
// writes img_rec, writes the depth planes, then the sources of the warp backward's g_rec, g_proj_depth, g_comp_depth (N one, C aller's, A ssembled)
static const char *const kPhotoTruth[16] = {
    "000NNN", "000NNN", "000NNN", "000CNN",      // neither g_diff nor g_weight: no assembly, g_img_rec goes straight to the warp
    "000NNN", "101NAA", "000NNN", "101CAA",      // g_weight alone: the depth planes and their cotangents; g_rec is still the caller's
    "000NNN", "110ANN", "000NNN", "110ANN",      // g_diff alone: the assembly's g_rec (it has added g_img_rec already)
    "000NNN", "111AAA", "000NNN", "111AAA",
};

static void check_photo() {
    const char names[3] = {'N', 'C', 'A'};
    for (int c = 0; c < 16; c++) {
        const PhotoBwdPlan p = photo_bwd_plan(c & 8, c & 4, c & 2, c & 1);
        const char got[7] = {(char)('0' + p.fwd64), (char)('0' + p.fwd_rec), (char)('0' + p.fwd_depth), names[p.g_rec], names[p.g_pd], names[p.g_cd], 0};
        CHECK(strcmp(got, kPhotoTruth[c]) == 0, "photometric backward case %d: %s, truth %s", c, got, kPhotoTruth[c]);
        // an assembled cotangent exists only where the forward warp wrote its plane
        CHECK((p.g_rec == COT_ASSEMBLED) <= p.fwd_rec && (p.g_pd == COT_ASSEMBLED) <= p.fwd_depth && (p.g_cd == COT_ASSEMBLED) <= p.fwd_depth, "case %d: a plane read that was not written", c);
        CHECK(p.g_rec != COT_CALLER || (c & 2), "case %d: the caller's g_img_rec read though absent", c);
    }
}

// ---- geometry
static void check_geometry() {
    const struct { size_t hw; unsigned blocks; int lg; } px[] = {{16, 1, 4}, {35, 1, 6}, {255, 1, 8}, {256, 1, 8}, {257, 2, 9}, {1023, 4, 10}, {1024, 4, 10}, {1025, 5, 11}};
    for (const auto &r : px) {
        CHECK(blocks(r.hw) == r.blocks, "hw %zu: %u blocks", r.hw, blocks(r.hw));
        CHECK((size_t)blocks(r.hw) * 256 >= r.hw && ((size_t)blocks(r.hw) - 1) * 256 < r.hw, "hw %zu: the blocks do not cover the plane exactly", r.hw);
        CHECK(warp_plan(true, true, true, true, r.hw).lg_hw == r.lg && lg_ceil(r.hw) == r.lg, "hw %zu: lg_hw %d", r.hw, lg_ceil(r.hw));
        CHECK(median_hist_blocks(r.hw) == (int)r.blocks, "hw %zu: median blocks", r.hw);
    }
    CHECK(median_hist_blocks(256 * 63) == 63 && median_hist_blocks(256 * 64) == 64 && median_hist_blocks(256 * 64 + 1) == 64 && median_hist_blocks(640 * 192) == 64, "median blocks cap at 64");
    for (long long n = 1; n <= 9; n++)
        for (int aligned = 0; aligned <= 1; aligned++) {
            const DispBwdSplit s = disp_bwd_split(n, aligned != 0);
            const long long tail = s.threads - s.n4;
            CHECK(s.n4 >= 0 && tail >= 0 && 4 * s.n4 + tail == n, "n %lld aligned %d: %lld groups + %lld tail elements", n, aligned, s.n4, tail);      // every element once
            CHECK(aligned ? (s.n4 == n / 4 && tail < 4) : s.n4 == 0, "n %lld aligned %d: n4 %lld", n, aligned, s.n4);
        }
    const struct { int hw, nu, nbx, nb_bwd; } wl[] = {{32, 8, 1, 1}, {33, 9, 1, 1}, {34, 10, 1, 1}, {35, 11, 1, 1}, {561, 141, 1, 1}, {1024, 256, 1, 1}, {1028, 257, 1, 2},
                                                      {2048, 512, 1, 2}, {2052, 513, 2, 3}, {2051, 515, 2, 3}};
    for (const auto &r : wl) {
        const WindowLossGrid g = window_loss_grid(r.hw, 2);
        CHECK(g.nu == r.nu && g.nbx == r.nbx && g.nb_bwd == r.nb_bwd, "window loss hw %d: nu %d nbx %d bwd %d", r.hw, g.nu, g.nbx, g.nb_bwd);
        CHECK(4 * (r.hw >> 2) + (g.nu - (r.hw >> 2)) == r.hw, "window loss hw %d: the units do not cover the plane", r.hw);
    }
    const int ws[3] = {31, 32, 33}, hs[3] = {7, 8, 9};
    const unsigned want[3] = {1, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const TileGrid t = tile_grid(ws[i], hs[j], 32, 8);
            CHECK(t.x == want[i] && t.y == want[j], "tile grid of %d x %d: %u x %u", ws[i], hs[j], t.x, t.y);
        }
    const SmoothScratch s = smooth_scratch(2, 561);      // 17 x 33: three blocks
    CHECK(s.nb == 3 && s.partial_off == 4 && s.n_partial == 12 && s.bytes == 64, "smooth scratch: nb %d off %zu n %zu bytes %zu", s.nb, s.partial_off, s.n_partial, s.bytes);
    for (int N = 1; N <= 5; N++) {
        const SmoothScratch t = smooth_scratch(N, 35);
        CHECK(t.partial_off * sizeof(float) == (size_t)N * sizeof(double) && t.bytes == (t.partial_off + t.n_partial) * sizeof(float) && t.n_partial == (size_t)N * t.nb * 2,
              "smooth scratch at N %d: the means and the partial sums overlap or leave a gap", N);
    }
}

int main() {
    check_warp();
    check_maps();
    check_photo();
    check_geometry();
    if (bad) { printf("operator_plan_host: %d checks failed (PLANT=%d)\n", bad, PLANT); return 1; }
    printf("operator_plan_host ok: 16 + 32 + 16 backward cases, geometry\n");
    return 0;
}
