// layout.h -- the layout constants that host arithmetic and kernels share: tile sizes, record layouts, capacities of fixed tables.
// No HIP include: the kernel headers include it, and so do the host-only plan headers (dense_plan.h), which compile with a plain C++
// compiler.
#pragma once

#if defined(__HIPCC__)
#define TC_LAYOUT_HD __host__ __device__
#else
#define TC_LAYOUT_HD
#endif

// tile geometry of the hot kernel (one place to retune)
#ifndef TC_TILE_H
#define TC_TILE_H 16
#endif
// tile height of k_dense_joint's own grid (32 x 8 tiles of 256 threads by default; 16: the round-4 grid shared with the pair-form kernels)
#ifndef TC_JOINT_TILE_H
#define TC_JOINT_TILE_H 8
#endif

namespace tc {

constexpr int TILE_W = 32, TILE_H = TC_TILE_H, TILE_NT = TILE_W * TILE_H;      // (A/B builds: -DTC_TILE_H=8 -> 32 x 8 tiles of 256 threads)
constexpr int kJointTileW = 32, kJointTileH = TC_JOINT_TILE_H;      // k_dense_joint / k_dense_joint2's tiles (both joint modes launch on them)
// the pair-form dense kernel's own tile grid (32x16 tiles of 512 threads, as k_linearize; 16x16 / 256 threads measured slower except
// for 320x240 at B=1: 10.9 vs 11.8 us per launch there, 234 vs 200 us with the chip full)
constexpr int kDenseTileW = 32, kDenseTileH = 16, kDenseNT = kDenseTileW * kDenseTileH;

constexpr int RG = 16;       // workgroups per in-launch reduction group

template <int NP>
struct AccLayout {
    static constexpr int NH = NP * (NP + 1) / 2;
    static constexpr int OFF_HP = 0, OFF_GP = NH, OFF_HD = NH + NP, OFF_GD = 2 * NH + NP, OFF_S = 2 * NH + 2 * NP;
    static constexpr int NACC = 2 * NH + 2 * NP + 3;  // + sum(M W diff), sum(M), sum(dd)
};
constexpr int kMaxAcc = AccLayout<7>::NACC;
constexpr int kLinOut = 7 * 7 + 7 + 4;

constexpr int TC_MAX_COAL = 16;                // queued calls one merged launch sequence takes at most (kernels.h: CoalTab)

constexpr int JMAXS = 4;                       // sources per target the joint kernels are instantiated for (1 .. JMAXS) under the reference's loss
constexpr int JMAXS_OWN = 3;                   // ... and in the library's own joint mode (opts.dense_joint with window rule PAIR: 2 .. 3)
template <int NS> struct JointLayout {
    static constexpr int NP = 6 * NS;
    static constexpr int NHJ = NP * (NP + 1) / 2;
    static constexpr int OFF_G = NHJ, OFF_S = NHJ + NP, OFF_SHARE = OFF_S + 3, OFF_NM = OFF_SHARE + NS, NACC = OFF_NM + NS;
    static constexpr int JREC = (2 + 6 * NS + 3) / 4 * 4;     // floats per pixel record: g_rho, Dd, B[NS][6], padded to float4s
    TC_LAYOUT_HD static constexpr int tri(int r, int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }
};
constexpr int kJointSplitMax = 8;              // workgroups that share one target's record sum at most (JointSolveParams::nsplit)

constexpr int QRES_CELLS_PER_WG = 16;      // 4 waves x 4 cells: the cells of a wave are loaded together (a first version walked 16 cells per wave
                                           // one dependent load after the other: 25 us per linearisation at 240x320)

}  // namespace tc
