// frame_scale_kernel.h -- per-frame DNet scales: the exact lower median of EVERY frame's masked heights in ONE launch.
//   k_median_frames  input: the key planes [N][H*W] k_ground (scale_kernel.h) writes -- float bits of the height where the ground
//              mask holds, 0xFFFFFFFF elsewhere.  One workgroup per frame (grid.x = N) runs the four MSB-first 8-bit rounds of
//              k_sel_hist / k_sel_pick inside the launch: a 256-bin histogram in LDS with INTEGER atomics (the counts do not depend
//              on the order of the adds, so the selected key is the chain's, bit for bit), a pick (parallel prefix sum over the
//              bins), a barrier, the next round on the narrowed prefix.  No global histogram, no memset, nothing between workgroups.
//   Contention: in the top round nearly every height shares its exponent byte (and in the second round a wave's 64 neighbouring
//              ground pixels share one or two bins), so a wave's adds would queue on one LDS address.  The counting lanes of a wave
//              therefore add the bin of their first lane ONCE, with the number of lanes that share it (readfirstlane + ballot +
//              popcount), and only lanes of other bins add for themselves: one LDS atomic per wave and key in the top round.
//              (Repeating the step for up to eight bins per wave was measured and is slower: 56 against 28 us per frame on keys
//              spread over all bins of a round, where nothing queues and the extra ballots are pure cost.)
//   Reading:   ONE workgroup reads a 192 x 640 plane (480 KB) in 12.5 us, and again in 9-10 us per later round (in-kernel stamps), so
//              the plane is read from memory ONCE.  The top round, which has to see every key, also appends the masked keys to a list in LDS (one atomic
//              per wave and key: the wave's count, lanes place themselves by their rank in the ballot); the other three rounds
//              walk that list.  A frame with more masked keys than the list holds (lds_keys, at most kMedianLdsKeys) reads its
//              plane again in every round instead -- the same counts, hence the same bits.  Planes whose size is a multiple of four
//              keys are read as 16-byte vectors, eight per thread in flight (other sizes key by key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tc {

constexpr int kMedianThreads = 1024, kMedianUnroll = 8;
constexpr int kMedianLdsKeys = 36864;        // 144 KB of the CU's 160 KB: 30 % of a 192 x 640 frame

// one key into the round's histogram; `on`: the key counts in this round
__device__ __forceinline__ void median_hist_add(unsigned *hist, unsigned key, bool on, int shift, int lane) {
    if (on) {
        const unsigned bin = (key >> shift) & 255u;
        const unsigned lead = (unsigned)__builtin_amdgcn_readfirstlane((int)bin);      // the first counting lane's bin
        const bool same = bin == lead;
        const unsigned long long mates = __ballot(same);                              // (counting lanes only: the others are masked off)
        if (same) {
            if (lane == __ffsll((long long)mates) - 1) atomicAdd(&hist[lead], (unsigned)__popcll(mates));
        } else {
            atomicAdd(&hist[bin], 1u);
        }
    }
}

// the top round: every masked key into the histogram of its top byte and onto the list (while it has room)
__device__ __forceinline__ void median_first_add(unsigned *hist, unsigned *list, unsigned *list_n, int lds_keys, unsigned key, int lane) {
    const bool on = key != 0xFFFFFFFFu;
    median_hist_add(hist, key, on, 24, lane);
    if (on) {
        const unsigned long long mine = __ballot(true);                               // the masked lanes of this wave
        unsigned at = 0;
        if (lane == __ffsll((long long)mine) - 1) at = atomicAdd(list_n, (unsigned)__popcll(mine));
        at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);                        // (the first masked lane is the one that added)
        const unsigned pos = at + (unsigned)__popcll(mine & ((1ull << lane) - 1ull));
        if (pos < (unsigned)lds_keys) list[pos] = key;
    }
}

__global__ __launch_bounds__(kMedianThreads) void k_median_frames(const unsigned *keys, int hw, int lds_keys, float real_cam_height,
                                                                   float *scale_out, float *median_out, int *count_out) {
    __shared__ unsigned list[kMedianLdsKeys];
    __shared__ unsigned hist[256], scan[2][256];
    __shared__ unsigned s_k, s_prefix, s_list_n;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const unsigned *kp = keys + (size_t)n * hw;
    const bool vec = (hw & 3) == 0 && ((uintptr_t)kp & 15) == 0;             // (uniform over the workgroup)
    lds_keys = lds_keys < 0 ? 0 : (lds_keys > kMedianLdsKeys ? kMedianLdsKeys : lds_keys);
    unsigned prefix = 0, k = 0, count = 0;
    if (tid == 0) s_list_n = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned want = shift == 24 ? 0u : prefix >> (shift + 8);
        // below the top round a key counts when it is a masked height and carries the prefix picked so far
        auto counts = [&](unsigned key) { return key != 0xFFFFFFFFu && (key >> (shift + 8)) == want; };
        if (shift < 24 && count <= (unsigned)lds_keys) {                     // the list holds every masked key of the frame
            for (unsigned i = tid; i < count; i += kMedianThreads) {
                const unsigned key = list[i];
                median_hist_add(hist, key, (key >> (shift + 8)) == want, shift, lane);
            }
        } else if (vec) {
            const uint4 *kp4 = reinterpret_cast<const uint4 *>(kp);
            const int nv = hw >> 2;
            for (int base = 0; base < nv; base += kMedianThreads * kMedianUnroll) {
                uint4 q[kMedianUnroll];
#pragma unroll
                for (int j = 0; j < kMedianUnroll; j++) {
                    const int i = base + j * kMedianThreads + tid;
                    q[j] = i < nv ? kp4[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                }
#pragma unroll
                for (int j = 0; j < kMedianUnroll; j++) {
                    if (shift == 24) {
                        median_first_add(hist, list, &s_list_n, lds_keys, q[j].x, lane); median_first_add(hist, list, &s_list_n, lds_keys, q[j].y, lane);
                        median_first_add(hist, list, &s_list_n, lds_keys, q[j].z, lane); median_first_add(hist, list, &s_list_n, lds_keys, q[j].w, lane);
                    } else {
                        median_hist_add(hist, q[j].x, counts(q[j].x), shift, lane); median_hist_add(hist, q[j].y, counts(q[j].y), shift, lane);
                        median_hist_add(hist, q[j].z, counts(q[j].z), shift, lane); median_hist_add(hist, q[j].w, counts(q[j].w), shift, lane);
                    }
                }
            }
        } else {
            for (int base = 0; base < hw; base += kMedianThreads * kMedianUnroll) {
                unsigned key[kMedianUnroll];
#pragma unroll
                for (int j = 0; j < kMedianUnroll; j++) {
                    const int i = base + j * kMedianThreads + tid;
                    key[j] = i < hw ? kp[i] : 0xFFFFFFFFu;
                }
#pragma unroll
                for (int j = 0; j < kMedianUnroll; j++) {
                    if (shift == 24) median_first_add(hist, list, &s_list_n, lds_keys, key[j], lane);
                    else median_hist_add(hist, key[j], counts(key[j]), shift, lane);
                }
            }
        }
        __syncthreads();
        // pick: inclusive prefix sum of the bins (Hillis-Steele, two buffers); the bin whose running count first exceeds k holds rank k
        if (tid < 256) scan[0][tid] = hist[tid];
        __syncthreads();
        int cur = 0;
        for (int o = 1; o < 256; o <<= 1) {
            if (tid < 256) scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= o ? scan[cur][tid - o] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        if (shift == 24) {
            count = scan[cur][255];                                          // = s_list_n: every masked key was counted and listed once
            if (count == 0) {                                                // (uniform over the workgroup) no ground: what k_sel_pick writes
                if (tid == 0) {
                    const float med = __uint_as_float(0x7FC00000u);
                    if (median_out) median_out[n] = med;
                    scale_out[n] = real_cam_height / med;
                    if (count_out) count_out[n] = 0;
                }
                return;
            }
            k = (count - 1) / 2;                                             // torch.median: lower median
        }
        if (tid < 256) {
            const unsigned incl = scan[cur][tid], excl = incl - hist[tid];
            if (excl <= k && k < incl) { s_k = k - excl; s_prefix = prefix | ((unsigned)tid << shift); }      // exactly one bin
        }
        __syncthreads();
        k = s_k; prefix = s_prefix;
    }
    if (tid == 0) {
        const float med = __uint_as_float(prefix);
        if (median_out) median_out[n] = med;
        scale_out[n] = real_cam_height / med;                                // dnet_layers.py:325
        if (count_out) count_out[n] = (int)count;
    }
}

}  // namespace tc
