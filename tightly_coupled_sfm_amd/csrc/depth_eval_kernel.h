// depth_eval_kernel.h -- the Eigen depth evaluation of paper_plots_and_data/evaluate_depth_eigen.py:133-168 on the device.
//   k_depth_eval<T>  one workgroup per frame (grid.x = N): disparity plane [H][W] of T (float promoted to double, exact) against float32
//              ground truth [gt_h][gt_w] -> TCSFM_NEVAL doubles: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, n_valid, n_median.
//   A masked pixel's prediction is depth_unit / (the bilinear resize of the plane at that pixel): four taps of a plane that stays in
//   cache, float32 coefficients promoted to double, the horizontal pass first, every double operation rounded on its own (contraction
//   off, as k_disp_post) -- the arithmetic of tests/depth_eval_inputs.py, comparable with NumPy's bit for bit.  No resized plane is
//   written anywhere.
//   Passes over the frame's masked pixels (all inside the launch, nothing crosses workgroups):
//     0        count the mask and the median subset (gt < max_depth), append the masked pixels' indices to a list in LDS;
//     1 .. 4   exact select of the median subset's float32 ground truth, MSB first, 8 bits a round;
//     5 .. 12  the same over the float64 predictions (all keys are positive: the bit patterns order like the values);
//     13       the four sums and the three threshold counts, on the median-scaled, clipped predictions.
//   A select round is a 256-bin histogram in LDS with INTEGER atomics (frame_scale_kernel.h's median_hist_add: one atomic per wave for
//   the bin most lanes share) and a parallel prefix sum; the counts do not depend on the order of the adds.  Both middle ranks of an even
//   count are followed at once: while they share their prefix one histogram serves both, after they part each prefix has its own.
//   The list: KITTI's ground truth is sparse (about 5 % of 375 x 1242 survive crop and range test: 23 000 pixels), so passes 1 .. 12 walk
//   the list -- a 4-byte pixel index per masked pixel, each standing for one (gt, pred) pair: gt is gathered from the plane (cache), pred
//   recomputed from its four taps -- instead of the plane.  A frame with more masked pixels than the list holds (lds_pairs, at most
//   kEvalLdsPairs) scans its crop again in every pass: the same counts, hence the same bits.  The list's order depends on the order of
//   the appends; it feeds the histograms only.
//   Pass 13 always scans the crop in pixel order, so that a thread adds its pixels (index = tid mod 1024) in increasing order whatever
//   the list held: doubles, per thread, then over the wave (xor 32 .. 1), then over the waves in order.  No floating-point atomics;
//   the results are bit-reproducible and do not depend on lds_pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frame_scale_kernel.h"

namespace tc {

constexpr int kEvalThreads = 1024, kEvalWaves = kEvalThreads / 64, kEvalUnroll = 4;
constexpr int kEvalLdsPairs = 36864;         // 144 KB of the CU's 160 KB: 7.9 % of a 375 x 1242 frame
constexpr int kEvalOut = 10;                 // TCSFM_NEVAL

struct DepthEvalArgs {
    int H, W, gt_h, gt_w;
    int y0, y1, x0, x1;                      // the pixels the protocol looks at (the Eigen crop, or the whole plane)
    int benchmark, median_scaling, lds_pairs, pad;
    float min_f, max_f;                      // the mask's bounds, compared in float32
    double min_d, max_d;                     // the clip's: the same values promoted
    double depth_unit, scale_x, scale_y;     // scale = 1.0 / (n_dst / n_src), taken on the host
};

// one axis of the resize at output index d: tap indices s, s1 and the float32 weights w0, w1 (cv::resize INTER_LINEAR's coefficients)
__device__ __forceinline__ void eval_axis(int d, double scale, int n_src, int &s, int &s1, float &w0, float &w1) {
#pragma clang fp contract(off)
    const double t = (double)d + 0.5;
    const double u = t * scale;
    const double v = u - 0.5;
    float f = (float)v;                      // computed in double, rounded once
    const float fl = floorf(f);
    f = f - fl;
    s = (int)fl;
    if (fl < 0.f) { s = 0; f = 0.f; }
    if (fl >= (float)(n_src - 1)) { s = n_src - 1; f = 0.f; }
    s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    w0 = 1.f - f;
    w1 = f;
}

// depth_unit / (the resized plane at (y, x))
template <typename T>
__device__ __forceinline__ double eval_pred(const T *__restrict__ P, const DepthEvalArgs &a, int y, int x) {
#pragma clang fp contract(off)
    int sx, sx1, sy, sy1;
    float w0, w1, b0, b1;
    eval_axis(x, a.scale_x, a.W, sx, sx1, w0, w1);
    eval_axis(y, a.scale_y, a.H, sy, sy1, b0, b1);
    const T *r0 = P + (size_t)sy * a.W, *r1 = P + (size_t)sy1 * a.W;
    const double m00 = (double)r0[sx] * (double)w0;
    const double m01 = (double)r0[sx1] * (double)w1;
    const double top = m00 + m01;
    const double m10 = (double)r1[sx] * (double)w0;
    const double m11 = (double)r1[sx1] * (double)w1;
    const double bot = m10 + m11;
    const double v0 = top * (double)b0;
    const double v1 = bot * (double)b1;
    const double out = v0 + v1;
    return a.depth_unit / out;
}

__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kEvalThreads) void k_depth_eval(const T *__restrict__ disp, const float *__restrict__ gt, DepthEvalArgs a,
                                                             double *__restrict__ out) {
    __shared__ unsigned list[kEvalLdsPairs];
    __shared__ unsigned hist[2][256], scan[2][512];
    __shared__ double red[kEvalWaves][4];
    __shared__ unsigned long long s_prefix[2];
    __shared__ unsigned s_k[2], s_cnt[5];                        // s_cnt: n_valid, n_median, a1, a2, a3
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const T *P = disp + (size_t)n * a.H * a.W;
    const float *G = gt + (size_t)n * a.gt_h * a.gt_w;
    double *o = out + (size_t)n * kEvalOut;
    const unsigned rw = (unsigned)(a.x1 - a.x0), total = rw * (unsigned)(a.y1 - a.y0);
    const unsigned cap = (unsigned)(a.lds_pairs < 0 ? 0 : (a.lds_pairs > kEvalLdsPairs ? kEvalLdsPairs : a.lds_pairs));
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    auto masked = [&](float g) { return a.benchmark ? g > 0.f : (g > a.min_f && g < a.max_f); };
    // fn(idx, g) for every masked pixel of the crop, in pixel order per thread
    // (kEvalUnroll loads in flight per thread: one workgroup reads the plane, and a loop of dependent loads would wait out the memory's
    // latency once per pixel; a pixel past the crop's end reads as a hole)
    auto scan_crop = [&](auto &&fn) {
        for (unsigned base = 0; base < total; base += kEvalThreads * kEvalUnroll) {
            unsigned idx[kEvalUnroll];
            float g[kEvalUnroll];
#pragma unroll
            for (int j = 0; j < kEvalUnroll; j++) {
                const unsigned i = base + (unsigned)j * kEvalThreads + (unsigned)tid, r = i / rw;
                idx[j] = ((unsigned)a.y0 + r) * (unsigned)a.gt_w + (unsigned)a.x0 + (i - r * rw);
                g[j] = i < total ? G[idx[j]] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < kEvalUnroll; j++)
                if (masked(g[j])) fn(idx[j], g[j]);
        }
    };

    // ---- pass 0: the counts and the list
    if (tid < 5) s_cnt[tid] = 0;
    __syncthreads();
    scan_crop([&](unsigned idx, float g) {
        const unsigned long long mine = __ballot(true);                               // the masked lanes of this wave
        const unsigned long long sub = __ballot(g < a.max_f);                         // ... of the median subset
        unsigned at = 0;
        if (lane == __ffsll((long long)mine) - 1) {
            at = atomicAdd(&s_cnt[0], (unsigned)__popcll(mine));
            if (sub) atomicAdd(&s_cnt[1], (unsigned)__popcll(sub));
        }
        at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);                        // (the first masked lane is the one that added)
        const unsigned pos = at + (unsigned)__popcll(mine & ((1ull << lane) - 1ull));
        if (pos < cap) list[pos] = idx;
    });
    __syncthreads();
    const unsigned n_valid = s_cnt[0], n_med = s_cnt[1];
    const bool use_list = n_valid <= cap;                                             // (uniform) the list holds every masked pixel
    if (n_valid == 0 || (a.median_scaling && n_med == 0)) {                            // (uniform)
        if (tid < 7) o[tid] = nan;
        if (tid == 7) { o[7] = a.median_scaling ? nan : 1.0; o[8] = (double)n_valid; o[9] = (double)n_med; }
        return;
    }
    auto each = [&](auto &&fn) {
        if (use_list) {
            for (unsigned base = 0; base < n_valid; base += kEvalThreads * kEvalUnroll) {
                unsigned idx[kEvalUnroll];
                float g[kEvalUnroll];
#pragma unroll
                for (int j = 0; j < kEvalUnroll; j++) {
                    const unsigned i = base + (unsigned)j * kEvalThreads + (unsigned)tid;
                    idx[j] = i < n_valid ? list[i] : 0u;
                    g[j] = i < n_valid ? G[idx[j]] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < kEvalUnroll; j++)
                    if (masked(g[j])) fn(idx[j], g[j]);                               // (a listed pixel is masked)
            }
        } else {
            scan_crop(fn);
        }
    };
    auto pred_at = [&](unsigned idx) { const unsigned y = idx / (unsigned)a.gt_w; return eval_pred(P, a, (int)y, (int)(idx - y * (unsigned)a.gt_w)); };

    // ---- passes 1 .. 12: ranks (n_med - 1) / 2 and n_med / 2 of the subset's keys, bits [nbits - 1, 0], 8 a round
    auto select = [&](auto &&key, int nbits, unsigned long long &ra, unsigned long long &rb) {
        unsigned long long pa = 0, pb = 0;
        unsigned ka = (n_med - 1) / 2, kb = n_med / 2;
        for (int shift = nbits - 8; shift >= 0; shift -= 8) {
            if (tid < 512) hist[tid >> 8][tid & 255] = 0;
            __syncthreads();
            const bool top = shift == nbits - 8, split = pa != pb;                   // (uniform)
            const unsigned long long wa = top ? 0ull : pa >> (shift + 8), wb = top ? 0ull : pb >> (shift + 8);
            each([&](unsigned idx, float g) {
                if (!(g < a.max_f)) return;
                const unsigned long long k = key(idx, g);
                const unsigned long long hi = top ? 0ull : k >> (shift + 8);
                const unsigned bin = (unsigned)(k >> shift) & 255u;
                median_hist_add(hist[0], bin, hi == wa, 0, lane);
                if (split) median_hist_add(hist[1], bin, hi == wb, 0, lane);
            });
            __syncthreads();
            // pick: inclusive prefix sums of the bins (Hillis-Steele), threads 0 .. 255 for the lower rank, 256 .. 511 for the upper one
            const unsigned b = tid & 255, which = (unsigned)tid >> 8;
            unsigned mine = 0;
            if (tid < 512) { mine = hist[which && split ? 1 : 0][b]; scan[0][tid] = mine; }
            __syncthreads();
            int cur = 0;
            for (int s = 1; s < 256; s <<= 1) {
                if (tid < 512) scan[cur ^ 1][tid] = scan[cur][tid] + (b >= (unsigned)s ? scan[cur][tid - s] : 0u);
                cur ^= 1;
                __syncthreads();
            }
            if (tid < 512) {
                const unsigned incl = scan[cur][tid], excl = incl - mine, k = which ? kb : ka;
                if (excl <= k && k < incl) { s_k[which] = k - excl; s_prefix[which] = (which ? pb : pa) | ((unsigned long long)b << shift); }   // one bin each
            }
            __syncthreads();
            ka = s_k[0]; kb = s_k[1]; pa = s_prefix[0]; pb = s_prefix[1];
        }
        ra = pa; rb = pb;
    };
    double ratio = 1.0;
    if (a.median_scaling) {
#pragma clang fp contract(off)
        unsigned long long ga, gb, qa, qb;
        select([&](unsigned, float g) { return (unsigned long long)__float_as_uint(g); }, 32, ga, gb);
        select([&](unsigned idx, float) { return (unsigned long long)__double_as_longlong(pred_at(idx)); }, 64, qa, qb);
        // np.median: the middle element, or the mean of the two middle ones in the array's own dtype
        float med_g = __uint_as_float((unsigned)ga);
        double med_p = __longlong_as_double((long long)qa);
        if ((n_med & 1u) == 0) {
            const float sg = med_g + __uint_as_float((unsigned)gb);
            med_g = sg / 2.f;
            const double sp = med_p + __longlong_as_double((long long)qb);
            med_p = sp / 2.0;
        }
        ratio = (double)med_g / med_p;
    }

    // ---- pass 13: the sums, in pixel order per thread
    double s_abs = 0.0, s_sqrel = 0.0, s_sq = 0.0, s_log = 0.0;
    unsigned c1 = 0, c2 = 0, c3 = 0;
    scan_crop([&](unsigned idx, float gf) {
#pragma clang fp contract(off)
        double p = pred_at(idx);
        if (a.median_scaling) p = p * ratio;
        p = fmin(fmax(p, 0.0), a.max_d);                                              // np.clip(pred, 0, max_depth)
        if (p < a.min_d) p = a.min_d;
        if (p > a.max_d) p = a.max_d;
        const double g = (double)gf;
        const double q0 = g / p, q1 = p / g;
        const double thresh = q0 > q1 ? q0 : q1;
        c1 += thresh < 1.25; c2 += thresh < 1.5625; c3 += thresh < 1.953125;
        const double d = g - p;
        const double d2 = d * d;
        const double l = log(g) - log(p);
        const double l2 = l * l;
        const double ar = fabs(d) / g;
        const double sr = d2 / g;
        s_abs = s_abs + ar; s_sqrel = s_sqrel + sr; s_sq = s_sq + d2; s_log = s_log + l2;
    });
    s_abs = eval_wave_sum(s_abs); s_sqrel = eval_wave_sum(s_sqrel); s_sq = eval_wave_sum(s_sq); s_log = eval_wave_sum(s_log);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { c1 += __shfl_xor(c1, off, 64); c2 += __shfl_xor(c2, off, 64); c3 += __shfl_xor(c3, off, 64); }
    if (lane == 0) {
        double *r = red[tid >> 6];
        r[0] = s_abs; r[1] = s_sqrel; r[2] = s_sq; r[3] = s_log;
        atomicAdd(&s_cnt[2], c1); atomicAdd(&s_cnt[3], c2); atomicAdd(&s_cnt[4], c3);
    }
    __syncthreads();
    if (tid == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < kEvalWaves; w++)
            for (int j = 0; j < 4; j++) t[j] = t[j] + red[w][j];
        const double nv = (double)n_valid;
        o[0] = t[0] / nv; o[1] = t[1] / nv; o[2] = sqrt(t[2] / nv); o[3] = sqrt(t[3] / nv);
        o[4] = (double)s_cnt[2] / nv; o[5] = (double)s_cnt[3] / nv; o[6] = (double)s_cnt[4] / nv;
        o[7] = ratio; o[8] = nv; o[9] = (double)n_med;
    }
}

}  // namespace tc
