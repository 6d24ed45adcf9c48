// The flip post-processing of helpers.get_disp_for_eigen (optimization_experiments/helpers.py:35-49) on the device:
//   k_dn_head<MODE>: the depth network's head (depthnet_kernel.h k_dn_predict's own dn_head_disp) with the stores the sequence
//                    calls' disparity stage needs -- depth AND scaled disparity, or the scaled disparity alone;
//   k_disp_post<VEC>: batch_post_process_disparity (utils/learning_helpers.py:115-123) of the straight and the mirrored pass, float64 out;
//   flip_ramp.h:      its l_mask, on the host, in NumPy's own operations.
// The blend follows the reference's expression and order exactly -- every float64 operation rounded on its own, nothing contracted --
// so its result is comparable with NumPy's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "depthnet_kernel.h"
#include "flip_ramp.h"

namespace tc {

// ---------------------------------------------------------------------------------------------------------------
// What the head stores per pixel.  DN_HEAD_DEPTH_SCALED: disp_depth into `out`, disp_scaled into `out2` (two stores per thread);
// DN_HEAD_SCALED: disp_scaled into `out`.  disp_scaled is kernels.h' expression, the one k_disp_to_depth stores as scaled_disp: the bits
// of tcsfm_depthnet_forward followed by tcsfm_disp_to_depth.  k_dn_predict<false> / <true> stay as they are (disparity / depth alone).
enum { DN_HEAD_DEPTH_SCALED = 0, DN_HEAD_SCALED = 1 };

template <int MODE>
__global__ __launch_bounds__(256) void k_dn_head(const float *in, const float *w, const float *bias, float *out, float *out2, int N, int H,
                                                 int W, float min_disp, float max_disp) {
    const long long total = (long long)N * H * W;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float disp = dn_head_disp(in, w, bias, e, H, W);
    if (MODE == DN_HEAD_DEPTH_SCALED) {
        out[e] = disp_depth(disp, min_disp, max_disp);
        out2[e] = disp_scaled(disp, min_disp, max_disp);
    } else {
        out[e] = disp_scaled(disp, min_disp, max_disp);
    }
}

// one pixel of the blend:  r_mask * l + l_mask * r + (1.0 - l_mask - r_mask) * m,  m = float32(0.5 * (l + r)), left to right as NumPy
// evaluates it on float32 planes and a float64 ramp
__device__ __forceinline__ double disp_post_pixel(float l, float r, double lm, double rm) {
#pragma clang fp contract(off)
    const float sum = l + r;
    const float m = 0.5f * sum;
    const double a = rm * (double)l;
    const double b = lm * (double)r;
    const double ab = a + b;
    const double w0 = 1.0 - lm;
    const double w1 = w0 - rm;
    const double c = w1 * (double)m;
    return ab + c;
}

// l [n][H][W]: scaled disparity of the frames; rf [n][H][W]: of the mirrored frames, still mirrored (pixel x of the frame is rf's
// W - 1 - x); l_mask [W] doubles; out [n][H][W] float64.  Memory-bound and element-wise: a thread owns two neighbouring pixels of a row.
// VEC (W even, l and rf 8-byte aligned, out 16-byte aligned): one 8-byte load of l, one of rf -- lane i's pair sits 8 bytes BELOW lane
// i - 1's, so a wave still reads one contiguous run of the row -- and one 16-byte store: whole lines in and out.  Otherwise the same
// pixels with scalar accesses (odd W: a row's last thread owns one pixel).  rows = n * H.
template <bool VEC>
__global__ __launch_bounds__(256) void k_disp_post(const float *__restrict__ l, const float *__restrict__ rf, const double *__restrict__ l_mask,
                                                   double *__restrict__ out, long long rows, int W) {
    const int P = (W + 1) / 2;                                   // pairs per row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * P) return;
    const long long row = t / P;
    const int x0 = 2 * (int)(t - row * P), x1 = x0 + 1;
    const size_t base = (size_t)row * W;
    if (VEC) {
        const float2 lv = *reinterpret_cast<const float2 *>(l + base + x0);
        const float2 rv = *reinterpret_cast<const float2 *>(rf + base + (W - 2 - x0));      // (rf[W-1-x1], rf[W-1-x0])
        double2 o;
        o.x = disp_post_pixel(lv.x, rv.y, l_mask[x0], l_mask[W - 1 - x0]);
        o.y = disp_post_pixel(lv.y, rv.x, l_mask[x1], l_mask[W - 1 - x1]);
        *reinterpret_cast<double2 *>(out + base + x0) = o;
    } else {
        out[base + x0] = disp_post_pixel(l[base + x0], rf[base + W - 1 - x0], l_mask[x0], l_mask[W - 1 - x0]);
        if (x1 < W) out[base + x1] = disp_post_pixel(l[base + x1], rf[base + W - 1 - x1], l_mask[x1], l_mask[W - 1 - x1]);
    }
}

}  // namespace tc
