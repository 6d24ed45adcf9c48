// Host side of the 8-bit Lanczos resize (resize_u8_kernel.h; include/tcsfm.h: tcsfm_resize_coeffs, tcsfm_scale_intrinsics): the
// coefficient table of Pillow's Image.resize(..., LANCZOS) on 8-bit images, and the loaders' intrinsics scaling.  Pure C++, no HIP: the
// CPU tests and tests/asan/resize_host.cpp build it alone.
//
// One axis, input length `in` -> output length `out` (the reference's loaders: data/scannet_test_loader.py:157-170,
// data/create_kitti_odometry_data.py:56-65):
//   scale = in / out;  fs = max(scale, 1);  support = 3 fs;  ksize = (int)ceil(support) * 2 + 1
//   output xx:  center = (xx + 0.5) scale;  xmin = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - xmin
//               w[x] = lanczos((x + xmin - center + 0.5) / fs), normalised by their sum (added in order), then 22-bit fixed point, rounded
//               half away from zero.  Everything in double: the table is a function of (in, out) alone, equal on every host.
#pragma once
#include <math.h>
#include <stddef.h>
#include <vector>

namespace tc {

static inline int resize_ksize(int in, int out) {
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(3.0 * fs) * 2 + 1;
}

static inline double resize_sinc(double t) {
    if (t == 0.0) return 1.0;
    t *= M_PI;
    return sin(t) / t;
}

static inline double resize_lanczos(double t) { return (-3.0 <= t && t < 3.0) ? resize_sinc(t) * resize_sinc(t / 3.0) : 0.0; }

// bounds[out][2] = {xmin, n}, kk[out][ksize] (entries beyond n are 0); both may be NULL (then only ksize is returned).  in, out >= 1.
static inline int resize_coeffs(int in, int out, int *bounds, int *kk) {
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale, support = 3.0 * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!bounds || !kk) return ksize;
    std::vector<double> w((size_t)ksize);
    double *wp = w.data();
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            wp[x] = resize_lanczos((x + xmin - center + 0.5) / fs);
            ww += wp[x];
        }
        int *k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            if (x >= n) { k[x] = 0; continue; }
            const double v = ww != 0.0 ? wp[x] / ww : wp[x];
            k[x] = (int)(v < 0 ? -0.5 + v * 4194304.0 : 0.5 + v * 4194304.0);      // 1 << 22
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    return ksize;
}

// K of the src_h x src_w camera image -> K of the H x W image the networks read: row 0 times W / src_w, row 1 times H / src_h, in
// double, rounded to float once (the loaders' K[0] *= zoom_x; K[1] *= zoom_y on a float64 K); row 2 is copied.  K_out may be K_src.
static inline void scale_intrinsics(int src_h, int src_w, int H, int W, const float *K_src, float *K_out) {
    const double zx = (double)W / (double)src_w, zy = (double)H / (double)src_h;
    for (int i = 0; i < 3; i++) {
        const float a = K_src[i], b = K_src[3 + i], c = K_src[6 + i];
        K_out[i] = (float)((double)a * zx);
        K_out[3 + i] = (float)((double)b * zy);
        K_out[6 + i] = c;
    }
}

}  // namespace tc
