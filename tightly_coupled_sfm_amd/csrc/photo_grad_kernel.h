// photo_grad_kernel.h -- backward pass of the residual assembly behind tcsfm_photometric (train_mono.py:84-92, helpers.py:8-23, under
// autograd): gfx950 device code.
//
//   diff   = mean_c( w_l1 clamp(|y - x|, 0, 1) + w_ssim clamp((1 - SSIM(x, y)) / 2, 0, 1) ),   x = tgt, y = img_rec
//   weight = 1 - clamp(|cd - pd| / (cd + pd), 0, 1)
//
// Inputs per item: x, y [3,H,W], pd, cd [1,H,W] and the cotangents g_diff, g_weight [1,H,W] (each may be null = zero); outputs g_rec
// [3,H,W], g_pd, g_cd [1,H,W] (each may be null = not wanted).  torch's conventions at the kinks: sgn(0) = 0 and a clamp passes its
// gradient on the CLOSED interval (|y - x| = 1 at a saturated target over an out-of-frame sample and |r| = 1 at pd = 0 do occur).
//
// k_photo_bwd is a gather: one thread per pixel p of a PG_TW x PG_TH tile sums over the (at most nine) windows q that contain p, in
// one fixed order -- no atomics, bit-reproducible.  x and y are staged with a halo of 2 (through refl_idx, so the halo IS the
// ReflectionPad2d of losses.py:22); then per window q of the tile + a halo of 1 and per channel the three coefficients of
//     g_diff[q] (w_ssim / 3) (-1/2) d s_q / d y_p  =  A_q + B_q (y_p - y_q) + C_q (x_p - x_q)
// go to LDS (zero for a window outside the frame, outside the SSIM clamp or with a zero cotangent); then the 3 x 3 gather with the
// reflect multiplicity m(q, p) = how many of q's nine taps land on p (separable; 1 inside, 2 or 4 next to a border).  The statistics
// are k_ssim's shifted ones (differences to the window's centre pixel) and the coefficients are kept relative to that centre too, so
// fp32 does not cancel.  With A1 = 2 mux muy + C1, A2 = 2 sxy + C2, B1 = mux^2 + muy^2 + C1, B2 = sx + sy + C2, s = A1 A2 / (B1 B2):
//     d s_q / d y_p = (1/9) [ (2 mux A2 + 2 (x_p - mux) A1) / (B1 B2) - s (2 muy / B1 + 2 (y_p - muy) / B2) ].
#pragma once
#include "kernels.h"
#include "warp_grad_kernel.h"

namespace tc {

// The warp forward of the chain (tcsfm_photometric_backward): img_rec, proj_depth and comp_depth as k_warp_bwd sees them -- the bilinear
// cell, the sentinel and the Z clamp are k_warp's fp32 decisions, the values are evaluated in fp64 from the pair's fp64 intrinsics and
// transform and rounded once.  k_warp's own fp32 values carry several roundings of a coordinate of order W; the SSIM term (1 / (sx + sy
// + C2) in flat regions) and the depth-consistency term next to the clamp amplify them beyond what fp32 autograd shows.
struct WarpFwd64Params {
    const float *src, *depth_t, *depth_s;
    const PairConst *pc;
    const PairState *st;
    float *rec, *pd, *cd;               // each may be null
    int H, W;
};
__device__ __forceinline__ double warp_cell_sample(const float *__restrict__ img, int W, const WarpCell &t, double wx, double wy) {
    const double v00 = t.m00 ? (double)img[t.y0 * W + t.x0] : 0.0, v01 = t.m01 ? (double)img[t.y0 * W + t.x1] : 0.0;
    const double v10 = t.m10 ? (double)img[t.y1 * W + t.x0] : 0.0, v11 = t.m11 ? (double)img[t.y1 * W + t.x1] : 0.0;
    return (1.0 - wx) * (1.0 - wy) * v00 + wx * (1.0 - wy) * v01 + (1.0 - wx) * wy * v10 + wx * wy * v11;
}
__global__ __launch_bounds__(256) void k_warp_fwd64(WarpFwd64Params P) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    const int hw = P.H * P.W;
    if (idx >= hw) return;
    const int v = idx / P.W, u = idx - v * P.W;
    const float dep = P.depth_t[(size_t)n * hw + idx];
    Geo g;
    warp_geo(P.pc[n], P.W, P.H, u, v, dep, g);
    const bool oob = g.oobx || g.ooby;
    const PairState &S = P.st[n];
    const double fx = S.K[0], fy = S.K[4], cx = S.K[2], cy = S.K[5];
    const double *T = S.Tcur;
    const double D = (double)dep, c0 = ((double)u - cx) / fx * D, c1 = ((double)v - cy) / fy * D;
    const double X0 = T[0] * c0 + T[1] * c1 + T[2] * D + T[3];
    const double X1 = T[4] * c0 + T[5] * c1 + T[6] * D + T[7];
    const double X2 = T[8] * c0 + T[9] * c1 + T[10] * D + T[11];
    const double Z = g.zcl ? 1e-3 : X2, iz = 1.0 / Z;
    const double xp = (fx * X0 + cx * X2) * iz, yp = (fy * X1 + cy * X2) * iz;
    const double sx = (double)P.W / (double)(P.W - 1), sy = (double)P.H / (double)(P.H - 1);
    WarpCell t;
    warp_cell(P.W, P.H, u, v, g.rx, g.ry, oob, t);          // (out of range: every tap masked -> zeros, as tap1)
    const double wx = (xp * sx - 0.5) - (double)t.xi, wy = (yp * sy - 0.5) - (double)t.yi;
    if (P.rec)
        for (int ch = 0; ch < 3; ch++)
            P.rec[((size_t)n * 3 + ch) * hw + idx] = oob ? 0.f : (float)warp_cell_sample(P.src + ((size_t)n * 3 + ch) * hw, P.W, t, wx, wy);
    if (P.pd) P.pd[(size_t)n * hw + idx] = oob ? 0.f : (float)warp_cell_sample(P.depth_s + (size_t)n * hw, P.W, t, wx, wy);
    if (P.cd) P.cd[(size_t)n * hw + idx] = (float)Z;
}

constexpr int PG_TW = 32, PG_TH = 8;                                            // the tile: 256 threads, one per pixel
constexpr int PG_XW = PG_TW + 4, PG_XH = PG_TH + 4, PG_XN = PG_XW * PG_XH;      // x, y planes: tile + halo 2
constexpr int PG_CW = PG_TW + 2, PG_CH = PG_TH + 2, PG_CN = PG_CW * PG_CH;      // window coefficients: tile + halo 1

struct PhotoGradParams {
    const float *tgt, *rec, *pd, *cd;
    const float *g_diff, *g_weight;     // cotangents, each may be null (= zero)
    const float *g_rec_add;             // optional [N,3,H,W], added to g_rec (a cotangent that reaches img_rec directly)
    float *g_rec, *g_pd, *g_cd;         // each may be null (= not wanted)
    int H, W;
    float wl, ws;                       // w_l1 / 3, w_ssim / 3
};

// the coefficients of one window and channel from its nine reflected taps; k = g_diff[q] (w_ssim / 3) (-1/2).  T = float; double is
// the fallback the warp's backward took, not needed here.
template <typename T>
__device__ __forceinline__ void photo_window_coef(const float *xv, const float *yv, T k, float &A, float &B, float &C) {
    const T x0 = (T)xv[4], y0 = (T)yv[4];
    T sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const T a = (T)xv[i] - x0, b = (T)yv[i] - y0;      // shifted by the centre value, as k_ssim
        sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
    }
    const T n9 = (T)1 / (T)9;
    const T mdx = sx * n9, mdy = sy * n9, mux = x0 + mdx, muy = y0 + mdy;
    const T sigx = sxx * n9 - mdx * mdx, sigy = syy * n9 - mdy * mdy, sigxy = sxy * n9 - mdx * mdy;
    const T A1 = (T)2 * mux * muy + (T)SSIM_C1, A2 = (T)2 * sigxy + (T)SSIM_C2;
    const T B1 = mux * mux + muy * muy + (T)SSIM_C1, B2 = sigx + sigy + (T)SSIM_C2;
    const T iB1 = (T)1 / B1, iB2 = (T)1 / B2, s = A1 * A2 * iB1 * iB2;
    const T v = ((T)1 - s) * (T)0.5;
    A = B = C = 0.f;
    if (!(v >= (T)0 && v <= (T)1)) return;                 // outside the clamp of losses.py:41 (closed interval: the ends pass)
    const T kk = k * n9 * (T)2;
    A = (float)(kk * ((mux * A2 - mdx * A1) * iB1 * iB2 - s * (muy * iB1 - mdy * iB2)));
    B = (float)(-kk * s * iB2);
    C = (float)(kk * A1 * iB1 * iB2);
}

// how many of the three reflected taps q - 1, q, q + 1 of an in-frame q land on p (one axis)
__device__ __forceinline__ int photo_refl_mult(int q, int p, int n) {
    return (refl_idx(q - 1, n) == p) + (q == p) + (refl_idx(q + 1, n) == p);
}

__global__ __launch_bounds__(256) void k_photo_bwd(PhotoGradParams P) {
    __shared__ float xy[6][PG_XN];
    __shared__ float co[9][PG_CN];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int H = P.H, W = P.W, hw = H * W;
    const int x00 = blockIdx.x * PG_TW, y00 = blockIdx.y * PG_TH;
    const int tx = tid % PG_TW, ty = tid / PG_TW;
    const int px = x00 + tx, py = y00 + ty;
    const bool inimg = px < W && py < H;               // (a ragged tile: the thread still stages and meets the barriers)
    const int gi = py * W + px;
    if (P.g_rec != nullptr && P.g_diff != nullptr) {    // (uniform over the launch)
        const float *x = P.tgt + (size_t)n * 3 * hw, *y = P.rec + (size_t)n * 3 * hw;
        const float *gd = P.g_diff + (size_t)n * hw;
        for (int e = tid; e < PG_XN; e += 256) {
            const int ly = e / PG_XW, lx = e - ly * PG_XW;
            const int j = refl_idx(y00 + ly - 2, H) * W + refl_idx(x00 + lx - 2, W);      // always inside the frame
#pragma unroll
            for (int c = 0; c < 3; c++) { xy[c][e] = x[c * hw + j]; xy[3 + c][e] = y[c * hw + j]; }
        }
        __syncthreads();
        for (int e = tid; e < PG_CN; e += 256) {
            const int ly = e / PG_CW, lx = e - ly * PG_CW;
            const int qx = x00 + lx - 1, qy = y00 + ly - 1;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const float g = in ? gd[qy * W + qx] : 0.f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float A = 0.f, B = 0.f, C = 0.f;
                if (g != 0.f) {
                    float xv[9], yv[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) {
                        const int t = (ly + i / 3) * PG_XW + lx + (i % 3);      // window q's taps: rows ly .. ly + 2 of the halo-2 tile
                        xv[i] = xy[c][t]; yv[i] = xy[3 + c][t];
                    }
                    photo_window_coef<float>(xv, yv, g * P.ws * -0.5f, A, B, C);
                }
                co[3 * c][e] = A; co[3 * c + 1][e] = B; co[3 * c + 2][e] = C;
            }
        }
        __syncthreads();
        if (inimg) {
            const int pc = (ty + 2) * PG_XW + tx + 2;
            float xp[3], yp[3], acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; c++) { xp[c] = xy[c][pc]; yp[c] = xy[3 + c][pc]; }
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int qy = py + dy;
                if (qy < 0 || qy >= H) continue;
                const int my = photo_refl_mult(qy, py, H);
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = px + dx;
                    if (qx < 0 || qx >= W) continue;
                    const float m = (float)(my * photo_refl_mult(qx, px, W));
                    const int eq = (ty + 1 + dy) * PG_CW + tx + 1 + dx, ex = (ty + 2 + dy) * PG_XW + tx + 2 + dx;
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        acc[c] += m * (co[3 * c][eq] + co[3 * c + 1][eq] * (yp[c] - xy[3 + c][ex]) + co[3 * c + 2][eq] * (xp[c] - xy[c][ex]));
                }
            }
            const float gp = gd[gi] * P.wl;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = yp[c] - xp[c];
                const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);                     // sgn(0) = 0
                float r = acc[c] + (fabsf(d) <= 1.f ? gp * sg : 0.f);                        // clamp(0, 1): closed interval
                const size_t o = ((size_t)n * 3 + c) * hw + gi;
                if (P.g_rec_add != nullptr) r += P.g_rec_add[o];
                P.g_rec[o] = r;
            }
        }
    }
    if (inimg && P.g_weight != nullptr && (P.g_pd != nullptr || P.g_cd != nullptr)) {
        const size_t o = (size_t)n * hw + gi;
        const float pd = P.pd[o], cd = P.cd[o], gw = P.g_weight[o];
        // a handful of fp64 operations per pixel, rounded once: fp32 autograd knows these two to 3e-8 and the bound is 4 times that
        const double sum = (double)cd + (double)pd, dif = (double)cd - (double)pd;
        const double sg = dif > 0.0 ? 1.0 : (dif < 0.0 ? -1.0 : 0.0);
        const double t = fabs(dif) / sum;
        const double k = (t >= 0.0 && t <= 1.0) ? (double)gw * sg * 2.0 / (sum * sum) : 0.0;  // pd = 0 (out of frame): t = 1 exactly, passes
        if (P.g_pd != nullptr) P.g_pd[o] = (float)(k * (double)cd);
        if (P.g_cd != nullptr) P.g_cd[o] = (float)(-k * (double)pd);
    }
}

}  // namespace tc
