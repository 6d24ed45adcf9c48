// loss_grad_kernel.h -- backward passes of the three loss-side drop-ins of the reference's optimisation loop (optimizer.py:217-268 under
// autograd), and the device-side forward of the smoothness loss: gfx950 device code.
//
//   disp_to_depth   (utils/learning_helpers.py:77-86)   s = a + b disp, depth = 1 / s          -> k_disp_to_depth_bwd
//   SSIM_Loss       (losses.py:27-41)                   out = clamp((1 - SSIM(x, y)) / 2, 0, 1) -> k_ssim_bwd (with respect to x and/or y)
//   get_smooth_loss (losses.py:43-61)                   the scalar on the device                -> k_smooth_reduce (after k_smooth_mean, k_smooth)
//                                                       its gradient with respect to disp       -> k_smooth_bwd
//
// torch's conventions at the kinks: sgn(0) = 0 and a clamp passes its gradient on the CLOSED interval.  Every kernel is a gather or
// elementwise: no atomics, one fixed order, bit-reproducible.
#pragma once
#include "kernels.h"
#include "photo_grad_kernel.h"

namespace tc {

// ---------------------------------------------------------------------------------------------------------------
// disp_to_depth:  g_disp = b (g_s - g_depth / s^2),  s recomputed with k_disp_to_depth's own expression.  Thread t < n4 takes the float4
// t, the threads after them one element of the tail each (the host passes n4 = 0 when a pointer is not 16-byte aligned).
__device__ __forceinline__ float disp_to_depth_bwd1(float d, float gs, float gd, float min_disp, float max_disp) {
    const float s = min_disp + (max_disp - min_disp) * d;
    return (max_disp - min_disp) * (gs - gd / (s * s));
}
__global__ __launch_bounds__(256) void k_disp_to_depth_bwd(const float *disp, const float *g_s, const float *g_d, float *g_disp, long long n,
                                                           long long n4, float min_disp, float max_disp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n4) {
        const float4 d = reinterpret_cast<const float4 *>(disp)[t];
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = g_s ? reinterpret_cast<const float4 *>(g_s)[t] : z, b = g_d ? reinterpret_cast<const float4 *>(g_d)[t] : z;
        reinterpret_cast<float4 *>(g_disp)[t] = make_float4(disp_to_depth_bwd1(d.x, a.x, b.x, min_disp, max_disp), disp_to_depth_bwd1(d.y, a.y, b.y, min_disp, max_disp),
                                                            disp_to_depth_bwd1(d.z, a.z, b.z, min_disp, max_disp), disp_to_depth_bwd1(d.w, a.w, b.w, min_disp, max_disp));
        return;
    }
    const long long i = 4 * n4 + (t - n4);
    if (i >= n) return;
    g_disp[i] = disp_to_depth_bwd1(disp[i], g_s ? g_s[i] : 0.f, g_d ? g_d[i] : 0.f, min_disp, max_disp);
}

// ---------------------------------------------------------------------------------------------------------------
// SSIM_Loss: x, y, g_out [planes, H, W] -> g_x and/or g_y.  The tiled gather of k_photo_bwd (its tile, its halos, its reflect
// multiplicity photo_refl_mult), for both sides of one SSIM.  With the window's shifted statistics as in k_ssim and v = (1 - s) / 2,
//     g_out[q] dv_q / dy_p = Ay_q + B_q (y_p - y_q) + C_q (x_p - x_q),      g_out[q] dv_q / dx_p = Ax_q + B_q (x_p - x_q) + C_q (y_p - y_q):
// B = -kk s / B2 and C = kk A1 / (B1 B2) serve both sides, Ay and Ax are each other with x and y exchanged (kk = -g_out[q] / 9).  The
// expressions are photo_window_coef's (copied: that function yields one side only), so the coefficients stay relative to the centre.
struct SsimGradParams {
    const float *x, *y, *g_out;
    float *g_x, *g_y;                   // each may be null (= not wanted), not both
    int H, W;
};

__device__ __forceinline__ void ssim_window_coef(const float *xv, const float *yv, float k, float &Ax, float &Ay, float &B, float &C) {
    const float x0 = xv[4], y0 = yv[4];
    float sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float a = xv[i] - x0, b = yv[i] - y0;        // shifted by the centre value, as k_ssim
        sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
    }
    const float n9 = 1.f / 9.f;
    const float mdx = sx * n9, mdy = sy * n9, mux = x0 + mdx, muy = y0 + mdy;
    const float sigx = sxx * n9 - mdx * mdx, sigy = syy * n9 - mdy * mdy, sigxy = sxy * n9 - mdx * mdy;
    const float A1 = 2.f * mux * muy + SSIM_C1, A2 = 2.f * sigxy + SSIM_C2;
    const float B1 = mux * mux + muy * muy + SSIM_C1, B2 = sigx + sigy + SSIM_C2;
    const float iB1 = 1.f / B1, iB2 = 1.f / B2, s = A1 * A2 * iB1 * iB2;
    const float v = (1.f - s) * 0.5f;
    Ax = Ay = B = C = 0.f;
    if (!(v >= 0.f && v <= 1.f)) return;                   // outside the clamp of losses.py:41 (closed interval: the ends pass)
    const float kk = k * n9 * 2.f;
    Ay = kk * ((mux * A2 - mdx * A1) * iB1 * iB2 - s * (muy * iB1 - mdy * iB2));
    Ax = kk * ((muy * A2 - mdy * A1) * iB1 * iB2 - s * (mux * iB1 - mdx * iB2));
    B = -kk * s * iB2;
    C = kk * A1 * iB1 * iB2;
}

__global__ __launch_bounds__(256) void k_ssim_bwd(SsimGradParams P) {
    __shared__ float xy[2][PG_XN];
    __shared__ float co[4][PG_CN];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int H = P.H, W = P.W, hw = H * W;
    const int x00 = blockIdx.x * PG_TW, y00 = blockIdx.y * PG_TH;
    const int tx = tid % PG_TW, ty = tid / PG_TW;
    const int px = x00 + tx, py = y00 + ty;
    const float *x = P.x + (size_t)plane * hw, *y = P.y + (size_t)plane * hw, *go = P.g_out + (size_t)plane * hw;
    for (int e = tid; e < PG_XN; e += 256) {
        const int ly = e / PG_XW, lx = e - ly * PG_XW;
        const int j = refl_idx(y00 + ly - 2, H) * W + refl_idx(x00 + lx - 2, W);          // always inside the frame
        xy[0][e] = x[j]; xy[1][e] = y[j];
    }
    __syncthreads();
    for (int e = tid; e < PG_CN; e += 256) {
        const int ly = e / PG_CW, lx = e - ly * PG_CW;
        const int qx = x00 + lx - 1, qy = y00 + ly - 1;
        const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
        const float g = in ? go[qy * W + qx] : 0.f;
        float Ax = 0.f, Ay = 0.f, B = 0.f, C = 0.f;
        if (g != 0.f) {
            float xv[9], yv[9];
#pragma unroll
            for (int i = 0; i < 9; i++) {
                const int t = (ly + i / 3) * PG_XW + lx + (i % 3);          // window q's taps: rows ly .. ly + 2 of the halo-2 tile
                xv[i] = xy[0][t]; yv[i] = xy[1][t];
            }
            ssim_window_coef(xv, yv, g * -0.5f, Ax, Ay, B, C);
        }
        co[0][e] = Ax; co[1][e] = Ay; co[2][e] = B; co[3][e] = C;
    }
    __syncthreads();
    if (px >= W || py >= H) return;                         // (a ragged tile: the thread has staged and met the barriers)
    const int pc = (ty + 2) * PG_XW + tx + 2;
    const float xp = xy[0][pc], yp = xy[1][pc];
    float ax = 0.f, ay = 0.f;
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
            const float dxq = xp - xy[0][ex], dyq = yp - xy[1][ex];
            ax += m * (co[0][eq] + co[2][eq] * dxq + co[3][eq] * dyq);
            ay += m * (co[1][eq] + co[2][eq] * dyq + co[3][eq] * dxq);
        }
    }
    const size_t o = (size_t)plane * hw + py * W + px;
    if (P.g_x != nullptr) P.g_x[o] = ax;
    if (P.g_y != nullptr) P.g_y[o] = ay;
}

// ---------------------------------------------------------------------------------------------------------------
// get_smooth_loss on the device.  k_smooth_reduce follows k_smooth_mean and k_smooth (scale_kernel.h): one workgroup turns the nb
// per-workgroup partials of each image into stats[n] = (mean_n, sum_x_n, sum_y_n) and all of them into the scalar
// loss = sum_x / (N H (W - 1)) + sum_y / (N (H - 1) W).  Sums in double, strided per thread, then an LDS tree: one fixed order.
__global__ __launch_bounds__(256) void k_smooth_reduce(const float *partial, const double *mean, int N, int nb, int H, int W, double *stats,
                                                       float *loss) {
    __shared__ double rx[256], ry[256];
    const int tid = threadIdx.x;
    double tx = 0.0, ty = 0.0;                              // (kept by thread 0 only)
    for (int n = 0; n < N; n++) {
        double sx = 0.0, sy = 0.0;
        for (int i = tid; i < nb; i += 256) { sx += (double)partial[((size_t)n * nb + i) * 2]; sy += (double)partial[((size_t)n * nb + i) * 2 + 1]; }
        rx[tid] = sx; ry[tid] = sy; __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) { rx[tid] += rx[tid + o]; ry[tid] += ry[tid + o]; } __syncthreads(); }
        if (tid == 0) {
            stats[3 * n] = mean[n]; stats[3 * n + 1] = rx[0]; stats[3 * n + 2] = ry[0];
            tx += rx[0]; ty += ry[0];
        }
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(tx / ((double)N * H * (W - 1)) + ty / ((double)N * (H - 1) * W));
}

// Its backward.  With n = disp / (mean + 1e-7) the per-pixel part g_n is the signed sum of the (at most four) edge weights exp(-g)
// touching the pixel, over Nx = N H (W - 1) or Ny = N (H - 1) W; the coupling through the mean is the image's own share of the loss,
// l_n = sum_x_n / Nx + sum_y_n / Ny (= sum_j g_n[j] n_j), so   g_disp = g_loss (g_n - l_n / (H W)) / (mean + 1e-7).
// The weights are k_smooth's fp32 expressions.  The sign of an edge is taken from the two disparities themselves (and the sign of the
// normaliser): k_smooth's d0 - d1 inv contracts into one fma, which on two EQUAL disparities returns the rounding error of d0 instead
// of zero -- harmless in the sum, but sgn(0) = 0 must hold here.  The four weights are summed and scaled in fp64 and rounded once: in fp32 the
// per-pixel terms cancel against the mean term and item n of a batch no longer matched a one-item call within 4 float32 ulps.
struct SmoothGradParams {
    const float *disp, *img;
    const double *stats;                // [N,3]: mean, sum_x, sum_y
    const float *g_loss;                // one float
    float *g_disp;
    int H, W, N;
};
__device__ __forceinline__ float smooth_edge_weight(const float *im, int hw, int i, int j) {      // k_smooth's g and its exp, pixels i and j = i + 1 or i + W
    const float g = (fabsf(im[i] - im[j]) + fabsf(im[hw + i] - im[hw + j]) + fabsf(im[2 * hw + i] - im[2 * hw + j])) * (1.f / 3.f);
    return __expf(-g);
}
__device__ __forceinline__ double smooth_sgn(float a) { return a > 0.f ? 1.0 : (a < 0.f ? -1.0 : 0.0); }      // sgn(0) = 0

__global__ __launch_bounds__(256) void k_smooth_bwd(SmoothGradParams P) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, H = P.H, W = P.W, hw = H * W;
    if (idx >= hw) return;
    const int v = idx / W, u = idx - v * W;
    const double mean = P.stats[3 * n], sumx = P.stats[3 * n + 1], sumy = P.stats[3 * n + 2];
    const float *d = P.disp + (size_t)n * hw, *im = P.img + (size_t)n * 3 * hw;
    const double sn = (float)mean + 1e-7f < 0.f ? -1.0 : 1.0;      // the sign of k_smooth's normaliser (positive for any disparity map)
    const float d0 = d[idx];
    double gx = 0.0, gy = 0.0;
    if (u < W - 1) gx += smooth_sgn(d0 - d[idx + 1]) * (double)smooth_edge_weight(im, hw, idx, idx + 1);
    if (u > 0) gx -= smooth_sgn(d[idx - 1] - d0) * (double)smooth_edge_weight(im, hw, idx - 1, idx);
    if (v < H - 1) gy += smooth_sgn(d0 - d[idx + W]) * (double)smooth_edge_weight(im, hw, idx, idx + W);
    if (v > 0) gy -= smooth_sgn(d[idx - W] - d0) * (double)smooth_edge_weight(im, hw, idx - W, idx);
    const double Nx = (double)P.N * H * (W - 1), Ny = (double)P.N * (H - 1) * W;
    const double ln = sumx / Nx + sumy / Ny;
    P.g_disp[(size_t)n * hw + idx] = (float)((double)*P.g_loss * (sn * (gx / Nx + gy / Ny) - ln / (double)hw) / (mean + 1e-7));
}

}  // namespace tc
