// warp_grad_kernel.h -- backward pass of k_warp (inverse_warp2, models/stn.py:234-273, under autograd): gfx950 device code.
//
// Inputs of the forward plus three optional cotangents g_rec [N,3,H,W], g_pd, g_cd [N,1,H,W] (projected / computed depth);
// outputs d_depth_t, d_depth_s [N,1,H,W] and d_pose [N,6].  The validity mask, the image and the intrinsics take no gradient.
// Nothing is taped: every kernel recomputes the geometry with warp_geo and the cell with tap1's floor / in-frame logic
// (warp_cell), so the bilinear cell, the out-of-range sentinel and the Z clamp are the forward's own decisions, bit for bit.
//
//   k_warp_bwd        one thread per target pixel on k_warp's grid: grid_sampler_2d backward (zero padding, align_corners =
//                     False) -> d ix, d iy -> d(X/Z), d(Y/Z) -> d_depth_t (plain store) and the 3 x 4 gradient with respect to
//                     P = K[R|t], g_p (x) [cam; 1]: twelve sums, wave butterfly -> LDS -> one record per workgroup, all in fp64
//                     (decisions in fp32 as the forward takes them, values in fp64: see the kernel).
//   k_warp_pose_tail  one workgroup per item: the records summed in index order in double, then on ONE thread the closed-form
//                     chain d P / d (tx .. rz) of pose_vec2mat(-pose), R = Rx Ry Rz.
//   k_warp_gmax       per item max |g_pd| (integer atomic max on the bit patterns of non-negative floats: order-independent).
//   k_warp_scatter    the adjoint of the bilinear sample of depth_s: g_pd x weight to the (at most four) in-frame taps, summed in
//                     64-bit fixed point with integer atomics.  The scale is a power of two taken from the item's max |g_pd| so
//                     that H W contributions of weight <= 1 cannot overflow: order-independent, bit-reproducible.
//   k_warp_fix_out    fixed point -> fp32.
//
// c.es (the depth scale of the pose + scale refinement) is 1 on this path (run_init without a log-scale): the factors es of
// d pd / d tap and d D / d depth_t are omitted and there is no scale gradient.
#pragma once
#include "kernels.h"

namespace tc {

// the bilinear cell of tap1: weights, clamped tap coordinates, and which taps are real source pixels
struct WarpCell {
    float wx, wy;
    int xi, yi;                 // the cell: floor(ix), floor(iy)
    int x0, x1, y0, y1;
    bool m00, m01, m10, m11;
};
__device__ __forceinline__ void warp_cell(int W, int H, int ui, int vi, float rx, float ry, bool oob, WarpCell &t) {
    float fx = floorf(rx), fy = floorf(ry);
    t.wx = rx - fx; t.wy = ry - fy;
    const int xi = ui + (int)fx, yi = vi + (int)fy;
    t.xi = xi; t.yi = yi;
    bool x0in = (xi >= 0) && (xi < W), x1in = (xi >= -1) && (xi < W - 1);
    bool y0in = (yi >= 0) && (yi < H), y1in = (yi >= -1) && (yi < H - 1);
    t.x0 = min(max(xi, 0), W - 1); t.x1 = min(max(xi + 1, 0), W - 1);
    t.y0 = min(max(yi, 0), H - 1); t.y1 = min(max(yi + 1, 0), H - 1);
    t.m00 = x0in && y0in && !oob; t.m01 = x1in && y0in && !oob;
    t.m10 = x0in && y1in && !oob; t.m11 = x1in && y1in && !oob;
}

struct WarpGradParams {
    const float *src, *depth_t, *depth_s;
    const PairConst *pc;
    const PairState *st;                // the fp64 intrinsics and transform the constants were rounded from (init_pair)
    const float *g_rec, *g_pd, *g_cd;   // cotangents, each may be null (= zero)
    float *d_depth_t;                   // [N][H*W] or null
    double *blockrec;                   // [N][workgroups per item][12] or null (no pose gradient wanted)
    int H, W;
};

// d value / d ix and d value / d iy of one plane's bilinear sample, times the cotangent g: a tap outside the frame contributes zero
__device__ __forceinline__ void warp_cell_grad(const float *__restrict__ img, int W, const WarpCell &t, double wx, double wy, double g, double &gix, double &giy) {
    const double v00 = t.m00 ? (double)img[t.y0 * W + t.x0] : 0.0, v01 = t.m01 ? (double)img[t.y0 * W + t.x1] : 0.0;
    const double v10 = t.m10 ? (double)img[t.y1 * W + t.x0] : 0.0, v11 = t.m11 ? (double)img[t.y1 * W + t.x1] : 0.0;
    gix += g * ((1.0 - wy) * (v01 - v00) + wy * (v11 - v10));
    giy += g * ((1.0 - wx) * (v10 - v00) + wx * (v11 - v01));
}

// The DECISIONS (bilinear cell, in-frame taps, sentinel, clamp) are warp_geo's and warp_cell's, in fp32 as the forward takes them.  The
// VALUES are evaluated in fp64 from the pair's fp64 intrinsics and transform: a valid pixel just above the clamp carries a gradient
// ~ 1 / Z^2 that dominates its item, and in fp32 its Z = D + q2 (terms of order 1, result of order 1e-3) is known to 1e-4 only.
__global__ __launch_bounds__(256) void k_warp_bwd(WarpGradParams P) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    const int hw = P.H * P.W;
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; i++) acc[i] = 0.0;
    if (idx < hw) {     // (no early return: the wave reduction below needs every lane)
        const int v = idx / P.W, u = idx - v * P.W;
        const float dep = P.depth_t[(size_t)n * hw + idx];
        Geo g;
        warp_geo(P.pc[n], P.W, P.H, u, v, dep, g);
        const bool oob = g.oobx || g.ooby;
        const PairState &S = P.st[n];
        const double fx = S.K[0], fy = S.K[4], cx = S.K[2], cy = S.K[5];
        const double *T = S.Tcur;
        // pixel2cam -> [R|t] -> cam2pixel2 (es = 1)
        const double D = (double)dep, r0 = ((double)u - cx) / fx, r1 = ((double)v - cy) / fy;
        const double c0 = r0 * D, c1 = r1 * D;
        const double X0 = T[0] * c0 + T[1] * c1 + T[2] * D + T[3];
        const double X1 = T[4] * c0 + T[5] * c1 + T[6] * D + T[7];
        const double X2 = T[8] * c0 + T[9] * c1 + T[10] * D + T[11];
        const double Z = g.zcl ? 1e-3 : X2, iz = 1.0 / Z;
        const double xp = (fx * X0 + cx * X2) * iz, yp = (fy * X1 + cy * X2) * iz;
        // d ix / d (X/Z) = W / (W - 1), d iy / d (Y/Z) = H / (H - 1)
        const double sx = (double)P.W / (double)(P.W - 1), sy = (double)P.H / (double)(P.H - 1);
        // the sentinel is detached: such a pixel passes nothing from g_rec or g_pd
        double gix = 0.0, giy = 0.0;
        if (!oob && (P.g_rec || P.g_pd)) {
            WarpCell t;
            warp_cell(P.W, P.H, u, v, g.rx, g.ry, false, t);
            const double wx = (xp * sx - 0.5) - (double)t.xi, wy = (yp * sy - 0.5) - (double)t.yi;      // weights inside the forward's cell
            if (P.g_rec)
                for (int ch = 0; ch < 3; ch++)
                    warp_cell_grad(P.src + ((size_t)n * 3 + ch) * hw, P.W, t, wx, wy, (double)P.g_rec[((size_t)n * 3 + ch) * hw + idx], gix, giy);
            if (P.g_pd) warp_cell_grad(P.depth_s + (size_t)n * hw, P.W, t, wx, wy, (double)P.g_pd[(size_t)n * hw + idx], gix, giy);
        }
        const double gcd = P.g_cd ? (double)P.g_cd[(size_t)n * hw + idx] : 0.0;
        const double gxp = gix * sx, gyp = giy * sy;
        // gradient with respect to p = P [cam; 1]:  X/Z = p0 / Z, Y/Z = p1 / Z, Z = clamp(p2): a clamped Z is a constant and stops g_cd
        const double gp0 = gxp * iz, gp1 = gyp * iz;
        const double gp2 = g.zcl ? 0.0 : gcd - (gxp * xp + gyp * yp) * iz;
        if (P.d_depth_t) {      // d p / d D = K R K^-1 pix
            const double gX0 = fx * gp0, gX1 = fy * gp1, gX2 = cx * gp0 + cy * gp1 + gp2;
            P.d_depth_t[(size_t)n * hw + idx] = (float)(gX0 * (T[0] * r0 + T[1] * r1 + T[2]) + gX1 * (T[4] * r0 + T[5] * r1 + T[6]) +
                                                        gX2 * (T[8] * r0 + T[9] * r1 + T[10]));
        }
        acc[0] = gp0 * c0; acc[1] = gp0 * c1; acc[2] = gp0 * D; acc[3] = gp0;
        acc[4] = gp1 * c0; acc[5] = gp1 * c1; acc[6] = gp1 * D; acc[7] = gp1;
        acc[8] = gp2 * c0; acc[9] = gp2 * c1; acc[10] = gp2 * D; acc[11] = gp2;
    }
    if (P.blockrec == nullptr) return;
    // fixed-order fp64 butterfly over the wave (wave_reduce.h's butterfly is fp32), then LDS, then one record per workgroup
    __shared__ double red[4][12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        double s = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int t = threadIdx.x;
        P.blockrec[((size_t)n * gridDim.x + blockIdx.x) * 12 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

// d_pose[n] from the workgroup records: G = d L / d P (3 x 4), P = K T, T = pose_vec2mat(-pose) = [Rx(a) Ry(b) Rz(c) | -t],
// (a, b, c) = -(rx, ry, rz):  d L / d T = K' G,  d L / d t_i = -(K' G)_i3,  d L / d r_k = -<(K' G)[:, :3], d R / d angle_k>.
__global__ __launch_bounds__(64) void k_warp_pose_tail(const double *blockrec, int nblk, const float *pose, const float *K, float *d_pose) {
    const int n = blockIdx.x, tid = threadIdx.x;
    __shared__ double G[12];
    if (tid < 12) {
        double s = 0.0;
        for (int b = 0; b < nblk; b++) s += blockrec[((size_t)n * nblk + b) * 12 + tid];
        G[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double fx = (double)K[n * 9 + 0], fy = (double)K[n * 9 + 4], cx = (double)K[n * 9 + 2], cy = (double)K[n * 9 + 5];
    double dT[12];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        dT[j] = fx * G[j];
        dT[4 + j] = fy * G[4 + j];
        dT[8 + j] = cx * G[j] + cy * G[4 + j] + G[8 + j];
    }
    const double a = -(double)pose[n * 6 + 3], b = -(double)pose[n * 6 + 4], c = -(double)pose[n * 6 + 5];
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cc = cos(c), sc = sin(c);
    const double Rx[9] = {1, 0, 0, 0, ca, -sa, 0, sa, ca}, dRx[9] = {0, 0, 0, 0, -sa, -ca, 0, ca, -sa};
    const double Ry[9] = {cb, 0, sb, 0, 1, 0, -sb, 0, cb}, dRy[9] = {-sb, 0, cb, 0, 0, 0, -cb, 0, -sb};
    const double Rz[9] = {cc, -sc, 0, sc, cc, 0, 0, 0, 1}, dRz[9] = {-sc, -cc, 0, cc, -sc, 0, 0, 0, 0};
    double RyRz[9], RxRy[9], Da[9], Db[9], Dc[9], tmp[9];
    mat3_mul(Ry, Rz, RyRz);
    mat3_mul(Rx, Ry, RxRy);
    mat3_mul(dRx, RyRz, Da);
    mat3_mul(dRy, Rz, tmp);
    mat3_mul(Rx, tmp, Db);
    mat3_mul(RxRy, dRz, Dc);
    double ga = 0.0, gb = 0.0, gc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            ga += dT[4 * i + j] * Da[3 * i + j];
            gb += dT[4 * i + j] * Db[3 * i + j];
            gc += dT[4 * i + j] * Dc[3 * i + j];
        }
    float *o = d_pose + n * 6;
    o[0] = (float)(-dT[3]); o[1] = (float)(-dT[7]); o[2] = (float)(-dT[11]);
    o[3] = (float)(-ga); o[4] = (float)(-gb); o[5] = (float)(-gc);
}

// ---------------------------------------------------------------------------------------------------------------
// source-depth gradient: fixed-point scatter

// gmax[n] = bit pattern of max |g_pd| over item n (zero when the launch starts).  Non-negative floats order as their bit patterns,
// NaN above infinity: one integer atomic max per workgroup.
__global__ __launch_bounds__(256) void k_warp_gmax(const float *g_pd, unsigned *gmax, int hw) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    unsigned m = idx < hw ? (__float_as_uint(g_pd[(size_t)n * hw + idx]) & 0x7fffffffu) : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if (m != 0u) atomicMax(gmax + n, m);
    }
}

// The fixed-point exponent of an item: contributions are |g_pd w| <= gmax < 2^x (frexp), a destination receives at most H W <= 2^lg_hw
// of them, so with the scale 2^(62 - lg_hw - x) every sum stays below 2^62.  -> false when nothing is to be scattered (gmax zero) or
// the cotangent is not finite (the tail then writes NaN).
__device__ __forceinline__ bool warp_fix_exp(unsigned gmax_bits, int lg_hw, int &e) {
    e = 0;
    if (gmax_bits == 0u || gmax_bits >= 0x7f800000u) return false;
    int x;
    (void)frexpf(__uint_as_float(gmax_bits), &x);
    e = 62 - lg_hw - x;
    return true;
}

struct WarpScatterParams {
    const float *depth_t;
    const PairConst *pc;
    const float *g_pd;
    const unsigned *gmax;       // [N]
    long long *fix;             // [N][H*W] fixed-point sums, zero when the launch starts
    int H, W, lg_hw;
};

// The weights here are the forward's own fp32 weights (warp_cell: the fractional part of warp_geo's small relative coordinate), while
// k_warp_bwd forms its weights in fp64 inside the same cell: d_depth_s follows the fp32 sample position and d_depth_t / d_pose the
// fp64 one.  The two positions differ by the forward's own rounding (~1e-6 px); the cell and the in-frame taps are the same.
__global__ __launch_bounds__(256) void k_warp_scatter(WarpScatterParams P) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    const int hw = P.H * P.W;
    if (idx >= hw) return;
    int e;
    if (!warp_fix_exp(P.gmax[n], P.lg_hw, e)) return;
    const float gpd = P.g_pd[(size_t)n * hw + idx];
    if (gpd == 0.f) return;
    const int v = idx / P.W, u = idx - v * P.W;
    Geo g;
    warp_geo(P.pc[n], P.W, P.H, u, v, P.depth_t[(size_t)n * hw + idx], g);
    if (g.oobx || g.ooby) return;
    WarpCell t;
    warp_cell(P.W, P.H, u, v, g.rx, g.ry, false, t);
    const double scale = ldexp(1.0, e);
    long long *fix = P.fix + (size_t)n * hw;
    const float ax = 1.f - t.wx, ay = 1.f - t.wy;
    const float w4[4] = {ax * ay, t.wx * ay, ax * t.wy, t.wx * t.wy};
    const bool m4[4] = {t.m00, t.m01, t.m10, t.m11};
    const int i4[4] = {t.y0 * P.W + t.x0, t.y0 * P.W + t.x1, t.y1 * P.W + t.x0, t.y1 * P.W + t.x1};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (m4[k]) {
            const long long a = (long long)llrint((double)(gpd * w4[k]) * scale);
            if (a != 0) atomicAdd(reinterpret_cast<unsigned long long *>(fix + i4[k]), (unsigned long long)a);
        }
}

__global__ __launch_bounds__(256) void k_warp_fix_out(const long long *fix, const unsigned *gmax, float *d_depth_s, int hw, int lg_hw) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (idx >= hw) return;
    int e;
    const unsigned gm = gmax[n];
    const bool on = warp_fix_exp(gm, lg_hw, e);
    float r = 0.f;
    if (on) r = (float)((double)fix[(size_t)n * hw + idx] * ldexp(1.0, -e));
    else if (gm != 0u) r = __uint_as_float(0x7fc00000u);      // a cotangent that is not finite
    d_depth_s[(size_t)n * hw + idx] = r;
}

}  // namespace tc
