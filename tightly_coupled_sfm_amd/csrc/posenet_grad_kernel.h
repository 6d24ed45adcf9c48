// posenet_grad_kernel.h -- the PoseNet's gradient with respect to its INPUT (posenet_kernel.h's network, weights frozen: the
// default mode of the reference's test-time tuning, where the (tgt * valid | img_rec) input of every call after the first depends
// on the depths through the warp).  The training forward is pn_run unchanged; it keeps, per layer, the reduced raw convolution
// output, the (scale, shift) pairs and the per-group (mean, rstd) in a caller-owned tape.
//
// Per layer l = 7 .. 1, from da_l (the gradient of the layer's activation a_l = relu(x^ gamma + beta), x^ = (z - mean) rstd):
//   g  = da_l [a_l > 0]                      the mask is pn_act(raw, scale, shift) > 0 -- ONE device function for every kernel here
//   S1 = sum_group gamma g,  S2 = sum_group gamma g x^     (k_pnb_gsum: per (image, group), in double, fixed order, like k_pn_stats)
//   dz = rstd (gamma g - S1 / m - x^ S2 / m)               (k_pnb_dz: elementwise, in place over da_l)
//   da_{l-1} = stride-2 transposed convolution of dz with the standardised weights:
//     layers 2..7: depthnet_grad_kernel.h's k_dnb_dgrad (implicit GEMM on v_mfma_f32_16x16x4_f32, stride and zero padding in its
//                  gather table) on the transposed image of the forward's own prepared weights (k_pnb_prep_t: a permutation of w4,
//                  so both passes multiply by the same bits);
//     layer 1:     k_pnb_dgrad1, a per-pixel gather over the at most 4 x 4 taps of the pixel's parity, planar output, 1 / 0.22 folded in.
// No float atomics; every reduction has a fixed order; the work splits depend on the layer geometry only and one image is one grid
// row, so an image's gradient depends neither on the other images of the call nor on their number.
#pragma once
#include <hip/hip_runtime.h>
#include "posenet_kernel.h"

namespace tc {

// The activation the backward's ReLU decisions are taken on (tcsfm_debug_posenet_tape_layer exports it).  The forward applies the same
// expression while it loads its operands; the compiler may contract it differently there, which can change the value only within an
// ulp of zero.
__device__ __forceinline__ float pn_act(float raw, float scale, float shift) { return fmaxf(raw * scale + shift, 0.f); }

// ---- transposed weight images: permutations of the forward's prepared (standardised) weights ----------------------------------------
// generic layers: wt4[((tap * cout/16 + o16) * 4 + oq) * cin + ci] = float4 over ot of w^[o16*16 + 4 oq + ot][ci][tap]  (k_dnb_dgrad's layout)
__global__ __launch_bounds__(256) void k_pnb_prep_t(const pn_f4 *w4, pn_f4 *wt4, int cin, int cout, int ks) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)ks * ks * cin * cout) return;
    const int ci = (int)(e % cin), co = (int)((e / cin) % cout), tap = (int)(e / ((long long)cin * cout));
    const int c16n = cin / 16, o16n = cout / 16;
    const float v = reinterpret_cast<const float *>(w4)[((size_t)((tap * c16n + (ci >> 4)) * 4 + ((ci >> 2) & 3)) * cout + co) * 4 + (ci & 3)];
    reinterpret_cast<float *>(wt4)[((size_t)((tap * o16n + (co >> 4)) * 4 + ((co >> 2) & 3)) * cin + ci) * 4 + (co & 3)] = v;
}

// first layer (k_pn_prep's 7x7 grouping) -> wt1[((ky * 7 + kx) * 6 + ci) * 16 + co]
__global__ __launch_bounds__(256) void k_pnb_prep_t1(const pn_f4 *w4, float *wt1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 49 * 6 * 16) return;
    const int co = e & 15, ci = (e >> 4) % 6, tap = (e >> 4) / 6, ky = tap / 7, kx = tap - 7 * ky;
    const int combo = ci * 7 + ky, grp = combo >> 1, kq = 2 * (combo & 1) + (kx >> 2), t = kx & 3;
    wt1[e] = reinterpret_cast<const float *>(w4)[((size_t)(grp * 4 + kq) * 16 + co) * 4 + t];
}

// ---- head: da_7[n][p][c] = (0.01 / npix) sum_j d_pose[n][j] W_h[j][c]  (j ascending) ------------------------------------------------
__global__ __launch_bounds__(256) void k_pnb_head(const float *d_pose, const float *w, float *da, int N, int npix) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * npix * 256) return;
    const int c = (int)(e & 255), n = (int)(e / ((long long)npix * 256));
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 6; j++) s = fmaf(d_pose[n * 6 + j], w[j * 256 + c], s);
    da[e] = s * (0.01f / (float)npix);
}

struct PnbNormParams {
    const float *da;        // [N][npix][cout] gradient of the layer's activation
    const float *raw;       // [N][npix][cout] taped raw convolution output
    const float *scsh;      // [N][cout][2] taped (scale, shift)
    const float *mr;        // [N][16][2] taped (mean, rstd) per group
    const float *gamma;     // [cout] or null (1)
    float *ss;              // [N][16][2]: (S1 / m, S2 / m)
    float *dz;              // [N][npix][cout] (may alias da)
    int N, npix, cout;
};

// S1 / m and S2 / m of one (image, group): one workgroup, elements strided over the threads in k_pn_stats' order, double sums, tree in LDS
__global__ __launch_bounds__(256) void k_pnb_gsum(PnbNormParams P) {
    const int n = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int cg = P.cout / 16, total = P.npix * cg;
    const size_t base = (size_t)n * P.npix * P.cout;
    const float *scsh = P.scsh + (size_t)n * P.cout * 2;
    const float mean = P.mr[((size_t)n * 16 + g) * 2], rstd = P.mr[((size_t)n * 16 + g) * 2 + 1];
    __shared__ double r1[256], r2[256];
    double s1 = 0.0, s2 = 0.0;
    for (int e = tid; e < total; e += 256) {
        const int p = e / cg, c = g * cg + (e - p * cg);
        const size_t i = base + (size_t)p * P.cout + c;
        const float z = P.raw[i];
        const float gg = pn_act(z, scsh[2 * c], scsh[2 * c + 1]) > 0.f ? P.da[i] : 0.f;
        const float t = (P.gamma ? P.gamma[c] : 1.f) * gg, xh = (z - mean) * rstd;
        s1 += (double)t; s2 += (double)t * (double)xh;
    }
    r1[tid] = s1; r2[tid] = s2; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) { r1[tid] += r1[tid + o]; r2[tid] += r2[tid + o]; } __syncthreads(); }
    if (tid == 0) {
        P.ss[((size_t)n * 16 + g) * 2] = (float)(r1[0] / total);
        P.ss[((size_t)n * 16 + g) * 2 + 1] = (float)(r2[0] / total);
    }
}

// dz = rstd (gamma g - S1 / m - x^ S2 / m), one thread per pixel and 4 channels (in place over da)
__global__ __launch_bounds__(256) void k_pnb_dz(PnbNormParams P) {
    const int c4n = P.cout >> 2, cg = P.cout / 16;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)P.N * P.npix * c4n) return;
    const int c0 = 4 * (int)(e % c4n), n = (int)(e / ((long long)P.npix * c4n));
    const size_t i = (size_t)e * 4;
    const pn_f4 z = *reinterpret_cast<const pn_f4 *>(P.raw + i), d = *reinterpret_cast<const pn_f4 *>(P.da + i);
    const float *scsh = P.scsh + ((size_t)n * P.cout + c0) * 2;
    pn_f4 o;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int c = c0 + t, g = c / cg;
        const float mean = P.mr[((size_t)n * 16 + g) * 2], rstd = P.mr[((size_t)n * 16 + g) * 2 + 1];
        const float s1m = P.ss[((size_t)n * 16 + g) * 2], s2m = P.ss[((size_t)n * 16 + g) * 2 + 1];
        const float gg = pn_act(z[t], scsh[2 * t], scsh[2 * t + 1]) > 0.f ? d[t] : 0.f;
        const float xh = (z[t] - mean) * rstd;
        const float tg = (P.gamma ? P.gamma[c] : 1.f) * gg;
        o[t] = rstd * ((tg - s1m) - xh * s2m);
    }
    *reinterpret_cast<pn_f4 *>(P.dz + i) = o;
}

// the activation of a taped layer, for tests: act[i] = pn_act(raw, scale, shift)
__global__ __launch_bounds__(256) void k_pnb_act(const float *raw, const float *scsh, float *act, int N, int npix, int cout) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * npix * cout) return;
    const int c = (int)(e % cout), n = (int)(e / ((long long)npix * cout));
    const float *s = scsh + ((size_t)n * cout + c) * 2;
    act[e] = pn_act(raw[e], s[0], s[1]);
}

// ---- layer 1's input gradient: d_img[n][ci][y][x] = (1 / 0.22) sum_{ky, kx, co} dz1[n][(y + 3 - ky) / 2][(x + 3 - kx) / 2][co] w^[co][ci][ky][kx]
// over the taps whose (y + 3 - ky, x + 3 - kx) is even and inside the output grid (ky, kx, co ascending).  A workgroup owns pixels of
// ONE parity class (y & 1, x & 1): its tap set and weight addresses are wave-uniform.  grid = (ceil(ceil(H/2) ceil(W/2) / 256), 4, N).
__global__ __launch_bounds__(256) void k_pnb_dgrad1(const float *dz, const float *__restrict__ wt1, float *d_img, int H, int W, int oh, int ow) {
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1, n = blockIdx.z;
    const int hh = (H + 1) >> 1, wh = (W + 1) >> 1;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= hh * wh) return;
    const int y = 2 * (q / wh) + py, x = 2 * (q % wh) + px;
    if (y >= H || x >= W) return;
    const float *dzn = dz + (size_t)n * oh * ow * 16;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ky = (py + 1) & 1; ky < 7; ky += 2) {
        const int oy = (y + 3 - ky) >> 1;                 // y + 3 - ky is even here; negative -> oy < 0
        if (y + 3 - ky < 0 || oy >= oh) continue;
        for (int kx = (px + 1) & 1; kx < 7; kx += 2) {
            const int ox = (x + 3 - kx) >> 1;
            if (x + 3 - kx < 0 || ox >= ow) continue;
            const pn_f4 *dp = reinterpret_cast<const pn_f4 *>(dzn + ((size_t)oy * ow + ox) * 16);
            const pn_f4 d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
            const float dv[16] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3], d2[0], d2[1], d2[2], d2[3], d3[0], d3[1], d3[2], d3[3]};
            const float *w = wt1 + (ky * 7 + kx) * 96;
#pragma unroll
            for (int ci = 0; ci < 6; ci++)
#pragma unroll
                for (int co = 0; co < 16; co++) acc[ci] = fmaf(dv[co], w[ci * 16 + co], acc[ci]);
        }
    }
    const size_t hw = (size_t)H * W;
    float *o = d_img + (size_t)n * 6 * hw + (size_t)y * W + x;
#pragma unroll
    for (int ci = 0; ci < 6; ci++) o[ci * hw] = acc[ci] * (1.f / 0.22f);
}

}  // namespace tc
