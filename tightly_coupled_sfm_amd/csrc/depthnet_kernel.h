// depthnet_kernel.h -- the reference's depth network (models/depth_w_access.py, num_scales = 1) on gfx950: a ResNet18 encoder
// (torchvision BasicBlocks, BatchNorm with running statistics) and the U-Net decoder of depth_w_access.py:49-68 (nearest x2
// up-sampling, reflect-padded 3x3 convolutions, ELU, skip additions, an 8-channel feature convolution and a sigmoid head).
//
// Design (the machinery of posenet_kernel.h, see there):
//   * BatchNorm is folded into the convolution weights and biases ONCE at load time (host, float64); the weights are laid out
//     there for the matrix cores: w4[((tap * cin/16 + c16) * 4 + kq) * coutp + co] = float4 over t of w[co][c16*16 + 4 kq + t][tap];
//   * every convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), activations NHWC, operands global -> registers
//     with 16-byte loads.  The input transforms live in the A-operand gather: zero or reflect padding and nearest x2 up-sampling are
//     a per-lane row / column table (no padded or up-sampled copy is materialised); the first layer reads the caller's planar
//     NCHW images, normalises them ((x - 0.45) / 0.22) and optionally mirrors them horizontally;
//   * the epilogues are fused: bias, ReLU, residual add + ReLU, ELU, ELU + skip add; max pooling and the 8 -> 1 sigmoid head are
//     small kernels of their own;
//   * the work split of a layer (pixel blocks, channel blocks, waves sharing K) is a function of the layer's geometry only, never of
//     the number of images, and waves that share K are reduced through LDS in a fixed order: an image's result does not depend on
//     N or on the other images of the call.
#pragma once
#include <hip/hip_runtime.h>

namespace tc {

typedef float dn_f4 __attribute__((ext_vector_type(4)));

enum { DN_EPI_NONE = 0, DN_EPI_RELU = 1, DN_EPI_RES_RELU = 2, DN_EPI_ELU = 3, DN_EPI_ELU_ADD = 4 };

struct DnConvParams {
    const float *in;        // [N][ih][iw][cin] NHWC (the source grid: before up-sampling)
    const dn_f4 *w4;        // prepared weights (layout above)
    const float *bias;      // [coutp] (BatchNorm folded)
    const float *res;       // [N][oh][ow][cout]: residual (DN_EPI_RES_RELU, before the ReLU) or skip (DN_EPI_ELU_ADD, after the ELU)
    float *out;             // [N][oh][ow][cout]
    float *aux;             // DN_EPI_ELU_ADD: the ELU value before the skip add (training tape; NULL: not stored)
    int cin, cout, coutp;   // coutp = cout rounded up to 16 (the weight image's width; channels >= cout are zero and not stored)
    int ih, iw, oh, ow;
    int stride, pad, up, reflect, epi;
};

__device__ __forceinline__ float dn_elu(float v) { return v > 0.f ? v : expm1f(v); }

// One wave = PB blocks of 16 output pixels x NB blocks of 16 output channels, over 1 / KW of the input channel blocks.
// A workgroup = 4 waves: KW = 1: 4 consecutive pixel groups of the same channel blocks; KW = 4: ONE pixel group, its K split
// over the 4 waves and reduced through LDS in wave order (the small late layers, which otherwise run few, long serial chains).
// grid = (ceil(npix / (16 PB (4 / KW))), coutp / (16 NB), N).
template <int KS, int NB, int PB, int KW>
__global__ __launch_bounds__(256) void k_dn_conv(DnConvParams P) {
    constexpr int GC = 2;                                    // K groups whose loads are issued together
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int n = blockIdx.z;
    const int npix = P.oh * P.ow;
    const int pgrp = KW == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
    const int kpart = KW == 1 ? 0 : wave;
    const int pix0 = pgrp * PB * 16;
    const int cbase = blockIdx.y * 16 * NB;
    const int c16n = P.cin >> 4;
    const int clo = (c16n * kpart) / KW, chi = (c16n * (kpart + 1)) / KW;
    // per lane and pixel block: source row / column of every tap (-1: zero padding).  Reflect padding is applied on the
    // (virtual) up-sampled grid, then the nearest-neighbour source is row >> up.
    const int vh = P.ih << P.up, vw = P.iw << P.up;
    int ry[PB][KS], rx[PB][KS];
#pragma unroll
    for (int p = 0; p < PB; p++) {
        const int px = pix0 + 16 * p + m;
        const bool pv = px < npix;
        const int oy = pv ? px / P.ow : 0, ox = pv ? px - oy * P.ow : 0;
#pragma unroll
        for (int k = 0; k < KS; k++) {
            int uy = oy * P.stride + k - P.pad, ux = ox * P.stride + k - P.pad;
            if (P.reflect) {
                uy = uy < 0 ? -uy : (uy >= vh ? 2 * vh - 2 - uy : uy);
                ux = ux < 0 ? -ux : (ux >= vw ? 2 * vw - 2 - ux : ux);
            }
            ry[p][k] = (pv && uy >= 0 && uy < vh) ? (uy >> P.up) : -1;
            rx[p][k] = (ux >= 0 && ux < vw) ? (ux >> P.up) : -1;
        }
    }
    const float *img = P.in + (size_t)n * P.ih * P.iw * P.cin + 4 * kq;
    const dn_f4 *wl = P.w4 + (size_t)kq * P.coutp + cbase + m;
    dn_f4 acc[PB][NB];
#pragma unroll
    for (int p = 0; p < PB; p++)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[p][b] = (dn_f4){0.f, 0.f, 0.f, 0.f};
    if (pix0 < npix) {
#pragma unroll
        for (int ky = 0; ky < KS; ky++)
#pragma unroll
            for (int kx = 0; kx < KS; kx++) {
                const int tap = ky * KS + kx;
                int off[PB];
                bool ok[PB];
#pragma unroll
                for (int p = 0; p < PB; p++) {
                    ok[p] = ry[p][ky] >= 0 && rx[p][kx] >= 0;
                    off[p] = ok[p] ? (ry[p][ky] * P.iw + rx[p][kx]) * P.cin : 0;
                }
                const dn_f4 *wt = wl + (size_t)tap * c16n * 4 * P.coutp;
                for (int c0 = clo; c0 < chi; c0 += GC) {
                    dn_f4 a[GC][PB], b4[GC][NB];
#pragma unroll
                    for (int u = 0; u < GC; u++) {
                        const bool live = c0 + u < chi;              // (wave-uniform)
                        const int c = live ? c0 + u : c0;
#pragma unroll
                        for (int p = 0; p < PB; p++) a[u][p] = *reinterpret_cast<const dn_f4 *>(img + off[p] + c * 16);
#pragma unroll
                        for (int b = 0; b < NB; b++) b4[u][b] = wt[(size_t)c * 4 * P.coutp + b * 16];
                    }
                    __builtin_amdgcn_sched_barrier(0);      // all loads of the batch are issued before the first use
#pragma unroll
                    for (int u = 0; u < GC; u++) {
                        if (c0 + u >= chi) break;
#pragma unroll
                        for (int p = 0; p < PB; p++)
                            if (!ok[p]) a[u][p] = (dn_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < 4; t++)
#pragma unroll
                            for (int p = 0; p < PB; p++)
#pragma unroll
                                for (int b = 0; b < NB; b++) acc[p][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][p][t], b4[u][b][t], acc[p][b], 0, 0, 0);
                    }
                }
            }
    }
    if (KW > 1) {
        // fixed-order reduction of the K parts: ((w0 + w1) + w2) + w3, then wave 0 runs the epilogue
        __shared__ dn_f4 red[KW > 1 ? KW - 1 : 1][PB * NB][64];
        if (wave > 0)
#pragma unroll
            for (int p = 0; p < PB; p++)
#pragma unroll
                for (int b = 0; b < NB; b++) red[wave - 1][p * NB + b][lane] = acc[p][b];
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < KW - 1; w++)
#pragma unroll
            for (int p = 0; p < PB; p++)
#pragma unroll
                for (int b = 0; b < NB; b++) acc[p][b] += red[w][p * NB + b][lane];
    }
    // C/D layout of the 16x16 tile: column (output channel) = lane & 15, row (pixel) = 4 (lane >> 4) + reg
    const size_t obase = (size_t)n * npix * P.cout;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int co = cbase + b * 16 + m;
        if (co >= P.cout) continue;
        const float bs = P.bias[co];
#pragma unroll
        for (int p = 0; p < PB; p++) {
            const int prow0 = pix0 + 16 * p + 4 * kq;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int px = prow0 + r;
                if (px >= npix) continue;
                const size_t o = obase + (size_t)px * P.cout + co;
                float v = acc[p][b][r] + bs;
                switch (P.epi) {
                    case DN_EPI_RELU: v = fmaxf(v, 0.f); break;
                    case DN_EPI_RES_RELU: v = fmaxf(v + P.res[o], 0.f); break;
                    case DN_EPI_ELU: v = dn_elu(v); break;
                    case DN_EPI_ELU_ADD: {
                        const float e = dn_elu(v);
                        if (P.aux) P.aux[o] = e;
                        v = e + P.res[o];
                        break;
                    }
                    default: break;
                }
                P.out[o] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// first layer: conv1 7x7 stride 2, zero padding 3, 3 -> 64 channels, on the caller's planar images [N][3][H][W] normalised on the
// fly; BatchNorm folded, ReLU.  K is ordered as posenet_kernel.h's first layer: group g, quarter kq covers (ci, ky) = combo
// 2 g + (kq >> 1) and kx = 4 (kq & 1) + t, kx = 7 and combo >= 21 being zero weights (11 groups).  `flip` mirrors the input
// horizontally (column W - 1 - x is read for column x): bit-identical to running on torch.flip(imgs, [3]).
// One wave = PB blocks of 16 output pixels x 64 channels; grid = (ceil(npix / (64 PB)), 1, N).
struct DnConv1Params {
    const float *img;       // [N][3][H][W]
    const dn_f4 *w4;        // [(g * 4 + kq) * 64 + co]
    const float *bias;      // [64]
    float *out;             // [N][oh][ow][64]
    int ih, iw, oh, ow, flip;
};

template <int PB>
__global__ __launch_bounds__(256) void k_dn_conv1(DnConv1Params P) {
    constexpr int NB = 4, NG = 11;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int n = blockIdx.z;
    const int npix = P.oh * P.ow;
    const int pix0 = (blockIdx.x * 4 + wave) * PB * 16;
    const size_t hw = (size_t)P.ih * P.iw;
    const float *img = P.img + (size_t)n * 3 * hw;
    int oy[PB], ox[PB];
    bool pv[PB];
#pragma unroll
    for (int p = 0; p < PB; p++) {
        const int px = pix0 + 16 * p + m;
        pv[p] = px < npix;
        oy[p] = pv[p] ? px / P.ow : 0; ox[p] = pv[p] ? px - oy[p] * P.ow : 0;
    }
    dn_f4 acc[PB][NB];
#pragma unroll
    for (int p = 0; p < PB; p++)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[p][b] = (dn_f4){0.f, 0.f, 0.f, 0.f};
    if (pix0 < npix) {
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int combo = 2 * g + (kq >> 1);
            const bool cok = combo < 21;
            const int ci = cok ? combo / 7 : 0, ky = cok ? combo - 7 * (combo / 7) : 0;
            dn_f4 a[PB], b4[NB];
#pragma unroll
            for (int p = 0; p < PB; p++) {
                const int iy = oy[p] * 2 + ky - 3;
                const bool rowok = cok && pv[p] && iy >= 0 && iy < P.ih;
                const float *row = img + (size_t)ci * hw + (size_t)(rowok ? iy : 0) * P.iw;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int kx = 4 * (kq & 1) + t, ix = ox[p] * 2 + kx - 3;
                    const bool ok = rowok && kx < 7 && ix >= 0 && ix < P.iw;
                    const int sx = ok ? (P.flip ? P.iw - 1 - ix : ix) : 0;
                    const float v = row[sx];
                    a[p][t] = ok ? (v - 0.45f) / 0.22f : 0.f;      // depth_w_access.py:48, zero padding of the normalised image
                }
            }
#pragma unroll
            for (int b = 0; b < NB; b++) b4[b] = P.w4[(size_t)(g * 4 + kq) * 64 + b * 16 + m];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int p = 0; p < PB; p++)
#pragma unroll
                    for (int b = 0; b < NB; b++) acc[p][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][t], b4[b][t], acc[p][b], 0, 0, 0);
        }
    }
    float *out = P.out + (size_t)n * npix * 64;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int co = b * 16 + m;
        const float bs = P.bias[co];
#pragma unroll
        for (int p = 0; p < PB; p++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int px = pix0 + 16 * p + 4 * kq + r;
                if (px < npix) out[(size_t)px * 64 + co] = fmaxf(acc[p][b][r] + bs, 0.f);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// max pooling 3x3, stride 2, padding 1 (padding never wins: -inf), NHWC with C % 4 == 0; one thread per output pixel and 4 channels
__global__ __launch_bounds__(256) void k_dn_maxpool(const float *in, float *out, int N, int C, int ih, int iw, int oh, int ow) {
    const int c4n = C >> 2;
    const long long total = (long long)N * oh * ow * c4n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e % c4n);
    const long long q = e / c4n;
    const int ox = (int)(q % ow), oy = (int)((q / ow) % oh), n = (int)(q / ((long long)ow * oh));
    const float *src = in + (size_t)n * ih * iw * C + 4 * c4;
    dn_f4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int ky = 0; ky < 3; ky++) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= ih) continue;
        for (int kx = 0; kx < 3; kx++) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= iw) continue;
            const dn_f4 v = *reinterpret_cast<const dn_f4 *>(src + ((size_t)iy * iw + ix) * C);
#pragma unroll
            for (int t = 0; t < 4; t++) mx[t] = fmaxf(mx[t], v[t]);
        }
    }
    *reinterpret_cast<dn_f4 *>(out + (size_t)q * C + 4 * c4) = mx;
}

// ---------------------------------------------------------------------------------------------------------------
// predict_disps.0: reflect-padded 3x3 convolution 8 -> 1 (+ bias), sigmoid -> disparity [N][1][H][W]; one thread per pixel,
// the 72 weights are wave-uniform.  Fixed summation order: taps row-major, channels ascending.
// DEPTH (the sequence calls' depth stage, depthnet_host.h dn_decode): the thread stores disp_to_depth's depth of its disparity instead
// -- kernels.h disp_depth, the expression of k_disp_to_depth, on the value k_dn_predict<false> would have stored: the bits of
// tcsfm_depthnet_forward followed by tcsfm_disp_to_depth, with no disparity plane and no second launch.
// dn_head_disp: the sigmoid disparity of pixel e, shared with the heads of disp_post_kernel.h (k_dn_head), which store other functions of it.
__device__ __forceinline__ float dn_head_disp(const float *in, const float *w, const float *bias, long long e, int H, int W) {
    const int x = (int)(e % W), y = (int)((e / W) % H), n = (int)(e / ((long long)W * H));
    const float *src = in + (size_t)n * H * W * 8;
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
        int yy = y + ky - 1;
        yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            int xx = x + kx - 1;
            xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
            const dn_f4 *v = reinterpret_cast<const dn_f4 *>(src + ((size_t)yy * W + xx) * 8);
            const dn_f4 lo = v[0], hi = v[1];
#pragma unroll
            for (int c = 0; c < 4; c++) s = fmaf(lo[c], w[(c * 3 + ky) * 3 + kx], s);
#pragma unroll
            for (int c = 0; c < 4; c++) s = fmaf(hi[c], w[((c + 4) * 3 + ky) * 3 + kx], s);
        }
    }
    s += bias[0];
    return 1.f / (1.f + expf(-s));
}

template <bool DEPTH>
__global__ __launch_bounds__(256) void k_dn_predict(const float *in, const float *w, const float *bias, float *out, int N, int H, int W,
                                                    float min_disp, float max_disp) {
    const long long total = (long long)N * H * W;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float disp = dn_head_disp(in, w, bias, e, H, W);
    out[e] = DEPTH ? disp_depth(disp, min_disp, max_disp) : disp;
}

}  // namespace tc
