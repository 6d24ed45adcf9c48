// depthnet_grad_kernel.h -- the backward pass of depthnet_kernel.h's network (exact fp32, BatchNorm in evaluation mode,
// num_scales = 1).  The training forward reuses depthnet_kernel.h's kernels unchanged; it only keeps every activation the backward
// needs in a caller-owned tape.  Activation derivatives come from the saved outputs y (ReLU: y > 0, ELU: y > 0 ? 1 : y + 1,
// sigmoid: y (1 - y)), so no pre-activation is stored.
//
//   * data gradient of a convolution: an implicit GEMM on v_mfma_f32_16x16x4_f32 over K = (tap, cout) with the transposed weight
//     image wt4 (the forward's layout with cin and cout swapped).  A lane owns a pixel of the layer's input grid ("direct": zero
//     padding, no up-sampling, the previous layer's activation derivative, residual and skip gradients fused in the epilogue) or of
//     its padded virtual grid ("padded": reflect padding and / or nearest x2 up-sampling, whose adjoints -- fold the reflected
//     border back, sum each 2 x 2 -- run in k_dnb_fold together with the derivative).  Stride 2 and zero padding are in the gather
//     table (-1 = no contribution), as in the forward.  Work splits depend on the layer's geometry only, one image per grid row:
//     an image's data gradient does not depend on the other images of the call;
//   * weight gradient: a GEMM with M = cout, N = cin (per tap), K = pixels, split into per-image pixel chunks whose partials are
//     reduced in a fixed order (k_dnb_wsum): no float atomics, the result is bit-reproducible;
//   * the BatchNorm chain rule (k_dnb_param_grad) and the device re-fold of the parameters (k_dnb_fold_params, float64 with
//     contraction off: the same bits as tcsfm_depthnet_load's host fold).
#pragma once
#include <hip/hip_runtime.h>
#include "depthnet_kernel.h"

namespace tc {

enum { DN_ACT_NONE = 0, DN_ACT_RELU = 1, DN_ACT_ELU = 2 };

__device__ __forceinline__ float dn_dact(int act, float y) {
    return act == DN_ACT_RELU ? (y > 0.f ? 1.f : 0.f) : (act == DN_ACT_ELU ? (y > 0.f ? 1.f : y + 1.f) : 1.f);
}

struct DnDgradParams {
    const float *dz;        // [N][oh][ow][cout]: gradient of the layer's pre-activation
    const dn_f4 *wt4;       // wt4[((tap * coutp/16 + c16) * 4 + kq) * cin + ci] = float4 over t of w'[c16*16 + 4 kq + t][ci][tap]
    float *out;             // direct: [N][gh][gw][cin] (the input grid); padded: [N][gh][gw][cin] (the padded virtual grid)
    const float *add1, *add2;   // direct: gradients added before the derivative (NULL: none)
    const float *y;         // direct: the layer's input (the previous activation's output) for the derivative
    int act;                // direct: DN_ACT_*
    int cin, cout, coutp;
    int gh, gw, goff;       // lane grid and its origin in padded coordinates (direct: goff = pad; padded: 0)
    int oh, ow, stride, direct;
};

// One wave = PB blocks of 16 lane-grid pixels x NB blocks of 16 input channels, over 1 / KW of K; the layout and the fixed-order
// LDS reduction are k_dn_conv's.  grid = (ceil(gpix / (16 PB (4 / KW))), cin / (16 NB), N).
template <int KS, int NB, int PB, int KW>
__global__ __launch_bounds__(256) void k_dnb_dgrad(DnDgradParams P) {
    constexpr int GC = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int n = blockIdx.z;
    const int gpix = P.gh * P.gw;
    const int pgrp = KW == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
    const int kpart = KW == 1 ? 0 : wave;
    const int pix0 = pgrp * PB * 16;
    const int cbase = blockIdx.y * 16 * NB;
    const int c16n = P.coutp >> 4;
    const int clo = (c16n * kpart) / KW, chi = (c16n * (kpart + 1)) / KW;
    // output pixel read by (lane pixel, tap): (g + goff - k) / stride when divisible and inside the output grid, else -1
    int ry[PB][KS], rx[PB][KS];
#pragma unroll
    for (int p = 0; p < PB; p++) {
        const int px = pix0 + 16 * p + m;
        const bool pv = px < gpix;
        const int gy = pv ? px / P.gw : 0, gx = pv ? px - gy * P.gw : 0;
#pragma unroll
        for (int k = 0; k < KS; k++) {
            const int uy = gy + P.goff - k, ux = gx + P.goff - k;
            const int oy = uy >= 0 && uy % P.stride == 0 ? uy / P.stride : -1;
            const int ox = ux >= 0 && ux % P.stride == 0 ? ux / P.stride : -1;
            ry[p][k] = (pv && oy >= 0 && oy < P.oh) ? oy : -1;
            rx[p][k] = (ox >= 0 && ox < P.ow) ? ox : -1;
        }
    }
    const float *dz = P.dz + (size_t)n * P.oh * P.ow * P.cout;
    const dn_f4 *wl = P.wt4 + (size_t)kq * P.cin + cbase + m;
    dn_f4 acc[PB][NB];
#pragma unroll
    for (int p = 0; p < PB; p++)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[p][b] = (dn_f4){0.f, 0.f, 0.f, 0.f};
    if (pix0 < gpix) {
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
                    off[p] = ok[p] ? (ry[p][ky] * P.ow + rx[p][kx]) * P.cout : 0;
                }
                const dn_f4 *wt = wl + (size_t)tap * c16n * 4 * P.cin;
                for (int c0 = clo; c0 < chi; c0 += GC) {
                    dn_f4 a[GC][PB], b4[GC][NB];
#pragma unroll
                    for (int u = 0; u < GC; u++) {
                        const bool live = c0 + u < chi;
                        const int c = live ? c0 + u : c0;
                        const int ch = c * 16 + 4 * kq;
                        const bool cok = ch < P.cout;                // cout = 8: the upper half of the block is zero
                        const int chs = cok ? ch : 0;
#pragma unroll
                        for (int p = 0; p < PB; p++) {
                            a[u][p] = *reinterpret_cast<const dn_f4 *>(dz + off[p] + chs);
                            if (!cok) a[u][p] = (dn_f4){0.f, 0.f, 0.f, 0.f};
                        }
#pragma unroll
                        for (int b = 0; b < NB; b++) b4[u][b] = wt[(size_t)c * 4 * P.cin + b * 16];
                    }
                    __builtin_amdgcn_sched_barrier(0);
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
    const size_t obase = (size_t)n * gpix * P.cin;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int ci = cbase + b * 16 + m;
#pragma unroll
        for (int p = 0; p < PB; p++) {
            const int prow0 = pix0 + 16 * p + 4 * kq;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int px = prow0 + r;
                if (px >= gpix) continue;
                const size_t o = obase + (size_t)px * P.cin + ci;
                float v = acc[p][b][r];
                if (P.direct) {
                    if (P.add1) v += P.add1[o];
                    if (P.add2) v += P.add2[o];
                    if (P.act != DN_ACT_NONE) v *= dn_dact(P.act, P.y[o]);     // (y is NULL without an activation)
                }
                P.out[o] = v;
            }
        }
    }
}

// Adjoint of reflect padding (pad 1) and nearest x2 up-sampling, then the previous activation's derivative: for a pixel of the
// source grid [N][ih][iw][C], sum the padded-grid gradient src [N][gh][gw][C] over every padded position that reads it (rows and
// columns in a fixed order), add `add`, store the raw sum to raw_out (skip gradients) and sum * act'(y) to out (either may be NULL).
// With up = pad = reflect = 0 and gh = ih it is the elementwise (src + add) * act'(y).  One thread per pixel and 4 channels.
struct DnFoldParams {
    const float *src, *add, *y;
    float *out, *raw_out;
    int N, C, ih, iw, gh, gw, up, pad, reflect, act;
};

__device__ __forceinline__ int dnb_rows(int s, int up, int pad, int reflect, int v, int q[4]) {
    // padded positions (q = u + pad, plus the reflected border image) of the virtual rows u that read source row s
    int nq = 0;
    for (int d = 0; d <= up; d++) {
        const int u = (s << up) + d;
        q[nq++] = u + pad;
        if (reflect && pad == 1) {
            if (u == 1) q[nq++] = 0;                 // padded row -1 reflects to 1
            if (u == v - 2) q[nq++] = v + 1;         // padded row v reflects to v - 2
        }
    }
    return nq;
}

__global__ __launch_bounds__(256) void k_dnb_fold(DnFoldParams P) {
    const int c4n = P.C >> 2;
    const long long total = (long long)P.N * P.ih * P.iw * c4n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e % c4n);
    const long long q = e / c4n;
    const int x = (int)(q % P.iw), y = (int)((q / P.iw) % P.ih), n = (int)(q / ((long long)P.iw * P.ih));
    int qy[4], qx[4];
    const int ny = dnb_rows(y, P.up, P.pad, P.reflect, P.ih << P.up, qy);
    const int nx = dnb_rows(x, P.up, P.pad, P.reflect, P.iw << P.up, qx);
    const float *src = P.src ? P.src + (size_t)n * P.gh * P.gw * P.C + 4 * c4 : nullptr;
    dn_f4 s = {0.f, 0.f, 0.f, 0.f};
    if (P.src)                                       // (NULL: a zero gradient)
        for (int i = 0; i < ny; i++)
            for (int j = 0; j < nx; j++) s += *reinterpret_cast<const dn_f4 *>(src + ((size_t)qy[i] * P.gw + qx[j]) * P.C);
    const size_t o = (size_t)q * P.C + 4 * c4;
    if (P.add) s += *reinterpret_cast<const dn_f4 *>(P.add + o);
    if (P.raw_out) *reinterpret_cast<dn_f4 *>(P.raw_out + o) = s;
    if (P.out) {
        if (P.act != DN_ACT_NONE) {
            const dn_f4 yv = *reinterpret_cast<const dn_f4 *>(P.y + o);
#pragma unroll
            for (int t = 0; t < 4; t++) s[t] *= dn_dact(P.act, yv[t]);
        }
        *reinterpret_cast<dn_f4 *>(P.out + o) = s;
    }
}

// Max-pool backward (3x3, stride 2, padding 1) fused with the skip-0 gradient and conv1's ReLU: for every input pixel, the pooled
// gradients of the windows whose argmax it is (recomputed from the saved input; ties go to the first element in row-major window
// order, as in torch), in window order, + dskip, times (x > 0).  One thread per input pixel and 4 channels.
__global__ __launch_bounds__(256) void k_dnb_maxpool(const float *x, const float *dpool, const float *dskip, float *dz, int N, int C,
                                                     int ih, int iw, int oh, int ow) {
    const int c4n = C >> 2;
    const long long total = (long long)N * ih * iw * c4n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e % c4n);
    const long long q = e / c4n;
    const int ix = (int)(q % iw), iy = (int)((q / iw) % ih), n = (int)(q / ((long long)iw * ih));
    const float *src = x + (size_t)n * ih * iw * C + 4 * c4;
    const float *dp = dpool + (size_t)n * oh * ow * C + 4 * c4;
    dn_f4 g = {0.f, 0.f, 0.f, 0.f};
    for (int oy = iy / 2; oy <= (iy + 1) / 2; oy++) {                 // the windows 2 o - 1 .. 2 o + 1 that hold iy, ascending
        if (oy >= oh || 2 * oy - 1 > iy || 2 * oy + 1 < iy) continue;
        for (int ox = ix / 2; ox <= (ix + 1) / 2; ox++) {
            if (ox >= ow || 2 * ox - 1 > ix || 2 * ox + 1 < ix) continue;
            dn_f4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int ay[4] = {-1, -1, -1, -1}, ax[4] = {-1, -1, -1, -1};
            for (int ky = 0; ky < 3; ky++) {
                const int yy = 2 * oy - 1 + ky;
                if (yy < 0 || yy >= ih) continue;
                for (int kx = 0; kx < 3; kx++) {
                    const int xx = 2 * ox - 1 + kx;
                    if (xx < 0 || xx >= iw) continue;
                    const dn_f4 v = *reinterpret_cast<const dn_f4 *>(src + ((size_t)yy * iw + xx) * C);
#pragma unroll
                    for (int t = 0; t < 4; t++)
                        if (v[t] > mx[t] || ay[t] < 0) { mx[t] = v[t]; ay[t] = yy; ax[t] = xx; }
                }
            }
            const dn_f4 d = *reinterpret_cast<const dn_f4 *>(dp + ((size_t)oy * ow + ox) * C);
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (ay[t] == iy && ax[t] == ix) g[t] += d[t];
        }
    }
    const size_t o = (size_t)q * C + 4 * c4;
    if (dskip) g += *reinterpret_cast<const dn_f4 *>(dskip + o);
    const dn_f4 yv = *reinterpret_cast<const dn_f4 *>(x + o);
#pragma unroll
    for (int t = 0; t < 4; t++) g[t] = yv[t] > 0.f ? g[t] : 0.f;
    *reinterpret_cast<dn_f4 *>(dz + o) = g;
}

__device__ __forceinline__ int dnb_reflect(int u, int v) { return u < 0 ? -u : (u >= v ? 2 * v - 2 - u : u); }

// The sigmoid head's data gradient: for every pixel of the feature map f [N][H][W][8], the sum over the disparity pixels that read
// it through the reflect-padded 3x3 convolution (rows, columns, then taps in a fixed order) of ds * w, with ds = ddisp d (1 - d);
// times ELU'(f).  One thread per pixel.
__global__ __launch_bounds__(256) void k_dnb_head(const float *f, const float *disp, const float *ddisp, const float *w, float *dz,
                                                  int N, int H, int W) {
    const long long total = (long long)N * H * W;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int sx = (int)(e % W), sy = (int)((e / W) % H), n = (int)(e / ((long long)W * H));
    const size_t ib = (size_t)n * H * W;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int y = sy - 1; y <= sy + 1; y++) {
        if (y < 0 || y >= H) continue;
        for (int x = sx - 1; x <= sx + 1; x++) {
            if (x < 0 || x >= W) continue;
            const size_t p = ib + (size_t)y * W + x;
            const float d = disp[p], ds = ddisp[p] * (d * (1.f - d));
            for (int ky = 0; ky < 3; ky++) {
                if (dnb_reflect(y + ky - 1, H) != sy) continue;
                for (int kx = 0; kx < 3; kx++) {
                    if (dnb_reflect(x + kx - 1, W) != sx) continue;
#pragma unroll
                    for (int c = 0; c < 8; c++) g[c] = fmaf(ds, w[(c * 3 + ky) * 3 + kx], g[c]);
                }
            }
        }
    }
    const float *fv = f + (size_t)e * 8;
    float *o = dz + (size_t)e * 8;
#pragma unroll
    for (int c = 0; c < 8; c++) o[c] = g[c] * dn_dact(DN_ACT_ELU, fv[c]);
}

// The head's weight and bias gradient partials: block b = (image, chunk of DNB_HEAD_CHUNK pixels) -> part[b][0..71] (weight, reference
// order [c][ky][kx]) and part[b][72] (bias).  128 threads stride the chunk, then thread j sums the 128 partials in thread order.
constexpr int DNB_HEAD_CHUNK = 4096;
__global__ __launch_bounds__(128) void k_dnb_head_wgrad(const float *f, const float *disp, const float *ddisp, float *part, int H, int W,
                                                        int nchunk) {
    __shared__ float red[73][128];
    const int n = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int npix = H * W, p0 = ch * DNB_HEAD_CHUNK, p1 = min(npix, p0 + DNB_HEAD_CHUNK);
    float a[73];
#pragma unroll
    for (int j = 0; j < 73; j++) a[j] = 0.f;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 128) {
        const int y = p / W, x = p - y * W;
        const size_t pi = (size_t)n * npix + p;
        const float d = disp[pi], ds = ddisp[pi] * (d * (1.f - d));
#pragma unroll
        for (int ky = 0; ky < 3; ky++) {
            const int yy = dnb_reflect(y + ky - 1, H);
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                const int xx = dnb_reflect(x + kx - 1, W);
                const float *v = f + ((size_t)n * npix + (size_t)yy * W + xx) * 8;
#pragma unroll
                for (int c = 0; c < 8; c++) a[(c * 3 + ky) * 3 + kx] = fmaf(ds, v[c], a[(c * 3 + ky) * 3 + kx]);
            }
        }
        a[72] += ds;
    }
#pragma unroll
    for (int j = 0; j < 73; j++) red[j][threadIdx.x] = a[j];
    __syncthreads();
    if (threadIdx.x < 73) {
        float s = 0.f;
        for (int t = 0; t < 128; t++) s += red[threadIdx.x][t];
        part[(size_t)blockIdx.x * 73 + threadIdx.x] = s;
    }
}

// Weight-gradient partials of a convolution: M = cout (MB blocks of 16 per workgroup), N = 16 input channels, one accumulator per
// tap; K = the pixels of one chunk of one image, its 4-pixel steps dealt to the 4 waves in turn and the waves reduced through LDS in
// wave order.  part[(n * nchunk + chunk)][co][ci][tap] (the reference layout).  planar: conv1 (7x7/2, zero padding 3) on the
// normalised planar images: N = 32 (ci, kx) combinations in two blocks, the 7 "taps" are ky (depthnet_kernel.h's gather).
// grid = (N * nchunk, cin / 16 (planar: 2), coutp / (16 MB)).
struct DnWgradParams {
    const float *dz;        // [N][oh][ow][cout]
    const float *x;         // [N][ih][iw][cin] NHWC (planar: [N][3][ih][iw] images)
    float *part;
    int cin, cout, ih, iw, oh, ow, stride, pad, up, reflect, chunk, nchunk;
};

template <int T, int MB, bool PLANAR>
__global__ __launch_bounds__(256) void k_dnb_wgrad(DnWgradParams P) {
    constexpr int KS = PLANAR ? 7 : (T == 9 ? 3 : 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int n = blockIdx.x / P.nchunk, ch = blockIdx.x % P.nchunk;
    const int npix = P.oh * P.ow;
    const int p0 = ch * P.chunk, p1 = min(npix, p0 + P.chunk);
    const int cb = blockIdx.y * 16, cob = blockIdx.z * 16 * MB;
    const float *dz = P.dz + (size_t)n * npix * P.cout;
    const int vh = P.ih << P.up, vw = P.iw << P.up;
    // planar: column m of block y is the combination 16 y + m = 7 ci + kx (valid below 21)
    const int combo = cb + m;
    const bool cok = !PLANAR || combo < 21;
    const int pci = PLANAR ? (cok ? combo / 7 : 0) : 0, pkx = PLANAR ? (cok ? combo - 7 * (combo / 7) : 0) : 0;
    const float *xb = PLANAR ? P.x + ((size_t)n * 3 + pci) * P.ih * P.iw : P.x + (size_t)n * P.ih * P.iw * P.cin + cb + m;
    dn_f4 acc[MB][T];
#pragma unroll
    for (int i = 0; i < MB; i++)
#pragma unroll
        for (int t = 0; t < T; t++) acc[i][t] = (dn_f4){0.f, 0.f, 0.f, 0.f};
    for (int s = p0 + 4 * wave; s < p1; s += 16) {
        const int px = s + kq;
        const bool pv = px < p1;
        const int oy = pv ? px / P.ow : 0, ox = pv ? px - oy * P.ow : 0;
        float a[MB], b[T];
#pragma unroll
        for (int i = 0; i < MB; i++) {
            const int co = cob + 16 * i + m;
            a[i] = pv && co < P.cout ? dz[(size_t)px * P.cout + co] : 0.f;
        }
        if (PLANAR) {
            const int ix = ox * 2 + pkx - 3;
            const bool xok = pv && cok && ix >= 0 && ix < P.iw;
#pragma unroll
            for (int ky = 0; ky < T; ky++) {
                const int iy = oy * 2 + ky - 3;
                const bool ok = xok && iy >= 0 && iy < P.ih;
                const float v = xb[ok ? (size_t)iy * P.iw + ix : 0];
                b[ky] = ok ? (v - 0.45f) / 0.22f : 0.f;
            }
        } else {
#pragma unroll
            for (int ky = 0; ky < KS; ky++) {
                int uy = oy * P.stride + ky - P.pad;
                if (P.reflect) uy = dnb_reflect(uy, vh);
                const int sy = (uy >= 0 && uy < vh) ? (uy >> P.up) : -1;
#pragma unroll
                for (int kx = 0; kx < KS; kx++) {
                    int ux = ox * P.stride + kx - P.pad;
                    if (P.reflect) ux = dnb_reflect(ux, vw);
                    const int sx = (ux >= 0 && ux < vw) ? (ux >> P.up) : -1;
                    const bool ok = pv && sy >= 0 && sx >= 0;
                    const float v = xb[ok ? ((size_t)sy * P.iw + sx) * P.cin : 0];
                    b[ky * KS + kx] = ok ? v : 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < MB; i++)
#pragma unroll
            for (int t = 0; t < T; t++) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[t], acc[i][t], 0, 0, 0);
    }
    __shared__ dn_f4 red[3][MB * T][64];
    if (wave > 0)
#pragma unroll
        for (int i = 0; i < MB; i++)
#pragma unroll
            for (int t = 0; t < T; t++) red[wave - 1][i * T + t][lane] = acc[i][t];
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; w++)
#pragma unroll
        for (int i = 0; i < MB; i++)
#pragma unroll
            for (int t = 0; t < T; t++) acc[i][t] += red[w][i * T + t][lane];
    // C layout: column (input channel / combination) = m, row (output channel) = 4 kq + r
    const int cinT = PLANAR ? 147 : P.cin * T;
    float *out = P.part + (size_t)blockIdx.x * P.cout * cinT;
    if (!cok) return;
#pragma unroll
    for (int i = 0; i < MB; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int co = cob + 16 * i + 4 * kq + r;
            if (co >= P.cout) continue;
#pragma unroll
            for (int t = 0; t < T; t++) {
                const size_t idx = PLANAR ? (size_t)co * 147 + pci * 49 + t * 7 + pkx : (size_t)co * cinT + (size_t)(cb + m) * T + t;
                out[idx] = acc[i][t][r];
            }
        }
}

// Per-channel pixel sums of dz (the bias gradient before the chain rule): block = (image, chunk) -> part[block][cout]; thread c sums
// its channel over the chunk's pixels in order.
__global__ __launch_bounds__(256) void k_dnb_bgrad(const float *dz, float *part, int cout, int npix, int chunk, int nchunk) {
    const int n = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int p0 = ch * chunk, p1 = min(npix, p0 + chunk);
    for (int c = threadIdx.x; c < cout; c += 256) {
        float s = 0.f;
        for (int p = p0; p < p1; p++) s += dz[((size_t)n * npix + p) * cout + c];
        part[(size_t)blockIdx.x * cout + c] = s;
    }
}

// Fixed-order reduction of nparts partials of E elements: acc[e] (= or +=) sum over p in order of part[p][e]
__global__ __launch_bounds__(256) void k_dnb_wsum(const float *part, float *acc, long long E, int nparts, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float s = 0.f;
    for (int p = 0; p < nparts; p++) s += part[(size_t)p * E + e];
    acc[e] = accumulate ? acc[e] + s : s;
}

// Chain rule through the BatchNorm fold of one layer (s = gamma / sqrt(var + eps), w' = s w, b' = beta - mean s (+ conv bias)).
// dwf / dbf: gradients of the folded weight [cout][K] and bias; raw w [cout][K], gamma / mean / var (NULL: no BatchNorm).
// Writes (each output may be NULL): dw = s dw', dcb = db', dbeta = db', dgamma = (sum_k dw' w - db' mean) / sqrt(var + eps).
// One thread per output channel (the sum runs in k order, in float64).
__global__ __launch_bounds__(256) void k_dnb_param_grad(const float *dwf, const float *dbf, const float *w, const float *g, const float *rm,
                                                        const float *rv, float *dw, float *dcb, float *dgamma, float *dbeta, int cout, int K) {
#pragma clang fp contract(off)
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= cout) return;
    const double r = g ? sqrt((double)rv[co] + 1e-5) : 1.0;
    const double s = g ? (double)g[co] / r : 1.0;
    const float *d = dwf + (size_t)co * K;
    if (dw)
        for (int k = 0; k < K; k++) dw[(size_t)co * K + k] = (float)((double)d[k] * s);
    if (dcb) dcb[co] = dbf[co];
    if (dbeta) dbeta[co] = dbf[co];
    if (dgamma) {
        double acc = 0.0;
        const float *wr = w + (size_t)co * K;
        for (int k = 0; k < K; k++) acc += (double)d[k] * (double)wr[k];
        dgamma[co] = (float)((acc - (double)dbf[co] * (double)rm[co]) / r);
    }
}

// Device re-fold of one layer from its raw parameters (the arithmetic of tcsfm_depthnet_load's host fold, float64, no contraction):
// writes the forward image w4 (conv1: the 7x7 grouping), the transposed image wt4 (NULL for conv1) and the folded bias.
// Entries for output channels >= cout are never written (zeroed once at allocation).  One thread per (co, ci, tap).
__global__ __launch_bounds__(256) void k_dnb_fold_params(const float *w, const float *cb, const float *g, const float *be, const float *rm,
                                                         const float *rv, dn_f4 *w4, dn_f4 *wt4, float *bias, int cout, int cin, int ks,
                                                         int coutp) {
#pragma clang fp contract(off)
    const int T = ks * ks;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)cout * cin * T) return;
    const int tap = (int)(e % T), ci = (int)((e / T) % cin), co = (int)(e / ((long long)T * cin));
    double sc = 1.0, sh = 0.0;
    if (g) { sc = (double)g[co] / sqrt((double)rv[co] + 1e-5); sh = (double)be[co] - (double)rm[co] * sc; }
    if (cb) sh += (double)cb[co] * sc;
    const float v = (float)((double)w[e] * sc);
    float *w4f = reinterpret_cast<float *>(w4);
    if (ks == 7) {
        const int ky = tap / 7, kx = tap % 7, combo = ci * 7 + ky, gg = combo >> 1, kq = 2 * (combo & 1) + (kx >> 2), t = kx & 3;
        w4f[((size_t)(gg * 4 + kq) * coutp + co) * 4 + t] = v;
    } else {
        const int c16n = cin / 16, c16 = ci >> 4, kq = (ci >> 2) & 3, t = ci & 3;
        w4f[((size_t)((tap * c16n + c16) * 4 + kq) * coutp + co) * 4 + t] = v;
        const int o16n = coutp / 16, o16 = co >> 4, oq = (co >> 2) & 3, ot = co & 3;
        reinterpret_cast<float *>(wt4)[((size_t)((tap * o16n + o16) * 4 + oq) * cin + ci) * 4 + ot] = v;
    }
    if (ci == 0 && tap == 0) bias[co] = (float)sh;
}

}  // namespace tc
