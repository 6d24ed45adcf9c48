// posenet_wgrad_kernel.h -- the PoseNet's gradient with respect to its PARAMETERS (the reference's optimize_pose_weights_all mode,
// optimization_experiments/optimizer.py:187-189).  The backward walk of posenet_grad_kernel.h already produces, per layer, the
// masked activation gradient g = da [a > 0] and the pre-activation gradient dz; the kernels here turn them into parameter gradients:
//   d beta_c  = sum_{n,p} g,   d gamma_c = sum_{n,p} g x^      (x^ = (raw - mean) rstd from the taped mean_rstd: gamma may be 0)
//   d bias_c  = sum_{n,p} dz
//   G^[co][ci][ky][kx] = sum_{n,p} dz[n,p,co] a_{l-1}[n, 2 p + k - pad, ci]     (gradient of the STANDARDISED weight)
//   dw_i = (G^_i - mean(G^)) / (s + 1e-5) - w^_i (sum_j G^_j w^_j) / ((n - 1) s)   (conv2d_wn's chain rule, per filter)
//   d head_w[j][c] = (0.01 / npix) sum_n d_pose[n][j] sum_p a_7[n,p,c],   d head_b[j] = 0.01 sum_n d_pose[n][j]
// The weight gradient is an implicit GEMM on v_mfma_f32_16x16x4_f32 with K = the N npix output pixels of the call, dealt in contiguous
// parts to workgroups; its input operand, which the forward never writes, is formed ON LOAD: relu(raw scale + shift) of the previous
// layer's taped values through pn_act (the device function the ReLU decisions are taken with), layer 1 the caller's planar images
// normalised (x - 0.45) / 0.22.  A lane reads one channel of 4 pixels per tap and step, its (scale, shift) pair comes from L1: a
// materialised activation would cost a write and a read of every map to save one fused multiply-add and one max per load.
// No float atomics; partial sums are combined in a fixed order (waves through LDS in wave order, parts ascending in double).
#pragma once
#include <hip/hip_runtime.h>
#include "posenet_grad_kernel.h"

namespace tc {

// ---- per-channel sums over all images and pixels ----------------------------------------------------------------------------------
// mode 0: (sum g, sum g x^) from da (BEFORE k_pnb_dz overwrites it); mode 1: sum dz (AFTER it; P.da then holds dz).
// grid = (cout / 16, parts <= 16384 / cout); a workgroup = 16 channels x 16 row lanes; rows r = n npix + p of its part strided over the row lanes,
// double sums, the 16 row lanes added in lane order.  part[(blockIdx.y * cout + c) * 2 + {0, 1}]
__global__ __launch_bounds__(256) void k_pnw_chan(PnbNormParams P, double *part, long long rows_per_part, int mode) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), rl = threadIdx.x >> 4, cg = P.cout / 16, g = c / cg;
    const long long R = (long long)P.N * P.npix;
    const long long r0 = (long long)blockIdx.y * rows_per_part, r1 = r0 + rows_per_part < R ? r0 + rows_per_part : R;
    double s1 = 0.0, s2 = 0.0;
    for (long long r = r0 + rl; r < r1; r += 16) {
        const size_t i = (size_t)r * P.cout + c;
        if (mode) { s1 += (double)P.da[i]; continue; }
        const int n = (int)(r / P.npix);
        const float *scsh = P.scsh + ((size_t)n * P.cout + c) * 2;
        const float mean = P.mr[((size_t)n * 16 + g) * 2], rstd = P.mr[((size_t)n * 16 + g) * 2 + 1];
        const float z = P.raw[i];
        const float gg = pn_act(z, scsh[0], scsh[1]) > 0.f ? P.da[i] : 0.f;
        const float xh = (z - mean) * rstd;
        s1 += (double)gg; s2 += (double)gg * (double)xh;
    }
    __shared__ double red[16][16][2];
    red[rl][threadIdx.x & 15][0] = s1; red[rl][threadIdx.x & 15][1] = s2;
    __syncthreads();
    if (rl == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < 16; k++) { t1 += red[k][threadIdx.x][0]; t2 += red[k][threadIdx.x][1]; }
        part[((size_t)blockIdx.y * P.cout + c) * 2] = t1; part[((size_t)blockIdx.y * P.cout + c) * 2 + 1] = t2;
    }
}

// one workgroup per channel: the parts strided over the threads (ascending per thread), then the tree of k_pn_stats in LDS -> out0[c]
// (slot 0), out1[c] (slot 1); either may be null
__global__ __launch_bounds__(256) void k_pnw_chan_sum(const double *part, float *out0, float *out1, int cout, int parts) {
    const int c = blockIdx.x, tid = threadIdx.x;
    __shared__ double r1[256], r2[256];
    double t1 = 0.0, t2 = 0.0;
    for (int p = tid; p < parts; p += 256) { t1 += part[((size_t)p * cout + c) * 2]; t2 += part[((size_t)p * cout + c) * 2 + 1]; }
    r1[tid] = t1; r2[tid] = t2; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) { r1[tid] += r1[tid + o]; r2[tid] += r2[tid + o]; } __syncthreads(); }
    if (tid == 0) {
        if (out0) out0[c] = (float)r1[0];
        if (out1) out1[c] = (float)r2[0];
    }
}

// ---- weight-gradient partials ------------------------------------------------------------------------------------------------------
// M = 16 MB output channels, N = 16 input channels, K = the rows r = n npix + p of this part, 4 per step, the steps dealt to the 4
// waves in turn; one accumulator per tap of the workgroup:
//   PNW_ALL    every tap (3 x 3: T = 9)
//   PNW_ROW    one kernel row ky per workgroup (5 x 5: T = 5 kx; 25 accumulators per channel block would leave one wave per SIMD)
//   PNW_FIRST  layer 1 on the planar images: N = 16 of the 48 padded (ci, kx) combinations (42 valid), T = 7 ky
// The loop is latency-bound (a lane's T scalar loads feed T matrix instructions): the loads of U consecutive steps are issued
// together.  part[blockIdx.x][co][ci][ky][kx] (the reference's layout).
// grid = (parts, cin / 16 (PNW_ROW: x KS; PNW_FIRST: 3), cout / (16 MB)).
struct PnWgradParams {
    const float *dz;        // [N][npix][cout]
    const float *x;         // previous layer's taped raw output [N][ih][iw][cin] (PNW_FIRST: the images [N][6][ih][iw], planar)
    const float *scsh;      // previous layer's taped [N][cin][2] (PNW_FIRST: unused)
    float *part;
    long long rows, rows_per_part;
    int cin, cout, ih, iw, oh, ow, pad;
};
enum { PNW_ALL = 0, PNW_ROW = 1, PNW_FIRST = 2 };

template <int KS, int MB, int MODE>
__global__ __launch_bounds__(256) void k_pnw_wgrad(PnWgradParams P) {
    constexpr int T = MODE == PNW_ALL ? KS * KS : KS;
    constexpr int U = MB * T >= 16 ? 2 : 4;
    constexpr bool FIRST = MODE == PNW_FIRST;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int npix = P.oh * P.ow;
    const long long r0 = (long long)blockIdx.x * P.rows_per_part, r1 = r0 + P.rows_per_part < P.rows ? r0 + P.rows_per_part : P.rows;
    const int cb = (MODE == PNW_ROW ? blockIdx.y / KS : blockIdx.y) * 16, wky = MODE == PNW_ROW ? blockIdx.y % KS : 0;
    const int cob = blockIdx.z * 16 * MB;
    const int combo = cb + m;                               // PNW_FIRST: 7 ci + kx
    const bool cok = !FIRST || combo < 6 * KS;
    const int pci = FIRST ? (cok ? combo / KS : 0) : cb + m, pkx = FIRST ? (cok ? combo - KS * (combo / KS) : 0) : 0;
    pn_f4 acc[MB][T];
#pragma unroll
    for (int i = 0; i < MB; i++)
#pragma unroll
        for (int t = 0; t < T; t++) acc[i][t] = (pn_f4){0.f, 0.f, 0.f, 0.f};
    // this lane's row of the current step as (image, pixel): walked, not divided (a step advances every lane by 16 rows)
    long long r = r0 + 4 * wave + kq;
    int n = (int)(r / npix), p = (int)(r - (long long)n * npix);
    for (long long s = r0 + 4 * wave; s < r1; s += 16 * U) {
        float a[U][MB], b[U][T];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool pv = r < r1;
            const int oy = p / P.ow, ox = p - oy * P.ow;
#pragma unroll
            for (int i = 0; i < MB; i++) a[u][i] = pv ? P.dz[(size_t)r * P.cout + cob + 16 * i + m] : 0.f;
            if (FIRST) {
                const float *xb = P.x + ((size_t)(pv ? n : 0) * 6 + pci) * P.ih * P.iw;
                const int ix = ox * 2 + pkx - P.pad;
                const bool xok = pv && cok && ix >= 0 && ix < P.iw;
#pragma unroll
                for (int ky = 0; ky < KS; ky++) {
                    const int iy = oy * 2 + ky - P.pad;
                    const bool ok = xok && iy >= 0 && iy < P.ih;
                    const float v = xb[ok ? (size_t)iy * P.iw + ix : 0];
                    b[u][ky] = ok ? (v - 0.45f) * (1.f / 0.22f) : 0.f;          // the forward's own expression (k_pn_conv1)
                }
            } else {
                const int nn = pv ? n : 0;
                const float *xb = P.x + (size_t)nn * P.ih * P.iw * P.cin + pci;
                const float sc = P.scsh[((size_t)nn * P.cin + pci) * 2], sh = P.scsh[((size_t)nn * P.cin + pci) * 2 + 1];
#pragma unroll
                for (int t = 0; t < T; t++) {
                    const int ky = MODE == PNW_ROW ? wky : t / KS, kx = MODE == PNW_ROW ? t : t - KS * (t / KS);
                    const int iy = oy * 2 + ky - P.pad, ix = ox * 2 + kx - P.pad;
                    const bool ok = pv && iy >= 0 && iy < P.ih && ix >= 0 && ix < P.iw;
                    const float v = xb[ok ? ((size_t)iy * P.iw + ix) * P.cin : 0];
                    b[u][t] = ok ? pn_act(v, sc, sh) : 0.f;
                }
            }
            r += 16; p += 16;
            while (p >= npix) { p -= npix; n++; }
        }
        __builtin_amdgcn_sched_barrier(0);       // the loads of all U steps are issued before the first matrix instruction
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int i = 0; i < MB; i++)
#pragma unroll
                for (int t = 0; t < T; t++) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], b[u][t], acc[i][t], 0, 0, 0);
    }
    // waves 1, 2, 3 hand their accumulators to wave 0 one after the other (one wave's worth of LDS; fixed order)
    __shared__ pn_f4 red[MB * T][64];
    for (int w = 1; w < 4; w++) {
        if (wave == w)
#pragma unroll
            for (int i = 0; i < MB; i++)
#pragma unroll
                for (int t = 0; t < T; t++) red[i * T + t][lane] = acc[i][t];
        __syncthreads();
        if (wave == 0)
#pragma unroll
            for (int i = 0; i < MB; i++)
#pragma unroll
                for (int t = 0; t < T; t++) acc[i][t] += red[i * T + t][lane];
        __syncthreads();
    }
    if (wave > 0 || !cok) return;
    // C layout: column (input channel / combination) = m, row (output channel) = 4 kq + reg
    const int cinT = P.cin * KS * KS;
    float *out = P.part + (size_t)blockIdx.x * P.cout * cinT;
#pragma unroll
    for (int i = 0; i < MB; i++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int co = cob + 16 * i + 4 * kq + rr;
#pragma unroll
            for (int t = 0; t < T; t++) {
                const int tap = FIRST ? t * KS + pkx : (MODE == PNW_ROW ? wky * KS + t : t);
                out[(size_t)co * cinT + (size_t)pci * KS * KS + tap] = acc[i][t][rr];
            }
        }
}

// parts -> G^: one thread per element, parts ascending, in double, rounded to fp32
__global__ __launch_bounds__(256) void k_pnw_psum(const float *part, float *g, long long E, int parts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double s = 0.0;
    for (int p = 0; p < parts; p++) s += (double)part[(size_t)p * E + e];
    g[e] = (float)s;
}

// ---- conv2d_wn's chain rule, one workgroup per filter ------------------------------------------------------------------------------
// w: the RAW weights [cout][n] of the load; dw [cout][n]: G^ on entry (k_pnw_psum), the raw weight's gradient on exit.  The filter-wide
// sums (mean and unbiased deviation of w, sum G^, sum G^ w^) in double, as k_pn_prep's.
__global__ __launch_bounds__(256) void k_pnw_wstd(const float *w, float *dw, int n) {
    const int co = blockIdx.x, tid = threadIdx.x;
    const float *wc = w + (size_t)co * n;
    float *dc = dw + (size_t)co * n;
    __shared__ double red[256];
    auto total = [&](double v) {
        __syncthreads();
        red[tid] = v; __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        return red[0];
    };
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)wc[i];
    const double mean = total(s) / n;
    double q = 0.0;
    for (int i = tid; i < n; i += 256) { const double d = (double)wc[i] - mean; q += d * d; }
    const double sd = sqrt(total(q) / (n - 1)), inv = 1.0 / (sd + 1e-5);
    double sg = 0.0, sgw = 0.0;
    for (int i = tid; i < n; i += 256) { const double g = (double)dc[i]; sg += g; sgw += g * (((double)wc[i] - mean) * inv); }
    const double gmean = total(sg) / n;
    const double k2 = total(sgw) / ((double)(n - 1) * sd);
    for (int i = tid; i < n; i += 256) dc[i] = (float)(((double)dc[i] - gmean) * inv - (((double)wc[i] - mean) * inv) * k2);
}

// ---- head --------------------------------------------------------------------------------------------------------------------------
// grid = 16 workgroups of 16 channels x 16 image lanes: feat_n = sum_p a_7[n,p,c] (p ascending, double), the images n strided over the
// image lanes, the lanes added in lane order: d head_w[j][c] = (0.01 / npix) sum_n d_pose[n][j] feat_n.  Workgroup 0, threads 0..5:
// d head_b[j] = 0.01 sum_n d_pose[n][j] (n ascending).  Either output may be null.
__global__ __launch_bounds__(256) void k_pnw_head(const float *raw, const float *scsh, const float *d_pose, float *dw, float *db, int N, int npix) {
    const int cl = threadIdx.x & 15, nl = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
    __shared__ double red[16][16][6];
    if (dw) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int n = nl; n < N; n += 16) {
            const float sc = scsh[((size_t)n * 256 + c) * 2], sh = scsh[((size_t)n * 256 + c) * 2 + 1];
            double f = 0.0;
            for (int p = 0; p < npix; p++) f += (double)pn_act(raw[((size_t)n * npix + p) * 256 + c], sc, sh);
#pragma unroll
            for (int j = 0; j < 6; j++) acc[j] += (double)d_pose[n * 6 + j] * f;
        }
#pragma unroll
        for (int j = 0; j < 6; j++) red[nl][cl][j] = acc[j];
        __syncthreads();
        if (nl < 6) {        // thread (cl, j = nl)
            double t = 0.0;
            for (int k = 0; k < 16; k++) t += red[k][cl][nl];
            dw[nl * 256 + c] = (float)(t * (0.01 / (double)npix));
        }
    }
    if (db && blockIdx.x == 0 && threadIdx.x < 6) {
        double s = 0.0;
        for (int n = 0; n < N; n++) s += (double)d_pose[n * 6 + threadIdx.x];
        db[threadIdx.x] = (float)(0.01 * s);
    }
}

// out[i] = v (the NULL conventions of the device load: gamma 1, bias / beta 0)
__global__ __launch_bounds__(256) void k_pnw_fill(float *out, int n, float v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

}  // namespace tc
