// window_loss_kernel.h -- the window loss of the reference's test-time optimisation (optimizer.py:47-86) as one reduction and its
// backward as one element-wise launch: gfx950 device code.
//
//   forward term   (:47-73)  argmin:   N1 / D1,  N1 = sum diff_min valid_min weight[0,b],  D1 = sum valid_min
//                            plain:    0.25 N1 / D1 over all S B maps
//   inverse term   (:74-79)  0.25 N2 / D2,  N2 = sum diff valid weight am,  D2 = sum valid am   (am = auto_mask under automasking, else 1)
//   depth consist. (:83-86)  w (1 - W1 / n)  and, with the inverse term,  w (1 - W2 / n)
//
// All maps are [S B, 1, H, W] float32, source-major (rows s B .. (s + 1) B), as solve_pose_iteratively emits them.  Every product and
// every sum is in double; the scalar is rounded to float once, at the store.  No atomics: a thread sums its pixels over the sources,
// a wave its lanes (shuffles), a workgroup its waves (LDS, wave order), and k_window_loss_final the workgroups' partials in index order.
// The grid depends on the shape only, so a repeat gives the same bits.  A thread takes four consecutive pixels of a plane (one float4
// load per map where the plane's address is 16-byte aligned, four scalar loads otherwise); the H W % 4 pixels left over go one per
// thread.  Ties of the min over the sources go to the LOWEST source index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tc {

constexpr int WL_MAXS = 4;          // sources per target, as everywhere else in the library
constexpr int WL_NSUM = 6;          // N1, D1, N2, D2, W1, W2
constexpr int WL_NSTAT = 7;         // ... and n, the element count of one side
constexpr int WL_UNITS = 2;         // units (of four pixels, or one tail pixel) per thread of the forward
constexpr int WL_CHUNK = 512;       // partial rows k_window_loss_final stages in LDS at a time
// the four pixels of a unit, unrolled (a tail unit's pixels 1 .. 3 are loaded as zeros: they add nothing to a sum and are not stored)
#define WL_EACH(k) _Pragma("unroll") for (int k = 0; k < 4; k++)

struct WindowLossParams {
    const float *f_diff, *f_valid, *f_weight, *f_ame;       // forward side; f_ame (auto_mask_error) is read under argmin && automask only
    const float *i_diff, *i_valid, *i_weight, *i_am;        // inverse side (read when inverse); i_am (auto_mask) under automask only
    int B, S, hw, argmin, automask, inverse;
    double w;                                               // depth-consistency weight, 0 = term off
};

// the pixels of unit u of a plane of hw pixels: units 0 .. hw / 4 - 1 are four pixels each, the units after them one tail pixel each
__device__ __forceinline__ int wl_unit(int u, int hw, int &p0) {
    const int n4 = hw >> 2;
    if (u < n4) { p0 = 4 * u; return 4; }
    p0 = 4 * n4 + (u - n4);
    return 1;
}
__device__ __forceinline__ int wl_units(int hw) { return (hw >> 2) + (hw & 3); }

// cnt (4 or 1) floats from p: one 16-byte load where the address allows
__device__ __forceinline__ void wl_load(const float *p, int cnt, float *v) {
    if (cnt == 4) {
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
        }
    } else {
        v[0] = p[0]; v[1] = v[2] = v[3] = 0.f;
    }
}
__device__ __forceinline__ void wl_store(float *p, int cnt, const float *v) {
    if (cnt == 4) {
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
    } else {
        p[0] = v[0];
    }
}

// the argmin form's per-pixel quantities of target b (optimizer.py:47-68): diff_min, its source (lowest index on a tie), valid_min
struct WlMin { double diff_min, valid_min; int arg; };
__device__ __forceinline__ void wl_min4(const WindowLossParams &P, int b, int p0, int cnt, WlMin *m) {
    double vs[4] = {0.0, 0.0, 0.0, 0.0};
    float dm[4], am[4];
    for (int s = 0; s < P.S; s++) {
        const size_t o = ((size_t)s * P.B + b) * P.hw + p0;
        float d[4], v[4], a[4];
        wl_load(P.f_diff + o, cnt, d);
        wl_load(P.f_valid + o, cnt, v);
        if (P.automask) wl_load(P.f_ame + o, cnt, a);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (s == 0) { dm[k] = d[k]; m[k].arg = 0; if (P.automask) am[k] = a[k]; }
            else {
                if (d[k] < dm[k]) { dm[k] = d[k]; m[k].arg = s; }        // strict: a tie keeps the lower index
                if (P.automask && a[k] < am[k]) am[k] = a[k];
            }
            vs[k] += (double)v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double vm = vs[k] < 0.0 ? 0.0 : (vs[k] > 1.0 ? 1.0 : vs[k]);      // clamp(sum, 0, 1)
        if (P.automask) vm *= (dm[k] < am[k]) ? 1.0 : 0.0;
        m[k].diff_min = (double)dm[k]; m[k].valid_min = vm;
    }
}

// grid (blocks per target, B), 256 threads; partial [gridDim.y * gridDim.x][WL_NSUM], row = blockIdx.y * gridDim.x + blockIdx.x
__global__ __launch_bounds__(256) void k_window_loss(WindowLossParams P, double *partial) {
    __shared__ double red[4][WL_NSUM];
    const int tid = threadIdx.x, b = blockIdx.y, nu = wl_units(P.hw);
    double acc[WL_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int u0 = blockIdx.x * 256 * WL_UNITS;
    for (int j = 0; j < WL_UNITS; j++) {
        const int u = u0 + j * 256 + tid;
        if (u >= nu) break;
        int p0;
        const int cnt = wl_unit(u, P.hw, p0);
        if (P.argmin) {
            WlMin m[4];
            wl_min4(P, b, p0, cnt, m);
            float w0[4];
            wl_load(P.f_weight + (size_t)b * P.hw + p0, cnt, w0);
            WL_EACH(k) { acc[0] += m[k].diff_min * m[k].valid_min * (double)w0[k]; acc[1] += m[k].valid_min; }
        }
        for (int s = 0; s < P.S; s++) {
            const size_t o = ((size_t)s * P.B + b) * P.hw + p0;
            float d[4], v[4], w[4], a[4];
            wl_load(P.f_weight + o, cnt, w);
            if (!P.argmin) { wl_load(P.f_diff + o, cnt, d); wl_load(P.f_valid + o, cnt, v); }
            WL_EACH(k) {
                if (!P.argmin) { acc[0] += (double)d[k] * (double)v[k] * (double)w[k]; acc[1] += (double)v[k]; }
                acc[4] += (double)w[k];
            }
            if (P.inverse) {
                wl_load(P.i_diff + o, cnt, d); wl_load(P.i_valid + o, cnt, v); wl_load(P.i_weight + o, cnt, w);
                if (P.automask) wl_load(P.i_am + o, cnt, a);
                WL_EACH(k) {
                    const double va = P.automask ? (double)v[k] * (double)a[k] : (double)v[k];
                    acc[2] += (double)d[k] * (double)w[k] * va; acc[3] += va; acc[5] += (double)w[k];
                }
            }
        }
    }
    // lanes -> wave (a fixed shuffle tree), waves -> workgroup (wave order)
#pragma unroll
    for (int i = 0; i < WL_NSUM; i++)
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
    if ((tid & 63) == 0)
        for (int i = 0; i < WL_NSUM; i++) red[tid >> 6][i] = acc[i];
    __syncthreads();
    if (tid < WL_NSUM) partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * WL_NSUM + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one workgroup: the nb partial rows added in index order (staged through LDS WL_CHUNK rows at a time, so the loads run in parallel
// and only the additions are serial), then the scalar.  stats = N1, D1, N2, D2, W1, W2, n.
__global__ __launch_bounds__(256) void k_window_loss_final(const double *partial, int nb, WindowLossParams P, double *stats, float *loss) {
    __shared__ double buf[WL_CHUNK * WL_NSUM];
    __shared__ double tot[WL_NSUM];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int r0 = 0; r0 < nb; r0 += WL_CHUNK) {
        const int nr = nb - r0 < WL_CHUNK ? nb - r0 : WL_CHUNK;
        for (int e = tid; e < nr * WL_NSUM; e += 256) buf[e] = partial[(size_t)r0 * WL_NSUM + e];
        __syncthreads();
        if (tid < WL_NSUM)
            for (int r = 0; r < nr; r++) s += buf[r * WL_NSUM + tid];
        __syncthreads();
    }
    if (tid < WL_NSUM) tot[tid] = s;
    __syncthreads();
    if (tid != 0) return;
    const double n = (double)P.S * (double)P.B * (double)P.hw;
    for (int i = 0; i < WL_NSUM; i++) stats[i] = tot[i];
    stats[6] = n;
    double L = (P.argmin ? 1.0 : 0.25) * tot[0] / tot[1];        // a zero denominator gives nan / inf, as the torch expression does
    if (P.inverse) L += 0.25 * tot[2] / tot[3];
    if (P.w != 0.0) {
        L += P.w * (1.0 - tot[4] / n);
        if (P.inverse) L += P.w * (1.0 - tot[5] / n);
    }
    *loss = (float)L;
}

// Backward: one element-wise launch, grid (blocks per target, B), one unit per thread.  It recomputes diff_min, the arg-min and
// valid_min from the inputs; each closed form is evaluated in double, multiplied by g_loss in double and rounded once.
//   argmin:  g_fwd_diff[s]   = [s = argmin] valid_min weight[0] / D1          g_fwd_weight[s] = [s = 0] diff_min valid_min / D1 - w / n
//   plain:   g_fwd_diff      = 0.25 valid weight / D1                         g_fwd_weight    = 0.25 diff valid / D1 - w / n
//   inverse: g_inv_diff      = 0.25 valid am weight / D2                      g_inv_weight    = 0.25 diff valid am / D2 - w / n
// Without the inverse term both inverse outputs are exact zeros.  A null output is not written.
struct WindowLossGradParams {
    WindowLossParams in;
    const double *stats;
    const float *g_loss;
    float *g_f_diff, *g_f_weight, *g_i_diff, *g_i_weight;
};

__global__ __launch_bounds__(256) void k_window_loss_bwd(WindowLossGradParams G) {
    const WindowLossParams &P = G.in;
    const int u = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (u >= wl_units(P.hw)) return;
    int p0;
    const int cnt = wl_unit(u, P.hw, p0);
    const double g = (double)*G.g_loss, D1 = G.stats[1], D2 = G.stats[3];
    const double dc = P.w != 0.0 ? P.w / G.stats[6] : 0.0;
    const bool fwd = G.g_f_diff != nullptr || G.g_f_weight != nullptr;
    WlMin m[4];
    float w0[4];
    if (P.argmin && fwd) {
        wl_min4(P, b, p0, cnt, m);
        if (G.g_f_diff != nullptr) wl_load(P.f_weight + (size_t)b * P.hw + p0, cnt, w0);
    }
    for (int s = 0; s < P.S; s++) {
        const size_t o = ((size_t)s * P.B + b) * P.hw + p0;
        float d[4], v[4], w[4], a[4], out[4];
        if (fwd && P.argmin) {
            if (G.g_f_diff != nullptr) {
                WL_EACH(k) out[k] = (float)(g * (m[k].arg == s ? m[k].valid_min * (double)w0[k] / D1 : 0.0));
                wl_store(G.g_f_diff + o, cnt, out);
            }
            if (G.g_f_weight != nullptr) {
                WL_EACH(k) out[k] = (float)(g * ((s == 0 ? m[k].diff_min * m[k].valid_min / D1 : 0.0) - dc));
                wl_store(G.g_f_weight + o, cnt, out);
            }
        } else if (fwd) {
            wl_load(P.f_valid + o, cnt, v);
            if (G.g_f_diff != nullptr) {
                wl_load(P.f_weight + o, cnt, w);
                WL_EACH(k) out[k] = (float)(g * (0.25 * ((double)v[k] * (double)w[k]) / D1));
                wl_store(G.g_f_diff + o, cnt, out);
            }
            if (G.g_f_weight != nullptr) {
                wl_load(P.f_diff + o, cnt, d);
                WL_EACH(k) out[k] = (float)(g * (0.25 * ((double)d[k] * (double)v[k]) / D1 - dc));
                wl_store(G.g_f_weight + o, cnt, out);
            }
        }
        if (G.g_i_diff == nullptr && G.g_i_weight == nullptr) continue;
        if (!P.inverse) {
            WL_EACH(k) out[k] = 0.f;
            if (G.g_i_diff != nullptr) wl_store(G.g_i_diff + o, cnt, out);
            if (G.g_i_weight != nullptr) wl_store(G.g_i_weight + o, cnt, out);
            continue;
        }
        wl_load(P.i_valid + o, cnt, v);
        if (P.automask) wl_load(P.i_am + o, cnt, a);
        double va[4];
        WL_EACH(k) va[k] = P.automask ? (double)v[k] * (double)a[k] : (double)v[k];
        if (G.g_i_diff != nullptr) {
            wl_load(P.i_weight + o, cnt, w);
            WL_EACH(k) out[k] = (float)(g * (0.25 * (va[k] * (double)w[k]) / D2));
            wl_store(G.g_i_diff + o, cnt, out);
        }
        if (G.g_i_weight != nullptr) {
            wl_load(P.i_diff + o, cnt, d);
            WL_EACH(k) out[k] = (float)(g * (0.25 * ((double)d[k] * va[k]) / D2 - dc));
            wl_store(G.g_i_weight + o, cnt, out);
        }
    }
}

}  // namespace tc
