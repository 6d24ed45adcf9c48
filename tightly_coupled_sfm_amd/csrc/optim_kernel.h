// optim_kernel.h -- the optimiser step of the reference's weight-tuning loop (optimization_experiments/optimizer.py:211-214 builds
// torch.optim.Adam / SGD over the selected parameters, :266-268 calls step()) as ONE launch over all tensors of an optimiser.
//   * work items are (tensor, chunk) pairs from a table built when the optimiser is created (optim_host.h); the grid is capped and
//     strides over the table, so sixty encoder tensors or three hundred tiny ones cost one launch, not one each;
//   * memory bound (Adam: read p, g, m, v, write p, m, v = 28 B per element): a chunk is walked in groups of four floats that are
//     16-byte aligned IN THE PARAMETER's address space.  Parameters are views into the caller's storage (4-byte alignment only), so a
//     tensor has a scalar head of up to three elements, an aligned body of 16-byte accesses and a scalar tail.  The optimiser's own
//     arenas (moments, snapshot) are laid out with the parameter's 16-byte phase; a gradient with another phase is read with scalar
//     loads while p, m and v keep their 16-byte accesses;
//   * one thread owns an element: no atomics, no LDS, no scratch, bit-reproducible;
//   * Adam is torch.optim.Adam's single-tensor arithmetic (weight_decay = 0, amsgrad = False) in fp32 with contraction off:
//         m += (1 - b1) (g - m);   v = b2 v + (1 - b2) g g;   p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//     with bc1 = 1 - b1^t, bc2 = 1 - b2^t; the host computes 1 - b1, 1 - b2, lr / bc1 and sqrt(bc2) in double and rounds each once.
//     SGD is torch.optim.SGD(params) as the reference calls it: p -= lr g.
//   * the same walk copies parameters into the snapshot arena and back (tcsfm_optim_snapshot / tcsfm_optim_restore).
#pragma once
#include <hip/hip_runtime.h>

namespace tc {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 2048;          // elements of a work item: two groups of four per thread
constexpr int OPT_MAX_BLOCKS = 2048;

enum { OPT_ADAM = 0, OPT_SGD = 1, OPT_SNAPSHOT = 2, OPT_RESTORE = 3 };

// fixed per tensor for the optimiser's life.  m / v / snap (NULL when the arena does not exist) share p's 16-byte phase.
struct OptTensor {
    float *p, *m, *v, *snap;
    long long numel;
};
// per tensor and per step: the gradient (NULL: the tensor is skipped), a = lr / bc1 (SGD: lr), b = sqrt(bc2)
struct OptStep {
    const float *g;
    float a, b;
};
// chunk `chunk` of tensor `tensor`: the elements whose index i has (i + phase) / OPT_CHUNK == chunk, phase = p's offset in floats
// from the 16-byte boundary below it
struct OptWork {
    int tensor, chunk;
};
struct OptScalars {
    float one_m_b1, b2, one_m_b2, eps;
};

struct opt_f4 { float x, y, z, w; } __attribute__((aligned(16)));

template <int KIND>
__device__ __forceinline__ void opt_update(float &p, float g, float &m, float &v, const OptStep &S, const OptScalars &C) {
#pragma clang fp contract(off)
    if (KIND == OPT_ADAM) {
        m = m + C.one_m_b1 * (g - m);
        v = C.b2 * v + (C.one_m_b2 * g) * g;
        const float denom = sqrtf(v) / S.b + C.eps;
        p = p - S.a * (m / denom);
    } else {
        p = p - S.a * g;
    }
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void k_optim(const OptTensor *__restrict__ tensors, const OptStep *__restrict__ steps,
                                                       const OptWork *__restrict__ work, int nwork, OptScalars C) {
    for (int wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
        const OptWork wk = work[wi];
        const OptTensor T = tensors[wk.tensor];
        OptStep S = {nullptr, 0.f, 0.f};
        if (KIND == OPT_ADAM || KIND == OPT_SGD) {
            S = steps[wk.tensor];
            if (!S.g) continue;                     // p.grad is None: torch skips the tensor (block-uniform)
        }
        const int phase = (int)(((unsigned long long)T.p >> 2) & 3);
        const bool g_vec = (KIND == OPT_ADAM || KIND == OPT_SGD) && ((((unsigned long long)T.p ^ (unsigned long long)S.g) & 15) == 0);
#pragma unroll
        for (int r = 0; r < OPT_CHUNK / (4 * OPT_THREADS); r++) {
            // group q covers the elements i0 .. i0 + 3; i0 may be negative in the tensor's first group (the head)
            const long long q = (long long)wk.chunk * (OPT_CHUNK / 4) + r * OPT_THREADS + threadIdx.x;
            const long long i0 = q * 4 - phase;
            if (i0 >= T.numel) continue;
            if (i0 >= 0 && i0 + 4 <= T.numel) {     // aligned body: 16-byte accesses
                opt_f4 *pp = reinterpret_cast<opt_f4 *>(T.p + i0);
                if (KIND == OPT_SNAPSHOT) { *reinterpret_cast<opt_f4 *>(T.snap + i0) = *pp; continue; }
                if (KIND == OPT_RESTORE) { *pp = *reinterpret_cast<const opt_f4 *>(T.snap + i0); continue; }
                opt_f4 p = *pp, g, m = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
                if (g_vec) g = *reinterpret_cast<const opt_f4 *>(S.g + i0);
                else { g.x = S.g[i0]; g.y = S.g[i0 + 1]; g.z = S.g[i0 + 2]; g.w = S.g[i0 + 3]; }
                if (KIND == OPT_ADAM) { m = *reinterpret_cast<const opt_f4 *>(T.m + i0); v = *reinterpret_cast<const opt_f4 *>(T.v + i0); }
                opt_update<KIND>(p.x, g.x, m.x, v.x, S, C);
                opt_update<KIND>(p.y, g.y, m.y, v.y, S, C);
                opt_update<KIND>(p.z, g.z, m.z, v.z, S, C);
                opt_update<KIND>(p.w, g.w, m.w, v.w, S, C);
                *pp = p;
                if (KIND == OPT_ADAM) { *reinterpret_cast<opt_f4 *>(T.m + i0) = m; *reinterpret_cast<opt_f4 *>(T.v + i0) = v; }
            } else {                                // head or tail: element by element, inside [0, numel) only
                for (int k = 0; k < 4; k++) {
                    const long long i = i0 + k;
                    if (i < 0 || i >= T.numel) continue;
                    if (KIND == OPT_SNAPSHOT) { T.snap[i] = T.p[i]; continue; }
                    if (KIND == OPT_RESTORE) { T.p[i] = T.snap[i]; continue; }
                    float p = T.p[i], m = 0.f, v = 0.f;
                    if (KIND == OPT_ADAM) { m = T.m[i]; v = T.v[i]; }
                    opt_update<KIND>(p, S.g[i], m, v, S, C);
                    T.p[i] = p;
                    if (KIND == OPT_ADAM) { T.m[i] = m; T.v[i] = v; }
                }
            }
        }
    }
}

}  // namespace tc
