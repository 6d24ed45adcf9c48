// 8-bit camera frames -> the planar float32 frames every other kernel reads (include/tcsfm.h: tcsfm_sequence_frame_format,
// tcsfm_frames_from_u8).  The reference does this on the host (utils/custom_transforms.py:62-76 ArrayToTensor: transpose to
// C x H x W, .float() / 255); here the bytes cross PCIe and one launch per chunk of frames turns them into floats on the device.
//
// value: float(b) / 255.0f, a TRUE fp32 division (correctly rounded: the build has no fast-math) -- float(b) * (1.0f / 255) differs
// from it for 126 of the 256 byte values.
//
// work split: blockIdx.y = frame, a thread owns 4 consecutive pixels p .. p+3 (p a multiple of 4) of it and all three channels.
//   loads   HWC: the 12 bytes of the 4 pixels start at byte 3 p = 12 t of the frame -> three 32-bit loads when the FRAME's address is
//           4-byte aligned.  CHW: channel c's 4 bytes start at c H W + p -> one 32-bit load when that PLANE's address is 4-byte
//           aligned.  Both are per-frame facts (the frames of a batch are 3 H W bytes apart: misaligned when H W % 4 != 0; an
//           operator's src may sit anywhere), wave-uniform, and decided from the address itself.  Otherwise: byte loads.
//   stores  VST (chosen by the launcher): every plane (dst + (3 f + c) H W floats) is 16-byte aligned -- H W % 4 == 0 and aligned
//           bases -- so there is no tail and a thread writes one 16-byte store per plane.  Otherwise scalar stores, and the last
//           H W % 4 pixels of a frame (n < 4) are a scalar tail.  (A template parameter, not a branch on the address: with both
//           forms in one body the compiler merges them and splits the 16-byte store.)
//   mirror  the first `nm` frames of a launch are also written to dst2 (the ring's mirror slots): a chunk costs ONE launch.
// Every access is inside [src, src + 3 H W N) / [dst, dst + 3 H W N) / [dst2, dst2 + 3 H W nm): a wide access is taken only with
// n == 4, i.e. p + 3 < H W.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <bool HWC, bool VST>
__global__ __launch_bounds__(256) void k_frames_u8(const uint8_t *__restrict__ src, float *__restrict__ dst, float *__restrict__ dst2, int nm,
                                                   long long hw) {
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= hw) return;
    const int f = blockIdx.y;
    const int n = VST ? 4 : (hw - p < 4 ? (int)(hw - p) : 4);
    const uint8_t *s = src + (size_t)f * 3 * (size_t)hw;
    unsigned b[3][4];                                     // [channel][pixel]
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) b[c][i] = 0;
    if (HWC) {
        const uint8_t *q = s + 3 * (size_t)p;
        if (n == 4 && ((uintptr_t)s & 3) == 0) {
            const uint32_t *qw = (const uint32_t *)q;
            const uint32_t w[3] = {qw[0], qw[1], qw[2]};
#pragma unroll
            for (int k = 0; k < 12; k++) b[k % 3][k / 3] = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n) {
#pragma unroll
                    for (int c = 0; c < 3; c++) b[c][i] = q[3 * i + c];
                }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t *q = s + (size_t)c * (size_t)hw + (size_t)p;
            if (n == 4 && ((uintptr_t)q & 3) == 0) {
                const uint32_t w = *(const uint32_t *)q;
#pragma unroll
                for (int i = 0; i < 4; i++) b[c][i] = (w >> (8 * i)) & 255u;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n) b[c][i] = q[i];
            }
        }
    }
    float *d = dst + (size_t)f * 3 * (size_t)hw + (size_t)p;
    float *m = (dst2 && f < nm) ? dst2 + (size_t)f * 3 * (size_t)hw + (size_t)p : nullptr;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float4 v;
        v.x = (float)b[c][0] / 255.0f; v.y = (float)b[c][1] / 255.0f; v.z = (float)b[c][2] / 255.0f; v.w = (float)b[c][3] / 255.0f;
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float *o = t == 0 ? d : m;
            if (!o) continue;
            o += (size_t)c * (size_t)hw;
            if (VST) {
                *(float4 *)o = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n) o[i] = e[i];
            }
        }
    }
}

// N frames of `hwc ? [N,H,W,3] : [N,3,H,W]` bytes at src -> [N,3,H,W] floats at dst (and the first nm of them at dst2, when given)
static inline hipError_t launch_frames_u8(hipStream_t stream, bool hwc, int N, const uint8_t *src, float *dst, float *dst2, int nm, size_t hw) {
    const unsigned gx = (unsigned)(((hw + 3) / 4 + 255) / 256);
    for (int f0 = 0; f0 < N; f0 += 65535) {               // (gridDim.y is a 16-bit quantity)
        const int nf = N - f0 < 65535 ? N - f0 : 65535;
        const int nmf = dst2 && nm > f0 ? (nm - f0 < nf ? nm - f0 : nf) : 0;
        const uint8_t *s = src + (size_t)f0 * 3 * hw;
        float *d = dst + (size_t)f0 * 3 * hw, *d2 = nmf ? dst2 + (size_t)f0 * 3 * hw : nullptr;
        const bool vst = hw % 4 == 0 && (((uintptr_t)d | (uintptr_t)d2) & 15) == 0;
        auto k = hwc ? (vst ? k_frames_u8<true, true> : k_frames_u8<true, false>) : (vst ? k_frames_u8<false, true> : k_frames_u8<false, false>);
        hipLaunchKernelGGL(k, dim3(gx, (unsigned)nf), dim3(256), 0, stream, s, d, d2, nmf, (long long)hw);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}
