// Camera-size 8-bit frames -> the H x W frames the solver and the networks read, with Pillow's bytes (include/tcsfm.h:
// tcsfm_sequence_frame_source, tcsfm_resize_u8).  The reference shrinks every frame on the host with PIL's
// Image.resize((W, H), Image.ANTIALIAS) -- Lanczos, support 3 source-scale pixels (data/scannet_test_loader.py:157-170 at run time,
// data/create_kitti_odometry_data.py:56-65 and data/create_kitti_eigen_data.py:30-35 offline); the networks were trained on exactly
// those images.  Pillow's 8-bit resize is integer arithmetic, so the kernel returns its bytes exactly:
//   coefficients  22-bit fixed point, made on the host in double (resize_coeffs.h), one table per axis, cached on the handle
//   a pass        acc = (1 << 21) + sum byte[xmin + x] * k[x] in int32 (sum |k| < 1.5 * 2^22, so |acc| < 2^31), byte = clamp(acc >> 22, 0, 255)
//   two passes    horizontal, then vertical ON THE BYTES of the horizontal one; a pass whose in == out is skipped (a plain copy)
//
// work split: one launch per chunk of frames, both passes in it.  blockIdx = (tile column, tile row, frame); a workgroup of 256 owns
//   RZ_TW x RZ_TH = 32 x 32 output pixels, all three channels.  Coefficient windows move monotonically with the output index, so the
//   tile reads the source rectangle [xmin(first col), xmax(last col)) x [ymin(first row), ymax(last row)) and nothing else.
//   1. the tile's slices of the two tables go to LDS (a row of ksize ints per output index; ksize is odd: conflict-free by lane)
//   2. horizontal: the rectangle's rows, RZ_RB = 24 at a time, are STAGED in LDS -- 32 lanes per row, three rows per thread; the bytes
//      between the first and the last 4-byte boundary of the row segment go as 32-bit loads, the 0-3 bytes before and after as byte
//      loads (decided from the address: a frame, a row, a plane or an operator's src may sit at any byte; the LDS copy keeps the
//      address's low two bits, so both sides of a 32-bit move are aligned).  The loads go to registers first (rz_load_row) and to LDS
//      afterwards (rz_store_row): a batch's loads are all in flight together, and the NEXT batch's are issued before this batch is
//      convolved.  Then thread (row, column) convolves its three channels from the staged bytes and writes the pixel as one word of
//      the intermediate image s_mid[row][column] = r | g << 8 | b << 16.  It exists in LDS only.
//   3. vertical: thread (row, column) of the tile, four rows each, convolves down s_mid and writes the output: (float)b / 255.0f -- the
//      true division k_frames_u8 makes -- to the planar float frames (and, for the first nm frames, to dst2: the ring's mirror slots), or
//      the byte in the source's layout.  Lanes run along a row: float stores are 128-byte runs.
//   A source byte is fetched once per tile that reaches it: the tiles' rectangles overlap by the filter's window (6 source-scale pixels
//   in 32 + 6 per axis, 19 % at any ratio >= 1); the next tile's fetch of the halo hits L2.
//
// LDS (160 KiB per CU, gfx950): s_mid 300 rows x 128 B = 38 400, staging 24 x 924 = 22 176, tables 2 x 32 x 49 x 4 = 12 544, bounds 512:
//   73 632 B per workgroup, two workgroups (8 waves) per CU; 95 VGPRs (interleaved) / 127 (planar: three segments per row in flight),
//   no scratch.  A 4-frame KITTI chunk is 480 workgroups, 1.9 per CU: the LDS does not limit it.  A 64 x 32 tile would halve the column
//   halo but needs 77 KiB for s_mid alone at the largest ratio and leaves 60 workgroups per KITTI frame -- fewer than the chip's 256 CUs
//   on a 4-frame chunk; 32 x 32 gives 120 per frame.
// measured (rocprofv3 kernel trace, 4 interleaved 1241 x 376 frames -> 640 x 192 floats): 24.5 us per launch against a byte bound of
//   1.8 us (5.6 MB read + 5.9 MB written at 6.3 TB/s): the kernel is bound by its own instruction stream -- 13 taps per output and pass,
//   each a coefficient read and three byte reads from LDS -- not by memory.  Tried and measured on the same chunk: 8-row batches with
//   load -> store -> barrier in turn 26.1 us, the register-staged pipeline above 24.9, the packed s_mid (one LDS read per vertical tap
//   instead of three) 24.5, uniform ksize-long tap loops unrolled by four 25.6, one unaligned 32-bit LDS read per interleaved pixel
//   40.4.  What bounds the remaining time has not been isolated.
//
// limits (resize_refusal below; the setter and the operator refuse beyond them with TCSFM_E_ARG):
//   in <= 8 * out per axis.  Then ksize <= 2 * 24 + 1 = 49 = RZ_MAX_KSIZE, and a tile's 32 outputs reach at most 31 * 8 + 2 * 24 + 1 = 297
//   source rows / columns (first window's start >= c0 - 24.5, last window's end <= c31 + 24.5, c31 - c0 = 31 * 8): <= RZ_MAX_SPAN = 304
//   columns and <= RZ_MAX_ROWS = 300 rows.  Upscaling (in < out) has ksize 7 and reaches <= 38.  Sides: 1 .. 32768.
//   The table builder measures every tile's rectangle against these constants and refuses a table that does not fit, so the kernel's LDS
//   indices are bounded by what the host checked, not by the argument above.
// Every global access is inside [src, src + 3 h w N) / dst's N frames / dst2's nm frames: a staged row segment is [a, a + len) exactly,
// and its 32-bit loads cover only whole words inside it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "resize_coeffs.h"

#define RZ_TW 32
#define RZ_TH 32
#define RZ_RB 24                      // source rows staged at a time: 256 threads = 8 row groups x 32 lanes, 3 rows each
#define RZ_MAX_KSIZE 49
#define RZ_MAX_SPAN 304               // source columns of a tile
#define RZ_MAX_ROWS 300               // source rows of a tile
#define RZ_SUB (RZ_MAX_SPAN + 4)      // staged bytes of one plane's row segment: span + up to 3 bytes of address offset, a multiple of 4
#define RZ_ROWB (3 * RZ_SUB)          // staged bytes of a row: three plane segments, or one interleaved segment of 3 * span (+ 3)
#define RZ_MAX_RATIO 8
#define RZ_MAX_SIDE 32768

struct ResizeParams {
    const uint8_t *src;               // N frames of h x w, interleaved or planar
    void *dst;                        // float [N,3,H,W], or bytes in the source's layout
    float *dst2;                      // float output only: the first nm frames again (NULL: none)
    int nm;
    int sh, sw, H, W;
    int hp, vp;                       // pass present (in != out)
    int ksh, ksv;
    const int *bh, *kh, *bv, *kv;     // bounds [out][2] = {first tap, taps}, coefficients [out][ksize]
};

// The row segment [a, a + len) -> LDS at l + (a & 3) .. (l is 4-byte aligned), by the 32 lanes of a row group, in two steps so that the
// loads of a whole batch are in flight before anything waits for one: rz_load_row issues lane's loads into registers (NW words: the
// 32-bit words between the segment's first and last 4-byte boundary, lane, lane + 32, ...; one byte before them and one behind),
// rz_store_row puts them into LDS.  len <= 128 NW (the launcher's limits: 3 * RZ_MAX_SPAN <= 128 * 8, RZ_MAX_SPAN <= 128 * 3).
template <int NW>
struct RzRow {
    uint32_t w[NW];
    uint8_t hb, tb;
};

struct RzSplit {
    int head, body, done, tail;
    __device__ __forceinline__ RzSplit(const uint8_t *a, int len) {
        head = (int)((4 - ((uintptr_t)a & 3)) & 3);
        if (head > len) head = len;
        body = (len - head) >> 2; done = head + 4 * body; tail = len - done;
    }
};

template <int NW>
__device__ __forceinline__ void rz_load_row(const uint8_t *__restrict__ a, int len, int lane, RzRow<NW> &R) {
    const RzSplit s(a, len);
    const uint32_t *aw = (const uint32_t *)(a + s.head);   // (aligned whenever body > 0)
#pragma unroll
    for (int i = 0; i < NW; i++) R.w[i] = lane + 32 * i < s.body ? aw[lane + 32 * i] : 0u;
    R.hb = lane < s.head ? a[lane] : (uint8_t)0;
    R.tb = lane < s.tail ? a[s.done + lane] : (uint8_t)0;
}

template <int NW>
__device__ __forceinline__ void rz_store_row(const uint8_t *a, int len, int lane, const RzRow<NW> &R, uint8_t *l) {
    const RzSplit s(a, len);
    uint8_t *d = l + ((uintptr_t)a & 3);
    uint32_t *dw = (uint32_t *)(d + s.head);
#pragma unroll
    for (int i = 0; i < NW; i++)
        if (lane + 32 * i < s.body) dw[lane + 32 * i] = R.w[i];
    if (lane < s.head) d[lane] = R.hb;
    if (lane < s.tail) d[s.done + lane] = R.tb;
}

__device__ __forceinline__ int rz_clip8(int acc) {
    const int v = acc >> 22;                               // (arithmetic)
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <bool HWC, bool F32>
__global__ __launch_bounds__(256) void k_resize_u8(ResizeParams P) {
    __shared__ uint32_t s_stage_w[RZ_RB * RZ_ROWB / 4];
    __shared__ uint32_t s_mid[RZ_MAX_ROWS * RZ_TW];       // the intermediate image: a pixel per word, r | g << 8 | b << 16
    __shared__ int s_kh[RZ_TW * RZ_MAX_KSIZE], s_kv[RZ_TH * RZ_MAX_KSIZE];
    __shared__ int s_bh[RZ_TW * 2], s_bv[RZ_TH * 2];
    uint8_t *s_stage = (uint8_t *)s_stage_w;
    const int t = threadIdx.x, f = blockIdx.z;
    const int xx0 = blockIdx.x * RZ_TW, yy0 = blockIdx.y * RZ_TH;
    const int tw = P.W - xx0 < RZ_TW ? P.W - xx0 : RZ_TW, th = P.H - yy0 < RZ_TH ? P.H - yy0 : RZ_TH;
    // the source rectangle of the tile, from the tables in memory (uniform loads; the host checked: span <= RZ_MAX_SPAN, nrows <=
    // RZ_MAX_ROWS, inside the frame), so that the first batch's loads can be issued before anything else
    const int x0 = P.hp ? P.bh[2 * xx0] : xx0, span = P.hp ? P.bh[2 * (xx0 + tw - 1)] + P.bh[2 * (xx0 + tw - 1) + 1] - x0 : tw;
    const int y0 = P.vp ? P.bv[2 * yy0] : yy0, nrows = P.vp ? P.bv[2 * (yy0 + th - 1)] + P.bv[2 * (yy0 + th - 1) + 1] - y0 : th;
    const size_t plane = (size_t)P.sh * P.sw;
    const uint8_t *fs = P.src + (size_t)f * 3 * plane;
        // 2. horizontal pass: staged rows -> s_mid[row][channel][column].  A batch is RZ_RB rows: row group rr = t / 32 owns rows rr, rr + 8, ..
    const int rr = t >> 5, lane = t & 31;
    constexpr int RPT = RZ_RB / 8, NP = HWC ? 1 : 3, NW = HWC ? 8 : 3;      // rows per thread and batch; segments per row; words per lane and segment
    RzRow<NW> regs[RPT][NP];
    auto seg = [&](int r, int c) { return fs + (HWC ? ((size_t)(y0 + r) * P.sw + x0) * 3 : (size_t)c * plane + (size_t)(y0 + r) * P.sw + x0); };
    const int seglen = HWC ? span * 3 : span;
    auto load_batch = [&](int r0) {
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int r = r0 + rr + 8 * q;
            if (r < nrows) {
#pragma unroll
                for (int c = 0; c < NP; c++) rz_load_row<NW>(seg(r, c), seglen, lane, regs[q][c]);
            }
        }
    };
    load_batch(0);
    // 1. the tile's tables (the first batch's loads are in flight)
    if (P.hp) {
        for (int i = t; i < tw * P.ksh; i += 256) s_kh[i] = P.kh[(size_t)xx0 * P.ksh + i];
        if (t < 2 * tw) s_bh[t] = P.bh[2 * xx0 + t];
    }
    if (P.vp) {
        for (int i = t; i < th * P.ksv; i += 256) s_kv[i] = P.kv[(size_t)yy0 * P.ksv + i];
        if (t < 2 * th) s_bv[t] = P.bv[2 * yy0 + t];
    }
    // (no barrier of their own: the tables are read behind the first barrier of the loop below, which runs at least once)
    for (int r0 = 0; r0 < nrows; r0 += RZ_RB) {
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int r = r0 + rr + 8 * q;
            if (r < nrows) {
#pragma unroll
                for (int c = 0; c < NP; c++) rz_store_row<NW>(seg(r, c), seglen, lane, regs[q][c], s_stage + (rr + 8 * q) * RZ_ROWB + c * RZ_SUB);
            }
        }
        __syncthreads();
        if (r0 + RZ_RB < nrows) load_batch(r0 + RZ_RB);    // the next batch's loads fly while this one is convolved
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int r = r0 + rr + 8 * q;
            if (r >= nrows || lane >= tw) continue;
            int off[3];                                    // LDS offset of pixel x0's byte of channel c in this row
#pragma unroll
            for (int c = 0; c < 3; c++)
                off[c] = (rr + 8 * q) * RZ_ROWB + (HWC ? (int)((uintptr_t)seg(r, 0) & 3) + c : c * RZ_SUB + (int)((uintptr_t)seg(r, c) & 3));
            // (one 32-bit LDS read at an interleaved pixel's byte address, whatever its alignment, was measured: the kernel took 40 us
            // instead of 25 on a 4-frame KITTI chunk -- byte reads it is)
            constexpr int PS = HWC ? 3 : 1;                // bytes between a channel's neighbouring pixels in a staged row
            auto pixel = [&](int x, int c3[3]) {
#pragma unroll
                for (int c = 0; c < 3; c++) c3[c] = s_stage[off[c] + x * PS];
            };
            int v[3];
            if (P.hp) {
                const int xr = s_bh[2 * lane] - x0, n = s_bh[2 * lane + 1];
                const int *k = s_kh + lane * P.ksh;
                int acc[3] = {1 << 21, 1 << 21, 1 << 21};
                for (int x = 0; x < n; x++) {
                    const int kx = k[x];
                    int b[3];
                    pixel(xr + x, b);
#pragma unroll
                    for (int c = 0; c < 3; c++) acc[c] += b[c] * kx;
                }
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = rz_clip8(acc[c]);
            } else {
                pixel(lane, v);
            }
            s_mid[r * RZ_TW + lane] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
        }
        __syncthreads();                                   // the staging rows are free again; after the last batch: s_mid is complete
    }
    // 3. vertical pass from s_mid, and the output
    const size_t HW = (size_t)P.H * P.W;
    for (int yy = rr; yy < th; yy += 8) {
        if (lane >= tw) continue;
        int v[3];
        if (P.vp) {
            const int yr = s_bv[2 * yy] - y0, n = s_bv[2 * yy + 1];
            const int *k = s_kv + yy * P.ksv;
            int acc[3] = {1 << 21, 1 << 21, 1 << 21};
            for (int y = 0; y < n; y++) {
                const int ky = k[y];
                const uint32_t w = s_mid[(yr + y) * RZ_TW + lane];
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += (int)((w >> (8 * c)) & 255u) * ky;
            }
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = rz_clip8(acc[c]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = (int)((s_mid[yy * RZ_TW + lane] >> (8 * c)) & 255u);
        }
        const size_t pix = (size_t)(yy0 + yy) * P.W + (size_t)(xx0 + lane);
        if (F32) {
            float *d = (float *)P.dst + (size_t)f * 3 * HW + pix;
            float *m = (P.dst2 && f < P.nm) ? P.dst2 + (size_t)f * 3 * HW + pix : nullptr;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float e = (float)v[c] / 255.0f;
                d[(size_t)c * HW] = e;
                if (m) m[(size_t)c * HW] = e;
            }
        } else {
            uint8_t *d = (uint8_t *)P.dst + (size_t)f * 3 * HW;
#pragma unroll
            for (int c = 0; c < 3; c++) d[HWC ? pix * 3 + c : (size_t)c * HW + pix] = (uint8_t)v[c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side

// NULL when (src_h, src_w) -> (H, W) is within the kernel's limits, else why not
static inline const char *resize_refusal(int src_h, int src_w, int H, int W) {
    if (src_h < 1 || src_w < 1 || H < 1 || W < 1) return "sizes must be positive";
    if (src_h > RZ_MAX_SIDE || src_w > RZ_MAX_SIDE) return "the source is larger than 32768 on a side";
    if ((long long)src_h > (long long)RZ_MAX_RATIO * H || (long long)src_w > (long long)RZ_MAX_RATIO * W)
        return "the source is more than 8 times the frame size along an axis (the LDS tile holds the rows of an 8x reduction)";
    return nullptr;
}

// the tables of one (src_h, src_w) -> (H, W) as the kernel reads them
struct ResizeTable {
    int sh = 0, sw = 0, H = 0, W = 0;
    int hp = 0, vp = 0, ksh = 0, ksv = 0;
    int *dev = nullptr;                                    // [bh: W*2][kh: W*ksh][bv: H*2][kv: H*ksv]  (a skipped pass has no entries)
    size_t off_kh = 0, off_bv = 0, off_kv = 0;
};

// host blob for ResizeTable::dev; false when a tile's source rectangle does not fit the kernel's LDS (cannot happen within resize_refusal)
static inline bool resize_build_table(ResizeTable &T, std::vector<int> &blob) {
    T.hp = T.sw != T.W; T.vp = T.sh != T.H;
    T.ksh = T.hp ? tc::resize_ksize(T.sw, T.W) : 0;
    T.ksv = T.vp ? tc::resize_ksize(T.sh, T.H) : 0;
    if (T.ksh > RZ_MAX_KSIZE || T.ksv > RZ_MAX_KSIZE) return false;
    const size_t nbh = T.hp ? (size_t)T.W * 2 : 0, nkh = (size_t)T.W * T.ksh, nbv = T.vp ? (size_t)T.H * 2 : 0, nkv = (size_t)T.H * T.ksv;
    T.off_kh = nbh; T.off_bv = nbh + nkh; T.off_kv = nbh + nkh + nbv;
    blob.assign(nbh + nkh + nbv + nkv + 1, 0);             // (+ 1: never empty)
    if (T.hp) tc::resize_coeffs(T.sw, T.W, blob.data(), blob.data() + T.off_kh);
    if (T.vp) tc::resize_coeffs(T.sh, T.H, blob.data() + T.off_bv, blob.data() + T.off_kv);
    auto fits = [](const int *b, int out, int in, int tile, int most) {
        for (int o0 = 0; o0 < out; o0 += tile) {
            const int o1 = (o0 + tile < out ? o0 + tile : out) - 1;
            for (int o = o0; o <= o1; o++)                 // every window inside the tile's rectangle, the rectangle inside the image
                if (b[2 * o] < b[2 * o0] || b[2 * o + 1] < 0 || b[2 * o] + b[2 * o + 1] > b[2 * o1] + b[2 * o1 + 1]) return false;
            if (b[2 * o0] < 0 || b[2 * o1] + b[2 * o1 + 1] > in || b[2 * o1] + b[2 * o1 + 1] - b[2 * o0] > most) return false;
        }
        return true;
    };
    if (T.hp && !fits(blob.data(), T.W, T.sw, RZ_TW, RZ_MAX_SPAN)) return false;
    if (T.vp && !fits(blob.data() + T.off_bv, T.H, T.sh, RZ_TH, RZ_MAX_ROWS)) return false;
    return true;
}

// N frames of `hwc ? [N,h,w,3] : [N,3,h,w]` bytes at src -> f32 ? [N,3,H,W] floats at dst (and the first nm of them at dst2, when given)
//                                                             : bytes [N,H,W,3] / [N,3,H,W] (the source's layout) at dst
static inline hipError_t launch_resize_u8(hipStream_t stream, const ResizeTable &T, bool hwc, bool f32, int N, const uint8_t *src, void *dst,
                                          float *dst2, int nm) {
    ResizeParams P;
    P.sh = T.sh; P.sw = T.sw; P.H = T.H; P.W = T.W; P.hp = T.hp; P.vp = T.vp; P.ksh = T.ksh; P.ksv = T.ksv;
    P.bh = T.dev; P.kh = T.dev + T.off_kh; P.bv = T.dev + T.off_bv; P.kv = T.dev + T.off_kv;
    const size_t fb = (size_t)3 * T.sh * T.sw, ob = (size_t)3 * T.H * T.W * (f32 ? sizeof(float) : 1);
    const dim3 tiles((unsigned)((T.W + RZ_TW - 1) / RZ_TW), (unsigned)((T.H + RZ_TH - 1) / RZ_TH));
    for (int f0 = 0; f0 < N; f0 += 65535) {               // (gridDim.z is a 16-bit quantity)
        const int nf = N - f0 < 65535 ? N - f0 : 65535;
        const int nmf = f32 && dst2 && nm > f0 ? (nm - f0 < nf ? nm - f0 : nf) : 0;
        P.src = src + (size_t)f0 * fb;
        P.dst = (uint8_t *)dst + (size_t)f0 * ob;
        P.dst2 = nmf ? dst2 + (size_t)f0 * 3 * T.H * T.W : nullptr;
        P.nm = nmf;
        auto k = hwc ? (f32 ? k_resize_u8<true, true> : k_resize_u8<true, false>) : (f32 ? k_resize_u8<false, true> : k_resize_u8<false, false>);
        hipLaunchKernelGGL(k, dim3(tiles.x, tiles.y, (unsigned)nf), dim3(256), 0, stream, P);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}
