// Host side of frame preparation (include/tcsfm.h: tcsfm_disp_post_process, tcsfm_flip_ramp, tcsfm_frames_from_u8, tcsfm_resize_u8,
// tcsfm_resize_coeffs, tcsfm_scale_intrinsics) and the three helpers the sequence calls and the depth network share with them:
// flip_ramp_device, launch_disp_post and resize_table.  Part of tcsfm_api.hip, the library's only translation unit: included after
// call_host.h (drain_queued), before depthnet_host.h and sequence_host.h, which use the helpers.
#pragma once

// The flip post-processing's ramp table (flip_ramp.h) for the handle's W on the device: built on the host on first use,
// kept for the handle's life.  NULL: h->err says why.
static const double *flip_ramp_device(tcsfm_handle h) {
    if (h->flip_ramp) return h->flip_ramp;
    std::vector<double> ramp((size_t)h->W);
    flip_ramp(h->W, ramp.data());
    DevBuf<double> dev;
    if (hipError_t e = DEV_RESERVE(dev, ramp.size())) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return nullptr; }
    if (hipError_t e = hipMemcpy(dev, ramp.data(), ramp.size() * sizeof(double), hipMemcpyHostToDevice)) {      // (synchronous: ramp is a temporary)
        h->err = std::string("hipMemcpy: ") + hipGetErrorString(e);
        return nullptr;
    }
    return h->flip_ramp = std::move(dev);
}

// k_disp_post over n planes: the vector form where the row pairs are aligned (W even, 8-byte l / rf, 16-byte out), else the scalar one
static hipError_t launch_disp_post(hipStream_t s, int n, int H, int W, const float *l, const float *rf, const double *ramp, double *out) {
    const long long rows = (long long)n * H, threads = rows * ((W + 1) / 2);
    const dim3 grid((unsigned)((threads + 255) / 256));
    const bool vec = W % 2 == 0 && (((uintptr_t)l | (uintptr_t)rf) & 7) == 0 && ((uintptr_t)out & 15) == 0;
    if (vec) hipLaunchKernelGGL(k_disp_post<true>, grid, dim3(256), 0, s, l, rf, ramp, out, rows, W);
    else hipLaunchKernelGGL(k_disp_post<false>, grid, dim3(256), 0, s, l, rf, ramp, out, rows, W);
    return hipGetLastError();
}

// The device copy of the resize tables for (src_h, src_w) -> the handle's (H, W): built on the host once per source size and kept for the
// handle's life (a handful of ints per output row and column).  NULL: h->err says why (the caller returns TCSFM_E_HIP / TCSFM_E_ARG).
static const ResizeTable *resize_table(tcsfm_handle h, int src_h, int src_w) {
    for (const auto &t : h->resize_tabs)
        if (t.sh == src_h && t.sw == src_w) return &t;
    tcsfm_ctx::OwnedResizeTable T;
    T.sh = src_h; T.sw = src_w; T.H = h->H; T.W = h->W;
    std::vector<int> blob;
    if (!resize_build_table(T, blob)) { h->err = "resize: the source size is beyond the kernel's tile (resize_u8_kernel.h)"; return nullptr; }
    if (hipError_t e = DEV_RESERVE(T.blob, blob.size())) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return nullptr; }
    if (hipError_t e = hipMemcpy(T.blob, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice)) {      // (synchronous: blob is a temporary)
        h->err = std::string("hipMemcpy: ") + hipGetErrorString(e);
        return nullptr;
    }
    T.dev = T.blob;
    h->resize_tabs.push_back(std::move(T));
    return &h->resize_tabs.back();
}

int tcsfm_disp_post_process(tcsfm_handle h, const tcsfm_opts *o, int N, const void *l_disp, const void *r_disp_mirrored, void *out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !l_disp || !r_disp_mirrored || !out) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: NULL argument");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: host_ptrs must be 0 (device pointers); a host caller has the sequence calls (tcsfm_sequence_disparity)");
    if (h->W < 2) return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: the ramp needs W >= 2");
    if ((((uintptr_t)l_disp | (uintptr_t)r_disp_mirrored) & 3) != 0 || ((uintptr_t)out & 7) != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_disp_post_process: the inputs must be aligned for float, out for double");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("l_disp", l_disp, (size_t)N * hw * sizeof(float)); a.in("r_disp_mirrored", r_disp_mirrored, (size_t)N * hw * sizeof(float));
    a.out("out", out, (size_t)N * hw * sizeof(double));
    if (int rc = check_overlap(h, "tcsfm_disp_post_process", a)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    const double *ramp = flip_ramp_device(h);
    if (!ramp) return TCSFM_E_HIP;
    HIPCHK(h, launch_disp_post(h->stream, N, h->H, h->W, (const float *)l_disp, (const float *)r_disp_mirrored, ramp, (double *)out));
    return TCSFM_OK;
}

int tcsfm_flip_ramp(int W, void *l_mask_out) {
    if (W < 2 || !l_mask_out) return TCSFM_E_ARG;
    tc::flip_ramp(W, (double *)l_mask_out);
    return TCSFM_OK;
}

int tcsfm_frames_from_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, const void *src, void *dst) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !src || !dst) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: NULL argument");
    if (format != TCSFM_FRAMES_U8_CHW && format != TCSFM_FRAMES_U8_HWC)
        return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: format must be TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC (float frames need no conversion)");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: host_ptrs must be 0 (device pointers); host frames go through the sequence calls (tcsfm_sequence_frame_format)");
    if (((uintptr_t)dst & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_frames_from_u8: dst must be aligned for float");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("src", src, (size_t)N * 3 * hw); a.out("dst", dst, (size_t)N * 3 * hw * sizeof(float));
    std::string msg;
    if (a.refused("tcsfm_frames_from_u8", msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    HIPCHK(h, launch_frames_u8(h->stream, format == TCSFM_FRAMES_U8_HWC, N, (const uint8_t *)src, (float *)dst, nullptr, 0, hw));
    return TCSFM_OK;
}

int tcsfm_resize_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, int src_h, int src_w, const void *src, int dst_format, void *dst) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !src || !dst) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: NULL argument");
    if (format != TCSFM_FRAMES_U8_CHW && format != TCSFM_FRAMES_U8_HWC)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: format must be TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC");
    if (dst_format != format && dst_format != TCSFM_FRAMES_F32_CHW)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: dst_format must be the source's format (bytes) or TCSFM_FRAMES_F32_CHW");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: host_ptrs must be 0 (device pointers); host frames go through the sequence calls (tcsfm_sequence_frame_source)");
    if (src_h <= 0 || src_w <= 0) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: src_h and src_w must be positive");
    if (const char *why = resize_refusal(src_h, src_w, h->H, h->W)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_resize_u8: ") + why).c_str());
    const bool f32 = dst_format == TCSFM_FRAMES_F32_CHW;
    if (f32 && ((uintptr_t)dst & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_resize_u8: a float dst must be aligned for float");
    const size_t hw = (size_t)h->H * h->W;
    ArgRanges a;
    a.in("src", src, (size_t)N * 3 * src_h * src_w); a.out("dst", dst, (size_t)N * 3 * hw * (f32 ? sizeof(float) : 1));
    std::string msg;
    if (a.refused("tcsfm_resize_u8", msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    const ResizeTable *T = resize_table(h, src_h, src_w);
    if (!T) return TCSFM_E_HIP;
    HIPCHK(h, launch_resize_u8(h->stream, *T, format == TCSFM_FRAMES_U8_HWC, f32, N, (const uint8_t *)src, dst, nullptr, 0));
    return TCSFM_OK;
}

int tcsfm_resize_coeffs(int in, int out, int *ksize_out, int *bounds, int *kk) {
    if (in < 1 || out < 1 || !ksize_out) return TCSFM_E_ARG;
    *ksize_out = tc::resize_coeffs(in, out, bounds, kk);
    return TCSFM_OK;
}

int tcsfm_scale_intrinsics(int src_h, int src_w, int H, int W, const void *K_src, void *K_out) {
    if (src_h < 1 || src_w < 1 || H < 1 || W < 1 || !K_src || !K_out) return TCSFM_E_ARG;
    tc::scale_intrinsics(src_h, src_w, H, W, (const float *)K_src, (float *)K_out);
    return TCSFM_OK;
}
