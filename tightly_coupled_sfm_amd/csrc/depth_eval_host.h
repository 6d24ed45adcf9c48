// Host side of the depth evaluation (depth_eval_kernel.h): the crop, the argument checks and the two entry points -- tcsfm_depth_eval on
// device pointers, tcsfm_sequence_depth_eval on the sequence calls' disparity store.  Part of tcsfm_api.hip, the library's only
// translation unit: included after the other host headers.
#pragma once

namespace {

// the pixels a protocol looks at: evaluate_depth_eigen.py:146-148's np.array([...]).astype(np.int32), or the whole plane
void depth_eval_crop(int protocol, int gt_h, int gt_w, int c[4]) {
    if (protocol == TCSFM_EVAL_EIGEN_BENCHMARK) { c[0] = 0; c[1] = gt_h; c[2] = 0; c[3] = gt_w; return; }
    c[0] = (int)(0.40810811 * (double)gt_h); c[1] = (int)(0.99189189 * (double)gt_h);
    c[2] = (int)(0.03594771 * (double)gt_w); c[3] = (int)(0.96405229 * (double)gt_w);
}

// what both entries refuse about the options and the ground truth's size; NULL when there is nothing to refuse
const char *depth_eval_refusal(const tcsfm_depth_eval_opts *e, int gt_h, int gt_w) {
    if (gt_h < 1 || gt_w < 1) return "gt_h and gt_w must be at least 1";
    if ((long long)gt_h * gt_w > 0x7FFFFFFFll) return "a ground-truth plane holds at most 2^31 - 1 pixels";
    if (e->protocol != TCSFM_EVAL_EIGEN && e->protocol != TCSFM_EVAL_EIGEN_BENCHMARK)
        return "protocol must be TCSFM_EVAL_EIGEN or TCSFM_EVAL_EIGEN_BENCHMARK";
    if (!(e->min_depth > 0.f && e->max_depth > e->min_depth) || !std::isfinite(e->max_depth)) return "need 0 < min_depth < max_depth";
    if (!(e->depth_unit > 0.0) || !std::isfinite(e->depth_unit)) return "depth_unit must be positive and finite";
    return nullptr;
}

hipError_t launch_depth_eval(hipStream_t s, const tcsfm_depth_eval_opts *e, int N, int disp_is_f64, int H, int W, const void *disp, int gt_h,
                             int gt_w, const float *gt, double *out) {
    DepthEvalArgs a;
    memset(&a, 0, sizeof(a));
    a.H = H; a.W = W; a.gt_h = gt_h; a.gt_w = gt_w;
    int c[4];
    depth_eval_crop(e->protocol, gt_h, gt_w, c);
    a.y0 = c[0]; a.y1 = c[1]; a.x0 = c[2]; a.x1 = c[3];
    a.benchmark = e->protocol == TCSFM_EVAL_EIGEN_BENCHMARK; a.median_scaling = e->median_scaling != 0;
    a.lds_pairs = e->lds_pairs < 0 ? kEvalLdsPairs : e->lds_pairs;
    a.min_f = e->min_depth; a.max_f = e->max_depth; a.min_d = (double)e->min_depth; a.max_d = (double)e->max_depth;
    a.depth_unit = e->depth_unit;
    a.scale_x = 1.0 / ((double)gt_w / (double)W); a.scale_y = 1.0 / ((double)gt_h / (double)H);
    if (disp_is_f64) hipLaunchKernelGGL(k_depth_eval<double>, dim3((unsigned)N), dim3(kEvalThreads), 0, s, (const double *)disp, gt, a, out);
    else hipLaunchKernelGGL(k_depth_eval<float>, dim3((unsigned)N), dim3(kEvalThreads), 0, s, (const float *)disp, gt, a, out);
    return hipGetLastError();
}

}  // namespace

void tcsfm_depth_eval_default_opts(tcsfm_depth_eval_opts *e) {
    if (!e) return;
    memset(e, 0, sizeof(*e));
    e->protocol = TCSFM_EVAL_EIGEN; e->median_scaling = 1; e->min_depth = 1e-3f; e->max_depth = 80.f; e->depth_unit = 30.0; e->lds_pairs = -1;
}

int tcsfm_depth_eval_crop(int protocol, int gt_h, int gt_w, int *crop_out) {
    if (!crop_out || gt_h < 1 || gt_w < 1 || (protocol != TCSFM_EVAL_EIGEN && protocol != TCSFM_EVAL_EIGEN_BENCHMARK)) return TCSFM_E_ARG;
    depth_eval_crop(protocol, gt_h, gt_w, crop_out);
    return TCSFM_OK;
}

int tcsfm_depth_eval(tcsfm_handle h, const tcsfm_opts *o, const tcsfm_depth_eval_opts *e, int N, int disp_is_f64, const void *disp, int gt_h,
                     int gt_w, const void *gt, void *metrics_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!o || !e || !disp || !gt || !metrics_out) return fail(h, TCSFM_E_ARG, "tcsfm_depth_eval: NULL argument");
    if (N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_depth_eval: N must be at least 1");
    if (o->host_ptrs != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_depth_eval: host_ptrs must be 0 (device pointers); a host caller has tcsfm_sequence_depth_eval");
    if (const char *why = depth_eval_refusal(e, gt_h, gt_w)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_depth_eval: ") + why).c_str());
    if (((uintptr_t)disp & (disp_is_f64 ? 7 : 3)) != 0 || ((uintptr_t)gt & 3) != 0 || ((uintptr_t)metrics_out & 7) != 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_depth_eval: disp and gt must be aligned for their types, metrics_out for double");
    ArgRanges a;
    a.in("disp", disp, (size_t)N * h->H * h->W * (disp_is_f64 ? sizeof(double) : sizeof(float)));
    a.in("gt", gt, (size_t)N * gt_h * gt_w * sizeof(float));
    a.out("metrics_out", metrics_out, (size_t)N * TCSFM_NEVAL * sizeof(double));
    if (int rc = check_overlap(h, "tcsfm_depth_eval", a)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    HIPCHK(h, launch_depth_eval(h->stream, e, N, disp_is_f64 != 0, h->H, h->W, disp, gt_h, gt_w, (const float *)gt, (double *)metrics_out));
    return TCSFM_OK;
}

int tcsfm_sequence_depth_eval(tcsfm_handle h, const tcsfm_depth_eval_opts *e, int T, int first, int count, int gt_h, int gt_w, const void *gt,
                              void *metrics_out) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    if (!e || !gt || !metrics_out) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_depth_eval: NULL argument");
    if (h->seq_disp_T == 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_depth_eval: nothing kept (the last sequence call failed or ran with the stage off: tcsfm_sequence_disparity)");
    if (T != h->seq_disp_T) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_depth_eval: T differs from the T of the last sequence call");
    if (first < 0 || count < 1 || first > T - count) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_depth_eval: need 0 <= first, count >= 1 and first + count <= T");
    if (const char *why = depth_eval_refusal(e, gt_h, gt_w)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_sequence_depth_eval: ") + why).c_str());
    const size_t gt_plane = (size_t)gt_h * gt_w * sizeof(float);
    ArgRanges a;
    a.in("gt", gt, (size_t)count * gt_plane); a.out("metrics_out", metrics_out, (size_t)count * TCSFM_NEVAL * sizeof(double));
    if (int rc = check_overlap(h, "tcsfm_sequence_depth_eval", a)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    // ground truth goes up in groups of at most 64 MB (a group of one frame when a plane is larger), the metrics come back once
    const size_t per_group = std::max<size_t>(1, std::min<size_t>((size_t)count, ((size_t)64 << 20) / gt_plane));
    // (a buffer that has to go may still be in use by the previous call's kernels on the stream)
    if (h->eval_gt_dev.p && h->eval_gt_dev.cap < per_group * gt_plane) HIPCHK(h, hipStreamSynchronize(h->stream));
    RESERVE(h, h->eval_gt_dev, per_group * gt_plane);
    if (h->eval_out_dev.p && h->eval_out_dev.cap < (size_t)count * TCSFM_NEVAL) HIPCHK(h, hipStreamSynchronize(h->stream));
    RESERVE(h, h->eval_out_dev, (size_t)count * TCSFM_NEVAL);
    const bool f64 = h->seq_disp_kept == TCSFM_SEQ_DISP_POST;
    const size_t plane = (size_t)h->H * h->W * (f64 ? sizeof(double) : sizeof(float));
    for (size_t g0 = 0; g0 < (size_t)count; g0 += per_group) {
        const size_t n = std::min(per_group, (size_t)count - g0);
        // (the stream orders this copy behind the kernel that read the previous group)
        HIPCHK(h, hipMemcpyAsync(h->eval_gt_dev.p, (const char *)gt + g0 * gt_plane, n * gt_plane, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, launch_depth_eval(h->stream, e, (int)n, f64, h->H, h->W, h->seq_disp_dev.p + ((size_t)first + g0) * plane, gt_h, gt_w,
                                    (const float *)h->eval_gt_dev.p, h->eval_out_dev.p + g0 * TCSFM_NEVAL));
    }
    HIPCHK(h, hipMemcpyAsync(metrics_out, h->eval_out_dev.p, (size_t)count * TCSFM_NEVAL * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return TCSFM_OK;
}
