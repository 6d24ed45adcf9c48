// Host side of the PoseNet (models/pose_models.py:88-147) and the coupled pose loop (train_mono.py:64-80): the tcsfm_posenet_* entry points,
// pose_loop and tcsfm_solve_pose_iteratively.  Part of tcsfm_api.hip, the library's only translation unit: included after context.h
// (tcsfm_ctx, fail, fail_alloc, HIPCHK, DEV_RESERVE, DeviceGuard, check_intrinsics), drain_queued and init_params, and before the sequence driver, which runs
// pose_loop on its lanes.  include/tcsfm.h declares the entry points, so they have C linkage here.
#pragma once

// What a load fills and every instance's launches read: the prepared and the raw convolution weights (conv2d_wn's chain rule needs the raw
// ones: tcsfm_posenet_param_backward; kept by both load paths), the biases, the GroupNorm parameters and the head.
struct PnWeights {
    DevBuf<pn_f4> w4[7];
    DevBuf<float> bias[7], gamma[7], beta[7], raww[7];
    DevBuf<float> head_w, head_b;
};

// The layer geometry and the work split: a function of the handle's frame size only.
struct PnGeometry {
    PnLayer L[7];
    int nb_cfg[2][7] = {}, ks_cfg[2][7] = {};   // (output-channel blocks per wave, K split) per layer: [0] few images (latency), [1] many
};

// One instance: the primary (tcsfm_posenet_create) owns the weights; tcsfm_odometry_sequence runs the network on the handle's lanes, and
// clone k works on lane k with its own activations and READS the primary's weights through `w`.  The primary outlives its clones
// (tcsfm_posenet_destroy destroys them first).
struct tcsfm_posenet : PnGeometry {
    tcsfm_ctx *h = nullptr;
    int max_images = 0, loaded = 0;
    int last_N = 0;              // images of the most recent evaluation (tcsfm_debug_posenet_layer reads its activations)
    PnWeights own;               // the primary's weights (empty in a clone)
    const PnWeights *w = &own;   // the weights the launches read: the primary's
    bool is_clone() const { return w != &own; }
    DevBuf<float> act[7], scsh[7], part[7];
    DevBuf<float> in_buf;        // [max_images,6,H,W] (tgt * valid | img_rec) written by the warp kernel
    DevBuf<float> pose;          // [max_images,6] running pose of the coupled loop
    std::vector<tcsfm_posenet *> clones;
    // tcsfm_posenet_backward (posenet_grad_host.h), the primary's only, all built at the first backward after a load: the transposed images
    // of the prepared weights (layer 1: the plain [ky][kx][ci][co] image), two gradient maps [max_images][largest layer output] and the
    // per-group sums [max_images][16][2]
    DevBuf<pn_f4> wt4[7];
    int wt_valid = 0;
    DevBuf<float> gbuf[2], gss;
    // tcsfm_posenet_param_backward (posenet_wgrad_host.h), built at the first parameter backward: the weight-gradient partials and the
    // per-channel double partials
    DevBuf<float> wpart;
    DevBuf<double> cpart;
};

void tcsfm_posenet_destroy(tcsfm_posenet *pn) {
    if (!pn) return;
    for (tcsfm_posenet *c : pn->clones) tcsfm_posenet_destroy(c);
    DeviceGuard dev_guard(pn->h->device);
    delete pn;
}

// activations, statistics and loop buffers of one PoseNet instance (layer geometry and work split already filled in)
static hipError_t pn_alloc_scratch(tcsfm_posenet *pn) {
    hipError_t e = hipSuccess;
    const int max_images = pn->max_images;
    for (int l = 0; l < 7 && e == hipSuccess; l++) {
        const PnLayer &L = pn->L[l];
        e = DEV_RESERVE(pn->act[l], (size_t)L.ksplit * max_images * L.oh * L.ow * L.cout);
        if (e == hipSuccess) e = DEV_RESERVE(pn->scsh[l], (size_t)max_images * L.cout * 2);
        if (e == hipSuccess && (pn->ks_cfg[0][l] == 1 || pn->ks_cfg[1][l] == 1))
            e = DEV_RESERVE(pn->part[l], (size_t)max_images * std::max((L.oh * L.ow + 63) / 64, L.oh * ((L.ow + 63) / 64)) * L.cout * 2);
    }
    if (e == hipSuccess) e = DEV_RESERVE(pn->in_buf, (size_t)max_images * 6 * pn->h->H * pn->h->W);
    if (e == hipSuccess) e = DEV_RESERVE(pn->pose, (size_t)max_images * 6);
    return e;
}

// the instance that runs `pn`'s network on lane context `c` (lane 0 = pn itself)
static tcsfm_posenet *pn_for_lane(tcsfm_posenet *pn, tcsfm_ctx *c) {
    if (pn->h == c) return pn;
    for (tcsfm_posenet *q : pn->clones)
        if (q->h == c) return q;
    tcsfm_posenet *q = new tcsfm_posenet();
    static_cast<PnGeometry &>(*q) = *pn;
    q->h = c; q->max_images = pn->max_images; q->loaded = pn->loaded; q->w = pn->w;
    if (pn_alloc_scratch(q) != hipSuccess) { tcsfm_posenet_destroy(q); return nullptr; }
    pn->clones.push_back(q);
    return q;
}

int tcsfm_posenet_create(tcsfm_handle h, int max_images, tcsfm_posenet **out) {
    if (!h || !out) return TCSFM_E_ARG;
    *out = nullptr;
    if (max_images < 1 || max_images > 4096) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_create: max_images out of range");
    DeviceGuard dev_guard(h->device);
    tcsfm_posenet *pn = new tcsfm_posenet();
    pn->h = h; pn->max_images = max_images;
    static const int chans[8] = {6, 16, 32, 64, 128, 256, 256, 256}, ksz[7] = {7, 5, 3, 3, 3, 3, 3};
    int ih = h->H, iw = h->W;
    hipError_t e = hipSuccess;
    for (int l = 0; l < 7; l++) {
        PnLayer &L = pn->L[l];
        L.cin = chans[l]; L.cout = chans[l + 1]; L.ks = ksz[l]; L.pad = (ksz[l] - 1) / 2;
        L.ih = ih; L.iw = iw; L.oh = (ih + 2 * L.pad - L.ks) / 2 + 1; L.ow = (iw + 2 * L.pad - L.ks) / 2 + 1;
        L.kgroups = l == 0 ? 21 : L.ks * L.ks * L.cin / 16;
        // Work split of a layer = (output-channel blocks of 16 per wave, K split).  A wave's K loop is a serial chain of loads and
        // matrix-core steps, and a window's fwd + inv pair is only 2 images: with 4 channel blocks per wave and K whole the small
        // layers ran on ~100 waves of ~300 dependent MFMAs each (15 us per layer whatever its size).  Two fixed regimes, chosen by
        // the number of images only (results do not depend on anything else):
        //   few images (N <= 4): as few channel blocks per wave as it takes to have ~800 waves for N = 2, then K split until they
        //                        exist or a wave's loop is down to 8 groups;
        //   many images:         up to 4 channel blocks per wave, K split only for the late layers (few output pixels).
        {
            const int pxb = (L.oh * L.ow + 15) / 16, cb = L.cout / 16;
            int nb = std::min(cb, 4), ks = 1;
            while (nb > 1 && pxb * (cb / nb) * 2 < 768) nb /= 2;
            while (ks < 16 && pxb * (cb / nb) * 2 * ks < 768 && L.kgroups / (2 * ks) >= 8) ks *= 2;
            pn->nb_cfg[0][l] = l == 0 ? 1 : nb; pn->ks_cfg[0][l] = l == 0 ? 1 : ks;
            pn->nb_cfg[1][l] = L.cout >= 64 ? 4 : cb;
            pn->ks_cfg[1][l] = L.oh * L.ow <= 512 ? std::min(16, (L.kgroups + 23) / 24) : 1;
        }
        L.ksplit = std::max(pn->ks_cfg[0][l], pn->ks_cfg[1][l]);     // allocation; the launch sets the split it uses
        if (L.oh < 1 || L.ow < 1) { tcsfm_posenet_destroy(pn); return fail(h, TCSFM_E_ARG, "tcsfm_posenet_create: image too small for seven stride-2 layers"); }
        const size_t nw4 = (size_t)L.kgroups * 4 * L.cout;
        if (e == hipSuccess) e = DEV_RESERVE(pn->own.w4[l], nw4);
        for (DevBuf<float> *b : {&pn->own.bias[l], &pn->own.gamma[l], &pn->own.beta[l]}) if (e == hipSuccess) e = DEV_RESERVE(*b, L.cout);
        if (e == hipSuccess) e = DEV_RESERVE(pn->own.raww[l], (size_t)L.cout * L.cin * L.ks * L.ks);
        ih = L.oh; iw = L.ow;
    }
    if (e == hipSuccess) e = DEV_RESERVE(pn->own.head_w, 6 * 256);
    if (e == hipSuccess) e = DEV_RESERVE(pn->own.head_b, 6);
    if (e == hipSuccess) e = pn_alloc_scratch(pn);
    if (e != hipSuccess) { tcsfm_posenet_destroy(pn); return fail_alloc(h, e, "tcsfm_posenet_create: allocation failed"); }
    *out = pn;
    return TCSFM_OK;
}

int tcsfm_posenet_load(tcsfm_posenet *pn, const float *const conv_w[7], const float *const conv_b[7], const float *const gn_w[7],
                       const float *const gn_b[7], const float *head_w, const float *head_b) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (!conv_w || !head_w || !head_b) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_load: NULL argument");
    DeviceGuard dev_guard(h->device);
    for (int l = 0; l < 7; l++) {
        const PnLayer &L = pn->L[l];
        if (!conv_w[l]) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_load: NULL convolution weight");
        const size_t nw = (size_t)L.cout * L.cin * L.ks * L.ks;
        HIPCHK(h, hipMemcpyAsync(pn->w->raww[l], conv_w[l], nw * sizeof(float), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_pn_prep, dim3(L.cout), dim3(256), 0, h->stream, (const float *)pn->w->raww[l], pn->w->w4[l], L.cin, L.cout, L.ks, l == 0 ? 1 : 0, 1);
        HIPCHK(h, hipStreamSynchronize(h->stream));    // the caller's host arrays are free once this returns; loading happens once per model
        std::vector<float> ones(L.cout, 1.f), zeros(L.cout, 0.f);
        HIPCHK(h, hipMemcpy(pn->w->bias[l], conv_b && conv_b[l] ? conv_b[l] : zeros.data(), L.cout * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(pn->w->gamma[l], gn_w && gn_w[l] ? gn_w[l] : ones.data(), L.cout * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(pn->w->beta[l], gn_b && gn_b[l] ? gn_b[l] : zeros.data(), L.cout * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(pn->w->head_w, head_w, 6 * 256 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(pn->w->head_b, head_b, 6 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipGetLastError());
    pn->loaded = 1;
    pn->wt_valid = 0;        // the backward's transposed images follow w4: rebuilt at the next tcsfm_posenet_backward
    return TCSFM_OK;
}

// The same from DEVICE pointers, stream-ordered: no host staging and no synchronisation, cheap enough to run after every optimiser
// step.  k_pn_prep reads the kept raw copy, as in tcsfm_posenet_load: the prepared weights have the same bits for the same values.
int tcsfm_posenet_load_device(tcsfm_posenet *pn, const float *const conv_w[7], const float *const conv_b[7], const float *const gn_w[7],
                              const float *const gn_b[7], const float *head_w, const float *head_b) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (!conv_w || !head_w || !head_b) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_load_device: NULL argument");
    if (pn->is_clone()) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_load_device: pn is a lane clone");
    for (int l = 0; l < 7; l++)
        if (!conv_w[l]) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_load_device: NULL convolution weight");
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    hipStream_t s = h->stream;
    for (int l = 0; l < 7; l++) {
        const PnLayer &L = pn->L[l];
        const size_t nw = (size_t)L.cout * L.cin * L.ks * L.ks, nc = L.cout * sizeof(float);
        HIPCHK(h, hipMemcpyAsync(pn->w->raww[l], conv_w[l], nw * sizeof(float), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_pn_prep, dim3(L.cout), dim3(256), 0, s, (const float *)pn->w->raww[l], pn->w->w4[l], L.cin, L.cout, L.ks, l == 0 ? 1 : 0, 1);
        const float *src[3] = {conv_b ? conv_b[l] : nullptr, gn_w ? gn_w[l] : nullptr, gn_b ? gn_b[l] : nullptr};
        float *dst[3] = {pn->w->bias[l], pn->w->gamma[l], pn->w->beta[l]};
        for (int k = 0; k < 3; k++) {
            if (src[k]) HIPCHK(h, hipMemcpyAsync(dst[k], src[k], nc, hipMemcpyDeviceToDevice, s));
            else hipLaunchKernelGGL(k_pnw_fill, dim3((L.cout + 255) / 256), dim3(256), 0, s, dst[k], L.cout, k == 1 ? 1.f : 0.f);
        }
    }
    HIPCHK(h, hipMemcpyAsync(pn->w->head_w, head_w, 6 * 256 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(pn->w->head_b, head_b, 6 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipGetLastError());
    pn->loaded = 1;
    pn->wt_valid = 0;
    return TCSFM_OK;
}

namespace {
// work split of layer l (0-based) in a call over N images: channel blocks per wave, K split, pixel blocks per wave
void pn_split(const tcsfm_posenet *pn, int l, int N, int *nb, int *ks, int *pb) {
    const int cfg = N <= 4 ? 0 : 1;
    const PnLayer &L = pn->L[l];
    *nb = pn->nb_cfg[cfg][l]; *ks = pn->ks_cfg[cfg][l];
    // two pixel blocks per wave in the many-images regime where a layer has pixels to spare (posenet_kernel.h k_pn_conv PB): a fixed
    // function of the regime and the layer, so results stay bit-identical for every batch within a regime
    // (A/B on one box, KITTI odometry sequence at 8 / 12 windows per call: layers 2-5 with two blocks 3 632-3 640 / 3 702-3 710 windows/s,
    // layer 2 only 3 609-3 637 / 3 621-3 626, none 3 504-3 510)
    static const int pb_min_px = getenv("TCSFM_PN_PB_MIN_PIXELS") ? atoi(getenv("TCSFM_PN_PB_MIN_PIXELS")) : 64;        // (measurement hook)
    *pb = (cfg == 1 && l > 0 && *nb >= 2 && L.oh * L.ow >= pb_min_px) ? 2 : 1;
}

// The tape of a training forward over N images (tcsfm_posenet_forward_train), layer after layer: the reduced raw output
// [N][npix][cout], the (scale, shift) pairs [N][cout][2], the groups' (mean, rstd) [N][16][2].  Offsets in floats; returns the total.
struct PnTapeLayer { size_t raw, scsh, mr; };
size_t pn_tape_layout(const tcsfm_posenet *pn, int N, PnTapeLayer t[7]) {
    size_t o = 0;
    for (int l = 0; l < 7; l++) {
        const PnLayer &L = pn->L[l];
        t[l].raw = o; o += (size_t)N * L.oh * L.ow * L.cout;
        t[l].scsh = o; o += (size_t)N * L.cout * 2;
        t[l].mr = o; o += (size_t)N * 32;
    }
    return o;
}

// the seven convolutions + statistics passes + head of one PoseNet evaluation on N samples; the first layer reads
// (imgA | imgB) per sample (strides in floats; window indexing when win_B > 0).  tape: the same launches, and what the backward
// needs is copied out layer by layer (pn_tape_layout)
int pn_run(tcsfm_posenet *pn, int N, const float *imgA, long long strideA, const float *imgB, long long strideB, int win_B, int win_S,
           float *pose, int accumulate, float *stacked, int it, int iters, const WinOff *wo = nullptr, float *tape = nullptr) {
    tcsfm_ctx *h = pn->h;
    pn->last_N = N;
    PnTapeLayer tl[7];
    if (tape) pn_tape_layout(pn, N, tl);
    for (int l = 0; l < 7; l++) {
        PnLayer L = pn->L[l];
        int nb, pb;
        pn_split(pn, l, N, &nb, &L.ksplit, &pb);
        PnConvParams P;
        memset(&P, 0, sizeof(P));
        P.imgA = imgA; P.imgB = imgB; P.strideA = strideA; P.strideB = strideB; P.win_B = win_B; P.win_S = win_S;
        if (wo) P.win_off = *wo;
        P.in = l > 0 ? pn->act[l - 1] : nullptr; P.scsh = l > 0 ? pn->scsh[l - 1] : nullptr;
        P.w4 = pn->w->w4[l]; P.bias = pn->w->bias[l]; P.out = pn->act[l]; P.part = L.ksplit == 1 ? pn->part[l] : nullptr; P.L = L; P.N = N;
        dim3 grid((L.oh * L.ow + 64 * pb - 1) / (64 * pb), L.cout / (16 * nb), N * L.ksplit);
        if (l == 0) {            // LDS-staged first layer: one workgroup per 64-pixel segment of two output rows
            grid = dim3(((L.oh + 1) / 2) * ((L.ow + 63) / 64), 1, N);
            hipLaunchKernelGGL(k_pn_conv1, grid, dim3(256), 0, h->stream, P);
        } else if (nb == 1) hipLaunchKernelGGL((k_pn_conv<1, false>), grid, dim3(256), 0, h->stream, P);
        else if (nb == 2 && pb == 2) hipLaunchKernelGGL((k_pn_conv<2, false, 2>), grid, dim3(256), 0, h->stream, P);
        else if (nb == 2) hipLaunchKernelGGL((k_pn_conv<2, false>), grid, dim3(256), 0, h->stream, P);
        else if (pb == 2) hipLaunchKernelGGL((k_pn_conv<4, false, 2>), grid, dim3(256), 0, h->stream, P);
        else hipLaunchKernelGGL((k_pn_conv<4, false>), grid, dim3(256), 0, h->stream, P);
        // GroupNorm statistics (+ K-split combination) as their own launch.  Round 3 measured the alternative -- statistics, K-split
        // combination and the head in the convolutions' tails by the last-arriver ticket protocol, 7 launches instead of 15: every
        // convolution became 6-8 us SLOWER (ticket round trips, acquire, serial tail of the last workgroup), 127.5 vs 119 us per
        // evaluation (profiles/r03_posenet_fused_tail_kernel_stats.csv, _timing.jsonl) -- a separate 16 N-workgroup pass is faster.
        PnStatsParams S;
        S.part = P.part; S.tiles = (int)grid.x;
        S.out = pn->act[l]; S.bias = pn->w->bias[l]; S.gamma = pn->w->gamma[l]; S.beta = pn->w->beta[l]; S.scsh = pn->scsh[l];
        S.N = N; S.npix = L.oh * L.ow; S.cout = L.cout; S.ksplit = L.ksplit;
        S.mr = tape ? tape + tl[l].mr : nullptr;
        hipLaunchKernelGGL(k_pn_stats, dim3(N, 16), dim3(256), 0, h->stream, S);
        if (tape) {          // K-split plane 0 holds the reduced sums once the statistics pass has run
            HIPCHK(h, hipMemcpyAsync(tape + tl[l].raw, pn->act[l], (size_t)N * L.oh * L.ow * L.cout * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(tape + tl[l].scsh, pn->scsh[l], (size_t)N * L.cout * 2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        }
    }
    PnHeadParams Hd;
    Hd.x = pn->act[6]; Hd.scsh = pn->scsh[6]; Hd.w = pn->w->head_w; Hd.b = pn->w->head_b; Hd.pose = pose; Hd.stacked = stacked;
    Hd.npix = pn->L[6].oh * pn->L[6].ow; Hd.accumulate = accumulate; Hd.it = it; Hd.iters = iters;
    hipLaunchKernelGGL(k_pn_head, dim3(N), dim3(256), 0, h->stream, Hd);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}
}  // namespace

int tcsfm_posenet_forward(tcsfm_posenet *pn, int N, const float *imgs, float *pose_out) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (!pn->loaded) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward: no weights loaded");
    if (N < 1 || N > pn->max_images || !imgs || !pose_out) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward: bad argument");
    {
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 6 * h->H * h->W * sizeof(float));
        a.out("pose_out", pose_out, (size_t)N * 6 * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_posenet_forward", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    const long long hw = (long long)h->H * h->W;
    return pn_run(pn, N, imgs, 6 * hw, imgs + 3 * hw, 6 * hw, 0, 0, pose_out, 0, nullptr, 0, 1);
}

int tcsfm_debug_posenet_split(tcsfm_posenet *pn, int layer, int N, int *oh, int *ow, int *nb, int *ks, int *pb) {
    if (!pn) return TCSFM_E_ARG;
    if (layer < 1 || layer > 7 || N < 1 || N > pn->max_images) return fail(pn->h, TCSFM_E_ARG, "tcsfm_debug_posenet_split: bad layer or N");
    int nb_, ks_, pb_;
    pn_split(pn, layer - 1, N, &nb_, &ks_, &pb_);
    if (oh) *oh = pn->L[layer - 1].oh;
    if (ow) *ow = pn->L[layer - 1].ow;
    if (nb) *nb = nb_;
    if (ks) *ks = ks_;
    if (pb) *pb = pb_;
    return TCSFM_OK;
}

int tcsfm_debug_posenet_layer(tcsfm_posenet *pn, int layer, int N, float *raw_out, float *scsh_out) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (layer < 1 || layer > 7) return fail(h, TCSFM_E_ARG, "tcsfm_debug_posenet_layer: layer out of range");
    if (N < 1 || N > pn->last_N) return fail(h, TCSFM_E_ARG, "tcsfm_debug_posenet_layer: N exceeds the most recent evaluation");
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    const PnLayer &L = pn->L[layer - 1];
    // K-split plane 0 holds the reduced sums (+ bias) once k_pn_stats has run: [last_N][npix][cout], the first N samples of it
    if (raw_out) HIPCHK(h, hipMemcpyAsync(raw_out, pn->act[layer - 1], (size_t)N * L.oh * L.ow * L.cout * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (scsh_out) HIPCHK(h, hipMemcpyAsync(scsh_out, pn->scsh[layer - 1], (size_t)N * L.cout * 2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return TCSFM_OK;
}

// the coupled loop of train_mono.py:64-80 on context `h` (the handle or one of its lanes; pn->h == h): network, warps, corrections
static int pose_loop(tcsfm_ctx *h, tcsfm_posenet *pn, int num_iter, int B, int S, const float *tgt, const float *srcs, const float *depth_t,
                     const float *depth_s, const float *K, float *poses_out, float *stacked_out, const WinOff *wo) {
    const int N = 2 * B * S;
    int rc;
    tcsfm_opts o; tcsfm_default_opts(&o);
    if ((rc = check_intrinsics(h, &o, K, B))) return rc;
    const long long hw = (long long)h->H * h->W;
    // full_poses = pose_model(cat(tgt | src ; src | tgt)), train_mono.py:54-64 -- the pairs are formed by indexing
    if ((rc = pn_run(pn, N, tgt, 3 * hw, srcs, 3 * hw, B, S, pn->pose, 0, stacked_out, 0, num_iter, wo))) return rc;
    for (int it = 1; it < num_iter; it++) {
        // inverse_warp2(src, d_t, d_s, -full_poses, K) with the next network input (tgt * valid | img_rec) written by the warp
        // itself (train_mono.py:69-76), then full_poses += pose_model(new_imgs) (:77-78)
        InitParams I = init_params(h, &o, N, pn->pose, nullptr, K, 0);
        I.K_mod = B;
        hipLaunchKernelGGL(k_init, dim3((N + 63) / 64), dim3(64), 0, h->stream, I);
        WarpParams W;
        memset(&W, 0, sizeof(W));
        W.src = srcs; W.depth_t = depth_t; W.depth_s = depth_s; W.pc = h->pconst; W.tgt = tgt; W.posenet_in = pn->in_buf;
        W.H = h->H; W.W = h->W; W.win_B = B; W.win_S = S;
        if (wo) W.win_off = *wo;
        hipLaunchKernelGGL(k_warp, dim3((unsigned)((hw + 255) / 256), N), dim3(256), 0, h->stream, W);
        if ((rc = pn_run(pn, N, pn->in_buf, 6 * hw, pn->in_buf + 3 * hw, 6 * hw, 0, 0, pn->pose, 1, stacked_out, it, num_iter))) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(poses_out, pn->pose, (size_t)N * 6 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return TCSFM_OK;
}

int tcsfm_solve_pose_iteratively(tcsfm_handle h, tcsfm_posenet *pn, int num_iter, int B, int S, const float *tgt, const float *srcs,
                                 const float *depth_t, const float *depth_s, const float *K, float *poses_out, float *stacked_out) {
    if (!h || !pn || pn->h != h) return TCSFM_E_ARG;
    if (!pn->loaded) return fail(h, TCSFM_E_ARG, "tcsfm_solve_pose_iteratively: no weights loaded");
    const int N = 2 * B * S;
    if (num_iter < 1 || B < 1 || S < 1 || N > pn->max_images || N > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_solve_pose_iteratively: sizes out of range");
    if (!tgt || !srcs || !depth_t || !depth_s || !K || !poses_out) return fail(h, TCSFM_E_ARG, "tcsfm_solve_pose_iteratively: NULL argument");
    {
        const size_t hw_b = (size_t)h->H * h->W * sizeof(float);
        ArgRanges a;
        a.in("tgt", tgt, (size_t)B * 3 * hw_b); a.in("srcs", srcs, (size_t)S * B * 3 * hw_b); a.in("depth_t", depth_t, (size_t)B * hw_b);
        a.in("depth_s", depth_s, (size_t)S * B * hw_b); a.in("K", K, (size_t)B * 9 * sizeof(float));
        a.out("poses_out", poses_out, (size_t)N * 6 * sizeof(float)); a.out("stacked_out", stacked_out, (size_t)N * num_iter * 6 * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_solve_pose_iteratively", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    return pose_loop(h, pn, num_iter, B, S, tgt, srcs, depth_t, depth_s, K, poses_out, stacked_out, nullptr);
}
