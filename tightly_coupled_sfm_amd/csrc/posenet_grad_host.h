// Host side of the PoseNet's gradients: the training forward with its tape and the backward walk that gives the input gradient
// (posenet_grad_kernel.h) and, for tcsfm_posenet_param_backward, the parameter gradients (posenet_wgrad_kernel.h, posenet_wgrad_host.h).
// Part of tcsfm_api.hip, the library's only translation unit: included after posenet_host.h (tcsfm_posenet, pn_run, pn_tape_layout)
// and depthnet_host.h, whose data-gradient dispatch (dn_split, dn_launch_ks<DnDgradKernel, KS>) layers 2..7 share.
#pragma once

namespace {
int pn_check_train(tcsfm_posenet *pn, int N, const char *fn) {
    tcsfm_ctx *h = pn->h;
    if (!pn->loaded) return fail(h, TCSFM_E_ARG, (std::string(fn) + ": no weights loaded").c_str());
    if (pn->is_clone()) return fail(h, TCSFM_E_ARG, (std::string(fn) + ": pn is a lane clone (the training calls run on the handle's own stream)").c_str());
    if (N < 1 || N > pn->max_images) return fail(h, TCSFM_E_ARG, (std::string(fn) + ": N out of range").c_str());
    return TCSFM_OK;
}

// transposed weight images and gradient scratch, once per load / per instance
int pnb_prepare(tcsfm_posenet *pn) {
    tcsfm_ctx *h = pn->h;
    hipError_t e = hipSuccess;
    for (int l = 0; l < 7 && e == hipSuccess; l++) {
        const PnLayer &L = pn->L[l];
        e = DEV_RESERVE(pn->wt4[l], (size_t)L.ks * L.ks * L.cin * L.cout / 4);
    }
    size_t map = 0;
    for (int l = 0; l < 7; l++) map = std::max(map, (size_t)pn->L[l].oh * pn->L[l].ow * pn->L[l].cout);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = DEV_RESERVE(pn->gbuf[k], (size_t)pn->max_images * map);
    if (e == hipSuccess) e = DEV_RESERVE(pn->gss, (size_t)pn->max_images * 32);
    if (e != hipSuccess) return fail_alloc(h, e, "tcsfm_posenet_backward: allocation failed");
    if (!pn->wt_valid) {
        hipLaunchKernelGGL(k_pnb_prep_t1, dim3(dn_blocks(49 * 6 * 16)), dim3(256), 0, h->stream, (const pn_f4 *)pn->w->w4[0], reinterpret_cast<float *>(pn->wt4[0].p));
        for (int l = 1; l < 7; l++) {
            const PnLayer &L = pn->L[l];
            hipLaunchKernelGGL(k_pnb_prep_t, dim3(dn_blocks((long long)L.ks * L.ks * L.cin * L.cout)), dim3(256), 0, h->stream, (const pn_f4 *)pn->w->w4[l],
                               pn->wt4[l], L.cin, L.cout, L.ks);
        }
        HIPCHK(h, hipGetLastError());
        pn->wt_valid = 1;
    }
    return TCSFM_OK;
}
}  // namespace

int tcsfm_posenet_tape_size(tcsfm_posenet *pn, int N, int64_t *floats_out) {
    if (!pn) return TCSFM_E_ARG;
    if (N < 1 || N > pn->max_images) return fail(pn->h, TCSFM_E_ARG, "tcsfm_posenet_tape_size: N out of range");
    if (!floats_out) return fail(pn->h, TCSFM_E_ARG, "tcsfm_posenet_tape_size: floats_out is NULL");
    PnTapeLayer t[7];
    *floats_out = (int64_t)pn_tape_layout(pn, N, t);
    return TCSFM_OK;
}

int tcsfm_posenet_forward_train(tcsfm_posenet *pn, int N, const float *imgs, float *pose_out, float *tape) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (int rc = pn_check_train(pn, N, "tcsfm_posenet_forward_train")) return rc;
    if (!imgs) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward_train: imgs is NULL");
    if (!pose_out) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward_train: pose_out is NULL");
    if (!tape) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward_train: tape is NULL");
    if (((uintptr_t)tape & 15) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_forward_train: tape must be 16-byte aligned");
    {
        PnTapeLayer tl[7];
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 6 * h->H * h->W * sizeof(float));
        a.out("pose_out", pose_out, (size_t)N * 6 * sizeof(float));
        a.out("tape", tape, (size_t)pn_tape_layout(pn, N, tl) * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_posenet_forward_train", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    const long long hw = (long long)h->H * h->W;
    return pn_run(pn, N, imgs, 6 * hw, imgs + 3 * hw, 6 * hw, 0, 0, pose_out, 0, nullptr, 0, 1, nullptr, tape);
}

namespace {
// The backward walk, shared by tcsfm_posenet_backward (req null) and tcsfm_posenet_param_backward: one dz per layer feeds the data
// gradient and, where asked for, the parameter gradients.  d_imgs null: layer 1's data gradient is skipped.
int pnb_walk(tcsfm_posenet *pn, int N, const float *imgs, const float *tape, const float *d_pose, float *d_imgs, const PnwReq *req) {
    tcsfm_ctx *h = pn->h;
    PnTapeLayer tl[7];
    pn_tape_layout(pn, N, tl);
    hipStream_t s = h->stream;
    float *da = pn->gbuf[0], *nxt = pn->gbuf[1];
    const int npix7 = pn->L[6].oh * pn->L[6].ow;
    if (req && (req->hw || req->hb))
        hipLaunchKernelGGL(k_pnw_head, dim3(16), dim3(256), 0, s, tape + tl[6].raw, tape + tl[6].scsh, d_pose, req->hw, req->hb, N, npix7);
    int last = 0;            // the lowest layer whose dz somebody needs
    if (!d_imgs) {
        last = 7;
        for (int l = 6; l >= 0; l--)
            if (req && (req->w[l] || req->b[l] || req->g[l] || req->be[l])) last = l;
        if (last == 7) { HIPCHK(h, hipGetLastError()); return TCSFM_OK; }
    }
    hipLaunchKernelGGL(k_pnb_head, dim3(dn_blocks((long long)N * npix7 * 256)), dim3(256), 0, s, d_pose, (const float *)pn->w->head_w, da, N, npix7);
    for (int l = 6; l >= last; l--) {
        const PnLayer &L = pn->L[l];
        PnbNormParams P;
        P.da = da; P.raw = tape + tl[l].raw; P.scsh = tape + tl[l].scsh; P.mr = tape + tl[l].mr; P.gamma = pn->w->gamma[l];
        P.ss = pn->gss; P.dz = da; P.N = N; P.npix = L.oh * L.ow; P.cout = L.cout;
        if (req && (req->be[l] || req->g[l])) pnw_chan(pn, P, 0, req->be[l], req->g[l]);
        hipLaunchKernelGGL(k_pnb_gsum, dim3(N, 16), dim3(256), 0, s, P);
        hipLaunchKernelGGL(k_pnb_dz, dim3(dn_blocks((long long)N * P.npix * (L.cout / 4))), dim3(256), 0, s, P);
        if (req && req->b[l]) pnw_chan(pn, P, 1, req->b[l], nullptr);
        if (req && req->w[l]) pnw_wgrad(pn, l, N, da, l == 0 ? imgs : tape + tl[l - 1].raw, l == 0 ? nullptr : tape + tl[l - 1].scsh, req->w[l]);
        if (l == last) {
            if (l == 0 && d_imgs) {
                const int hh = (L.ih + 1) / 2, wh = (L.iw + 1) / 2;
                hipLaunchKernelGGL(k_pnb_dgrad1, dim3(dn_blocks((long long)hh * wh), 4, N), dim3(256), 0, s, (const float *)da,
                                   (const float *)reinterpret_cast<float *>(pn->wt4[0].p), d_imgs, L.ih, L.iw, L.oh, L.ow);
            }
            break;
        }
        // data gradient onto the layer's input grid: k_dnb_dgrad "direct" (zero padding, stride 2), nothing fused in its epilogue.
        // The split is dn_split's function of (pixels, channel blocks): never of N
        DnDgradParams D;
        D.dz = da; D.wt4 = pn->wt4[l]; D.out = nxt; D.add1 = D.add2 = nullptr; D.y = nullptr; D.act = DN_ACT_NONE;
        D.cin = L.cin; D.cout = L.cout; D.coutp = L.cout; D.gh = L.ih; D.gw = L.iw; D.goff = L.pad; D.oh = L.oh; D.ow = L.ow;
        D.stride = 2; D.direct = 1;
        const int pixels = L.ih * L.iw, cblocks = L.cin / 16;
        const DnSplit sp = dn_split(pixels, cblocks);
        const int wg = 16 * sp.pb * (4 / sp.kw);
        const dim3 grid((pixels + wg - 1) / wg, cblocks / sp.nb, N);
        if (L.ks == 5) dn_launch_ks<DnDgradKernel, 5>(sp, grid, s, D);
        else dn_launch_ks<DnDgradKernel, 3>(sp, grid, s, D);
        std::swap(da, nxt);
    }
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}
}  // namespace

int tcsfm_posenet_backward(tcsfm_posenet *pn, int N, const float *tape, const float *d_pose, float *d_imgs) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (int rc = pn_check_train(pn, N, "tcsfm_posenet_backward")) return rc;
    if (!tape) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_backward: tape is NULL");
    if (((uintptr_t)tape & 15) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_backward: tape must be 16-byte aligned");
    if (!d_pose) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_backward: d_pose is NULL");
    if (!d_imgs) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_backward: d_imgs is NULL");
    {
        PnTapeLayer tl[7];
        ArgRanges a;
        a.in("tape", tape, (size_t)pn_tape_layout(pn, N, tl) * sizeof(float));
        a.in("d_pose", d_pose, (size_t)N * 6 * sizeof(float));
        a.out("d_imgs", d_imgs, (size_t)N * 6 * h->H * h->W * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_posenet_backward", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = pnb_prepare(pn)) return rc;
    return pnb_walk(pn, N, nullptr, tape, d_pose, d_imgs, nullptr);
}

int tcsfm_posenet_param_backward(tcsfm_posenet *pn, int N, const float *imgs, const float *tape, const float *d_pose, float *d_imgs,
                                 float *const conv_w_g[7], float *const conv_b_g[7], float *const gn_w_g[7], float *const gn_b_g[7],
                                 float *head_w_g, float *head_b_g) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (int rc = pn_check_train(pn, N, "tcsfm_posenet_param_backward")) return rc;
    if (!tape) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_param_backward: tape is NULL");
    if (((uintptr_t)tape & 15) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_param_backward: tape must be 16-byte aligned");
    if (!d_pose) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_param_backward: d_pose is NULL");
    PnwReq req;
    for (int l = 0; l < 7; l++) {
        req.w[l] = conv_w_g ? conv_w_g[l] : nullptr; req.b[l] = conv_b_g ? conv_b_g[l] : nullptr;
        req.g[l] = gn_w_g ? gn_w_g[l] : nullptr; req.be[l] = gn_b_g ? gn_b_g[l] : nullptr;
    }
    req.hw = head_w_g; req.hb = head_b_g;
    if (req.w[0] && !imgs) return fail(h, TCSFM_E_ARG, "tcsfm_posenet_param_backward: imgs is NULL (conv1's weight gradient reads the images)");
    {
        PnTapeLayer tl[7];
        ArgRanges a;
        const size_t img_b = (size_t)N * 6 * h->H * h->W * sizeof(float);
        if (req.w[0]) a.in("imgs", imgs, img_b);
        a.in("tape", tape, (size_t)pn_tape_layout(pn, N, tl) * sizeof(float));
        a.in("d_pose", d_pose, (size_t)N * 6 * sizeof(float));
        a.out("d_imgs", d_imgs, img_b);
        for (int l = 0; l < 7; l++) {
            const PnLayer &L = pn->L[l];
            a.out("conv_w_g", req.w[l], (size_t)L.cout * L.cin * L.ks * L.ks * sizeof(float), l);
            a.out("conv_b_g", req.b[l], L.cout * sizeof(float), l); a.out("gn_w_g", req.g[l], L.cout * sizeof(float), l);
            a.out("gn_b_g", req.be[l], L.cout * sizeof(float), l);
        }
        a.out("head_w_g", head_w_g, 6 * 256 * sizeof(float)); a.out("head_b_g", head_b_g, 6 * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_posenet_param_backward", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = pnb_prepare(pn)) return rc;
    if (int rc = pnw_prepare(pn)) return rc;
    return pnb_walk(pn, N, imgs, tape, d_pose, d_imgs, &req);
}

int tcsfm_debug_posenet_tape_layer(tcsfm_posenet *pn, int N, const float *tape, int layer, float *raw_out, float *scsh_out,
                                   float *mean_rstd_out, float *act_out) {
    if (!pn) return TCSFM_E_ARG;
    tcsfm_ctx *h = pn->h;
    if (N < 1 || N > pn->max_images) return fail(h, TCSFM_E_ARG, "tcsfm_debug_posenet_tape_layer: N out of range");
    if (!tape) return fail(h, TCSFM_E_ARG, "tcsfm_debug_posenet_tape_layer: tape is NULL");
    if (layer < 1 || layer > 7) return fail(h, TCSFM_E_ARG, "tcsfm_debug_posenet_tape_layer: layer out of range");
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    PnTapeLayer tl[7];
    pn_tape_layout(pn, N, tl);
    const PnLayer &L = pn->L[layer - 1];
    const PnTapeLayer &t = tl[layer - 1];
    const size_t nraw = (size_t)N * L.oh * L.ow * L.cout;
    if (raw_out) HIPCHK(h, hipMemcpyAsync(raw_out, tape + t.raw, nraw * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (scsh_out) HIPCHK(h, hipMemcpyAsync(scsh_out, tape + t.scsh, (size_t)N * L.cout * 2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (mean_rstd_out) HIPCHK(h, hipMemcpyAsync(mean_rstd_out, tape + t.mr, (size_t)N * 32 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (act_out) {
        hipLaunchKernelGGL(k_pnb_act, dim3(dn_blocks((long long)nraw)), dim3(256), 0, h->stream, tape + t.raw, tape + t.scsh, act_out, N, L.oh * L.ow, L.cout);
        HIPCHK(h, hipGetLastError());
    }
    return TCSFM_OK;
}
