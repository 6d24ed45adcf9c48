// Host side of the PoseNet's parameter gradients (posenet_wgrad_kernel.h): the requests of a call, the scratch and the per-layer
// launches that tcsfm_posenet_param_backward's walk (posenet_grad_host.h) makes beside the data gradient.  Part of tcsfm_api.hip, the
// library's only translation unit: included after posenet_host.h and before posenet_grad_host.h.
#pragma once

namespace {
// the gradients a call asks for (NULL: not wanted, its work is skipped)
struct PnwReq {
    float *w[7] = {}, *b[7] = {}, *g[7] = {}, *be[7] = {};
    float *hw = nullptr, *hb = nullptr;
};

// Split of a layer's R = N npix rows into contiguous parts.  Enough parts that a layer has ~1024 workgroups (layers 5..7 have a few
// hundred rows in all and 64..128 (ci, co) blocks), never fewer than 64 rows per part (4 steps per wave), at most 2048 rows per
// part (512 products per fp32 accumulator) unless that would take more than the cap: 256 parts, or what PNW_PART_FLOATS of partials
// hold.  A function of (R, layer) only.
constexpr long long PNW_PART_FLOATS = 16LL << 20;
struct PnwSplit { long long rpp; int parts; };
int pnw_mb(const PnLayer &L) { return L.ks == 7 ? 1 : 2; }      // channel blocks of 16 per workgroup: an input load feeds both
int pnw_base(const PnLayer &L) { return (L.ks == 7 ? 3 : L.ks == 5 ? 5 * (L.cin / 16) : L.cin / 16) * (L.cout / (16 * pnw_mb(L))); }
long long pnw_want(long long R, const PnLayer &L) {       // parts <= this; it grows with R up to the cap
    const int base = pnw_base(L);
    const long long E = (long long)L.cout * L.cin * L.ks * L.ks, cap = std::max(1LL, std::min(256LL, PNW_PART_FLOATS / E));
    const long long want = std::max((R + 2047) / 2048, std::min((long long)(1024 + base - 1) / base, (R + 63) / 64));
    return std::max(1LL, std::min(want, cap));
}
PnwSplit pnw_split(long long R, const PnLayer &L) {
    const long long want = pnw_want(R, L);
    PnwSplit s;
    s.rpp = (((R + want - 1) / want) + 15) / 16 * 16;
    s.parts = (int)((R + s.rpp - 1) / s.rpp);
    return s;
}

int pnw_prepare(tcsfm_posenet *pn) {
    tcsfm_ctx *h = pn->h;
    hipError_t e = hipSuccess;
    {
        size_t fl = 0;
        for (int l = 0; l < 7; l++) {
            const PnLayer &L = pn->L[l];
            fl = std::max(fl, (size_t)pnw_want((long long)pn->max_images * L.oh * L.ow, L) * L.cout * L.cin * L.ks * L.ks);
        }
        e = DEV_RESERVE(pn->wpart, fl);
    }
    if (e == hipSuccess) e = DEV_RESERVE(pn->cpart, (size_t)16384 * 2);
    if (e != hipSuccess) return fail_alloc(h, e, "tcsfm_posenet_param_backward: allocation failed");
    return TCSFM_OK;
}

// per-channel sums of layer l: mode 0 (before k_pnb_dz) -> d beta, d gamma; mode 1 (after it, P.da = dz) -> d bias
void pnw_chan(tcsfm_posenet *pn, const PnbNormParams &P, int mode, float *out0, float *out1) {
    hipStream_t s = pn->h->stream;
    const long long R = (long long)P.N * P.npix;
    const int want = (int)std::max(1LL, std::min((long long)(16384 / P.cout), (R + 255) / 256));      // cpart holds 16384 pairs
    const long long rpp = (R + want - 1) / want;
    const int parts = (int)((R + rpp - 1) / rpp);
    hipLaunchKernelGGL(k_pnw_chan, dim3(P.cout / 16, parts), dim3(256), 0, s, P, pn->cpart, rpp, mode);
    hipLaunchKernelGGL(k_pnw_chan_sum, dim3(P.cout), dim3(256), 0, s, (const double *)pn->cpart, out0, out1, P.cout, parts);
}

// weight gradient of layer l (0-based) from dz: partials, then their sum and conv2d_wn's chain rule into dw.
// x / scsh: the previous layer's taped raw output and (scale, shift) pairs (l == 0: the images, scsh unused)
void pnw_wgrad(tcsfm_posenet *pn, int l, int N, const float *dz, const float *x, const float *scsh, float *dw) {
    const PnLayer &L = pn->L[l];
    hipStream_t s = pn->h->stream;
    PnWgradParams P;
    P.dz = dz; P.x = x; P.scsh = scsh; P.part = pn->wpart;
    P.rows = (long long)N * L.oh * L.ow;
    const PnwSplit sp = pnw_split(P.rows, L);
    P.rows_per_part = sp.rpp;
    P.cin = L.cin; P.cout = L.cout; P.ih = L.ih; P.iw = L.iw; P.oh = L.oh; P.ow = L.ow; P.pad = L.pad;
    if (L.ks == 7) hipLaunchKernelGGL((k_pnw_wgrad<7, 1, PNW_FIRST>), dim3(sp.parts, 3, L.cout / 16), dim3(256), 0, s, P);
    else if (L.ks == 5) hipLaunchKernelGGL((k_pnw_wgrad<5, 2, PNW_ROW>), dim3(sp.parts, 5 * (L.cin / 16), L.cout / 32), dim3(256), 0, s, P);
    else hipLaunchKernelGGL((k_pnw_wgrad<3, 2, PNW_ALL>), dim3(sp.parts, L.cin / 16, L.cout / 32), dim3(256), 0, s, P);
    const int n = L.cin * L.ks * L.ks;
    const long long E = (long long)L.cout * n;
    hipLaunchKernelGGL(k_pnw_psum, dim3(dn_blocks(E)), dim3(256), 0, s, (const float *)pn->wpart, dw, E, sp.parts);
    hipLaunchKernelGGL(k_pnw_wstd, dim3(L.cout), dim3(256), 0, s, (const float *)pn->w->raww[l], dw, n);
}
}  // namespace
