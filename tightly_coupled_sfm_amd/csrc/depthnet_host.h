// Host side of the depth network (models/depth_w_access.py, num_scales = 1): ResNet18 encoder + U-Net decoder -- the topology, the work
// split, the forward walks, the tapes of the training forward, the backward walks and the tcsfm_depthnet_* entry points.
// Part of tcsfm_api.hip, the library's only translation unit: included after context.h (tcsfm_ctx, fail, fail_alloc, HIPCHK, DEV_RESERVE, DeviceGuard)
// and call_host.h (drain_queued) and the kernels' headers, and before the sequence driver, whose depth stage is dn_sequence_depths.  include/tcsfm.h
// declares the entry points, so they have C linkage here.
#pragma once
#include <memory>

namespace {
constexpr int DN_BLOCKS = 8, DN_UPS = 5;                       // residual blocks of the encoder, up-steps of the decoder
constexpr int DN_HEAD_W = 72, DN_HEAD_N = DN_HEAD_W + 1;       // predict_disps.0: weight [1,8,3,3], then its bias
const int DN_SKIP_C[5] = {64, 64, 128, 256, 512};
// up-step i adds skip 3 - i to its up-convolution; the last one has no skip left (the only place that says which)
constexpr bool dn_adds_skip(int i) { return i < DN_UPS - 1; }
unsigned dn_blocks(long long threads) { return (unsigned)((threads + 255) / 256); }       // grid of an elementwise launch

// Work split of a convolution-shaped kernel <KS, NB, PB, KW>: NB blocks of 16 channels and PB blocks of 16 pixels per wave, KW waves
// sharing one K loop.  A function of the pixels per image and the channel blocks only (never of N).
struct DnSplit { int nb, pb, kw; };
DnSplit dn_split(int pixels, int cblocks) {
    if (pixels >= 4096) return {std::min(4, cblocks), 2, 1};
    if (pixels >= 1024) return {std::min(2, cblocks), 1, 4};
    return {1, 1, 4};
}

struct DnLayer {
    int cin = 0, cout = 0, coutp = 0, ks = 0, stride = 1, pad = 0, up = 0, reflect = 0, epi = DN_EPI_NONE;
    int ih = 0, iw = 0, oh = 0, ow = 0;
    DnSplit sp = {1, 1, 1};             // of k_dn_conv: dn_split(oh * ow, coutp / 16)
    std::string wname, bname, bn;       // state_dict names: conv weight, conv bias ("" = none), BatchNorm prefix ("" = none)
    // training (tcsfm_depthnet_load_device), views into the instance's DnTrain: the transposed weight image of the data gradient (not for
    // conv1), the raw parameters' snapshot (w [cout][cin][ks][ks], then conv bias, gamma, beta, mean, var [cout] each) and the
    // folded-gradient accumulators (dw' [cout][cin ks ks], db' [cout])
    dn_f4 *wt4 = nullptr;
    float *raw = nullptr, *gw = nullptr, *gb = nullptr;
    int taps() const { return ks * ks; }
    size_t nw() const { return (size_t)cout * cin * ks * ks; }
    size_t w4_count() const { return (ks == 7 ? 11 : (size_t)taps() * (cin / 16)) * 4 * coutp; }     // dn_f4 elements of w4
    size_t map() const { return (size_t)oh * ow * cout; }                                             // floats of an image's output
};

// A residual block of the encoder: convolutions li (conv1) and li + 1 (conv2), and li + 2, the 1x1 downsample of its input, if `down`.
// Block j reads block j - 1's output (block 0 the pooled map); `skip`: which skip its output is (-1: none).
struct DnBlock { int li, down, skip; };

// What a load fills and every instance's launches read, per layer of tcsfm_depthnet::L: the folded weight image and the bias [coutp];
// predict_disps.0 weight [1,8,3,3] / bias [1].  A reload fills them in place.
struct DnWeights {
    std::vector<DevBuf<dn_f4>> w4;
    std::vector<DevBuf<float>> bias;
    DevBuf<float> pw, pb;
};

// The training state (allocated by the first tcsfm_depthnet_load_device; the primary's only)
struct DnTrain {
    DevBuf<float> tbuf;                 // one allocation: the layers' raw / gw / gb regions and the head's gradient accumulator
    float *hacc = nullptr;              // head: d predict_disps weight [DN_HEAD_W] + bias [1] (a view into tbuf)
    DevBuf<float> part, bpart, hpart;   // weight / bias / head partials of one image group
    DevBuf<float> gA, gB, gC, gD, gV;   // data-gradient scratch
    std::vector<DevBuf<dn_f4>> wt4;     // per layer: DnLayer::wt4
};
}  // namespace

struct tcsfm_depthnet {
    tcsfm_ctx *h = nullptr;
    int max_images = 0, loaded = 0;
    std::vector<DnLayer> L;             // [0] conv1, then the encoder's block convolutions, then the decoder (order of dn_layers)
    DnBlock blk[DN_BLOCKS] = {};
    int enc_end = 0;                    // index of the first decoder layer
    int up(int i) const { return enc_end + 2 * i; }       // up-convolution / iconv of up-step i, feature_convs.0
    int iconv(int i) const { return up(i) + 1; }
    int feat() const { return up(DN_UPS); }
    DnWeights own;                      // the primary's weights (empty in the clone)
    const DnWeights *w = &own;          // the weights the launches read: the primary's
    DevBuf<float> skip_own[5];          // tcsfm_depthnet_forward's own skips, NHWC ...
    float *skip[5] = {};                // ... as the table the walks take
    DevBuf<float> pool, t1, t2, ds;     // encoder scratch, N * H * W * 4 floats each
    DevBuf<float> u, x;                 // decoder scratch, N * H * W * 32 floats each
    // tcsfm_depthnet_disp_for_eigen / the sequence calls' disparity stage: scaled-disparity planes of ONE group of max_images images,
    // the straight pass's and the mirrored pass's (still mirrored); allocated on first use (dn_post_scratch), owned by the instance
    DevBuf<float> post_l, post_r;
    int train_loaded = 0;
    DnTrain train;
    // tcsfm_sequence_depthnet: the sequence calls' depth stage runs on `seq_clone` -- an instance of its own that READS this network's
    // weights through `w` (a reload fills them in place), with its own activations and no training state, and whose forward launches go
    // to `stream` (the handle's seq_pack) instead of the handle's stream.  It goes before this instance's weights do.
    hipStream_t stream = nullptr;       // forward launches go here when set (dn_stream)
    std::unique_ptr<tcsfm_depthnet> seq_clone;
};

namespace {
DnLayer dn_layer(int cin, int cout, int ks, int stride, int ih, int iw, int up, int reflect, int epi, const std::string &w,
                 const std::string &b, const std::string &bn) {
    DnLayer l;
    l.cin = cin; l.cout = cout; l.coutp = (cout + 15) / 16 * 16; l.ks = ks; l.stride = stride; l.pad = (ks - 1) / 2;
    l.up = up; l.reflect = reflect; l.epi = epi; l.ih = ih; l.iw = iw;
    const int vh = ih << up, vw = iw << up;
    l.oh = (vh + 2 * l.pad - ks) / stride + 1; l.ow = (vw + 2 * l.pad - ks) / stride + 1;
    l.wname = w; l.bname = b; l.bn = bn;
    l.sp = dn_split(l.oh * l.ow, l.coutp / 16);
    return l;
}

// the network's convolutions in evaluation order, and the encoder's block table
void dn_layers(tcsfm_depthnet *dn) {
    const int H = dn->h->H, W = dn->h->W;
    const std::string E = "encoder.encoder.";
    auto &L = dn->L;
    L.clear();
    L.push_back(dn_layer(3, 64, 7, 2, H, W, 0, 0, DN_EPI_RELU, E + "conv1.weight", "", E + "bn1"));
    L.back().oh = H / 2; L.back().ow = W / 2;
    int h = H / 4, w = W / 4, c = 64;
    for (int j = 0; j < DN_BLOCKS; j++) {
        const int stage = j / 2 + 1, b = j % 2, co = 64 << (stage - 1), down = b == 0 && stage > 1;
        const std::string pre = E + "layer" + std::to_string(stage) + "." + std::to_string(b) + ".";
        dn->blk[j] = {(int)L.size(), down, b == 1 ? stage : -1};
        L.push_back(dn_layer(c, co, 3, down ? 2 : 1, h, w, 0, 0, DN_EPI_RELU, pre + "conv1.weight", "", pre + "bn1"));
        const int oh = L.back().oh, ow = L.back().ow;
        L.push_back(dn_layer(co, co, 3, 1, oh, ow, 0, 0, DN_EPI_RES_RELU, pre + "conv2.weight", "", pre + "bn2"));
        if (down) L.push_back(dn_layer(c, co, 1, 2, h, w, 0, 0, DN_EPI_NONE, pre + "downsample.0.weight", "", pre + "downsample.1"));
        h = oh; w = ow; c = co;
    }
    dn->enc_end = (int)L.size();
    static const int planes[DN_UPS + 1] = {512, 256, 128, 64, 64, 32};
    for (int i = 0; i < DN_UPS; i++) {
        const std::string u = "depth_upconvs." + std::to_string(i) + ".1.conv.", ic = "iconvs." + std::to_string(i) + ".0.conv.";
        L.push_back(dn_layer(planes[i], planes[i + 1], 3, 1, h, w, 1, 1, dn_adds_skip(i) ? DN_EPI_ELU_ADD : DN_EPI_ELU, u + "weight", u + "bias", ""));
        h *= 2; w *= 2;
        L.push_back(dn_layer(planes[i + 1], planes[i + 1], 3, 1, h, w, 0, 1, DN_EPI_ELU, ic + "weight", ic + "bias", ""));
    }
    L.push_back(dn_layer(32, 8, 3, 1, h, w, 0, 1, DN_EPI_ELU, "feature_convs.0.0.conv.weight", "feature_convs.0.0.conv.bias", ""));
}

// dn_train_alloc's failure path: the training buffers go, and the layers' views into them
void dn_train_free(tcsfm_depthnet *dn) {
    dn->train = DnTrain();
    for (DnLayer &l : dn->L) { l.wt4 = nullptr; l.raw = l.gw = l.gb = nullptr; }
}

hipError_t dn_alloc_scratch(tcsfm_depthnet *dn) {
    const size_t N = (size_t)dn->max_images, hw = (size_t)dn->h->H * dn->h->W;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 5 && e == hipSuccess; k++) {
        e = DEV_RESERVE(dn->skip_own[k], N * (hw >> (2 * (k + 1))) * DN_SKIP_C[k]);
        dn->skip[k] = dn->skip_own[k];
    }
    for (DevBuf<float> *p : {&dn->pool, &dn->t1, &dn->t2, &dn->ds}) if (e == hipSuccess) e = DEV_RESERVE(*p, N * hw * 4);       // (H/4)(W/4) x 64 = H W x 4
    if (e == hipSuccess) e = DEV_RESERVE(dn->u, N * hw * 32);
    if (e == hipSuccess) e = DEV_RESERVE(dn->x, N * hw * 32);
    return e;
}

// forward launches of an instance: the handle's stream, or the sequence calls' stage stream for the clone they run
hipStream_t dn_stream(const tcsfm_depthnet *dn) { return dn->stream ? dn->stream : dn->h->stream; }

// the instance the sequence calls run `dn`'s network on (pn_for_lane's pattern): the geometry and work split of `dn`'s handle, `dn`'s
// weights to read, its own skips and scratch, no training state.  The caller binds its `stream` per call.
tcsfm_depthnet *dn_sequence_clone(tcsfm_depthnet *dn) {
    if (dn->seq_clone) return dn->seq_clone.get();
    std::unique_ptr<tcsfm_depthnet> q(new tcsfm_depthnet());
    q->h = dn->h; q->max_images = dn->max_images; q->loaded = dn->loaded; q->w = dn->w;
    dn_layers(q.get());
    if (dn_alloc_scratch(q.get()) != hipSuccess) return nullptr;
    dn->seq_clone = std::move(q);
    return dn->seq_clone.get();
}

// ---- the split kernels' dispatch: k_dn_conv (pixels = oh ow, blocks = coutp / 16) and k_dnb_dgrad (pixels = lane grid, blocks = cin / 16)
struct DnConvKernel {
    template <int KS, int NB, int PB, int KW>
    static void launch(dim3 grid, hipStream_t s, const DnConvParams &P) { hipLaunchKernelGGL((k_dn_conv<KS, NB, PB, KW>), grid, dim3(256), 0, s, P); }
};
struct DnDgradKernel {
    template <int KS, int NB, int PB, int KW>
    static void launch(dim3 grid, hipStream_t s, const DnDgradParams &P) { hipLaunchKernelGGL((k_dnb_dgrad<KS, NB, PB, KW>), grid, dim3(256), 0, s, P); }
};

template <class K, int KS, class Params>
void dn_launch_ks(DnSplit s, dim3 grid, hipStream_t st, const Params &P) {
    if (s.kw == 1 && s.nb == 4) K::template launch<KS, 4, 2, 1>(grid, st, P);
    else if (s.kw == 1 && s.nb == 2) K::template launch<KS, 2, 2, 1>(grid, st, P);
    else if (s.kw == 1) K::template launch<KS, 1, 2, 1>(grid, st, P);
    else if (s.nb == 2) K::template launch<KS, 2, 1, 4>(grid, st, P);
    else K::template launch<KS, 1, 1, 4>(grid, st, P);
}

template <class K, class Params>
void dn_launch_split(int ks, DnSplit s, int pixels, int cblocks, int N, const Params &P, hipStream_t stream) {
    const int wg = 16 * s.pb * (4 / s.kw);      // pixels of a workgroup
    const dim3 grid((pixels + wg - 1) / wg, cblocks / s.nb, N);
    if (ks == 1) dn_launch_ks<K, 1>(s, grid, stream, P);
    else dn_launch_ks<K, 3>(s, grid, stream, P);
}

void dn_conv(tcsfm_depthnet *dn, int li, int N, const float *in, const float *res, float *out, float *aux = nullptr) {
    const DnLayer &l = dn->L[li];
    DnConvParams P;
    P.in = in; P.w4 = dn->w->w4[li]; P.bias = dn->w->bias[li]; P.res = res; P.out = out; P.aux = aux;
    P.cin = l.cin; P.cout = l.cout; P.coutp = l.coutp; P.ih = l.ih; P.iw = l.iw; P.oh = l.oh; P.ow = l.ow;
    P.stride = l.stride; P.pad = l.pad; P.up = l.up; P.reflect = l.reflect; P.epi = l.epi;
    dn_launch_split<DnConvKernel>(l.ks, l.sp, l.oh * l.ow, l.coutp / 16, N, P, dn_stream(dn));
}

// ---- tapes of the training forward.  A tape of N images is a list of entries, each [N][per-image size] (entry-major), so a group of
// images [i0, i1) of a chunked call is a pointer offset in every entry.
// Encoder entries: the images, conv1's output (skip 0), the pooled map, then per block j conv1's output (t1) and the block's output.
enum { DN_TE_IMAGES, DN_TE_CONV1, DN_TE_POOL, DN_TE_BLOCKS };
constexpr int dn_te_t1(int j) { return DN_TE_BLOCKS + 2 * j; }
constexpr int dn_te_out(int j) { return dn_te_t1(j) + 1; }
// Decoder entries: skip 4, then per up-step i the up-convolution's ELU before the skip add (an entry only where a skip is added, before
// u; otherwise it IS u), the up-convolution's output u, the iconv's output x; then the features and the disparity.
enum { DN_TD_SKIP4, DN_TD_UPS };
constexpr int dn_td_u(int i) { return DN_TD_UPS + 3 * i + (dn_adds_skip(i) ? 1 : 0); }       // (the step without a skip is the last one)
constexpr int dn_td_elu(int i) { return dn_td_u(i) - (dn_adds_skip(i) ? 1 : 0); }
constexpr int dn_td_x(int i) { return dn_td_u(i) + 1; }
constexpr int DN_TD_FEAT = dn_td_x(DN_UPS - 1) + 1, DN_TD_DISP = DN_TD_FEAT + 1;

struct DnTape {
    std::vector<size_t> sz, off;        // per-image floats of each entry; offset of each entry for N images
    float *base = nullptr;
    int N = 0;
    float *at(int k, int i0) const { return base + off[k] + (size_t)i0 * sz[k]; }
    size_t total() const { size_t t = 0; for (size_t s : sz) t += s; return t * N; }
};

DnTape dn_tape_layout(const tcsfm_depthnet *dn, int dec, int N, float *base) {
    const size_t hw = (size_t)dn->h->H * dn->h->W;
    DnTape t;
    if (!dec) {
        const DnLayer &c1 = dn->L[0];
        t.sz.resize(dn_te_out(DN_BLOCKS - 1) + 1);
        t.sz[DN_TE_IMAGES] = 3 * hw; t.sz[DN_TE_CONV1] = c1.map(); t.sz[DN_TE_POOL] = (size_t)(c1.oh / 2) * (c1.ow / 2) * c1.cout;
        for (int j = 0; j < DN_BLOCKS; j++) t.sz[dn_te_t1(j)] = t.sz[dn_te_out(j)] = dn->L[dn->blk[j].li].map();
    } else {
        const DnLayer &u0 = dn->L[dn->up(0)];
        t.sz.resize(DN_TD_DISP + 1);
        t.sz[DN_TD_SKIP4] = (size_t)u0.ih * u0.iw * u0.cin;
        for (int i = 0; i < DN_UPS; i++) t.sz[dn_td_elu(i)] = t.sz[dn_td_u(i)] = t.sz[dn_td_x(i)] = dn->L[dn->up(i)].map();
        t.sz[DN_TD_FEAT] = hw * 8; t.sz[DN_TD_DISP] = hw;
    }
    t.off.assign(t.sz.size(), 0);
    size_t o = 0;
    for (size_t k = 0; k < t.sz.size(); k++) { t.off[k] = o; o += t.sz[k] * N; }
    t.base = base; t.N = N;
    return t;
}

// ---- forward walks.  Where each launch's output goes: the instance's scratch (inference) or a tape's entries (training).
struct DnEncDst { float *conv1, *pool, *t1[DN_BLOCKS], *out[DN_BLOCKS]; };
struct DnDecDst {
    float *aux[DN_UPS], *u[DN_UPS], *x[DN_UPS], *feat, *disp;
    int as_depth = 0;                   // the head stores disp_to_depth's depth (of min_disp, max_disp) into `disp` instead: k_dn_predict<true>
    float min_disp = 0.f, max_disp = 0.f;
    // disp_post_kernel.h k_dn_head: with as_depth, ALSO disp_to_depth's scaled disparity into `scaled`; scaled_only: that alone, into `disp`
    float *scaled = nullptr;
    int scaled_only = 0;
};

// a stage's first block leaves its output in t2 (its input is the pooled map or a skip), the second one in the stage's skip
DnEncDst dn_enc_scratch(const tcsfm_depthnet *dn, float *const sk[5]) {
    DnEncDst d = {sk[0], dn->pool, {}, {}};
    for (int j = 0; j < DN_BLOCKS; j++) { d.t1[j] = dn->t1; d.out[j] = dn->blk[j].skip >= 0 ? sk[dn->blk[j].skip] : dn->t2; }
    return d;
}
DnEncDst dn_enc_tape(const DnTape &t, int i0) {
    DnEncDst d = {t.at(DN_TE_CONV1, i0), t.at(DN_TE_POOL, i0), {}, {}};
    for (int j = 0; j < DN_BLOCKS; j++) { d.t1[j] = t.at(dn_te_t1(j), i0); d.out[j] = t.at(dn_te_out(j), i0); }
    return d;
}
DnDecDst dn_dec_scratch(const tcsfm_depthnet *dn, float *disp) {
    DnDecDst d = {{}, {}, {}, dn->u, disp};
    for (int i = 0; i < DN_UPS; i++) { d.u[i] = dn->u; d.x[i] = dn->x; }
    return d;
}
DnDecDst dn_dec_tape(const DnTape &t, int i0) {
    DnDecDst d = {{}, {}, {}, t.at(DN_TD_FEAT, i0), t.at(DN_TD_DISP, i0)};
    for (int i = 0; i < DN_UPS; i++) { d.aux[i] = dn_adds_skip(i) ? t.at(dn_td_elu(i), i0) : nullptr; d.u[i] = t.at(dn_td_u(i), i0); d.x[i] = t.at(dn_td_x(i), i0); }
    return d;
}

int dn_encode(tcsfm_depthnet *dn, int N, const float *imgs, int flip, const DnEncDst &d) {
    tcsfm_ctx *h = dn->h;
    const DnLayer &c1 = dn->L[0];
    DnConv1Params P1;
    P1.img = imgs; P1.w4 = dn->w->w4[0]; P1.bias = dn->w->bias[0]; P1.out = d.conv1; P1.ih = h->H; P1.iw = h->W; P1.oh = c1.oh; P1.ow = c1.ow; P1.flip = flip ? 1 : 0;
    hipLaunchKernelGGL(k_dn_conv1<2>, dim3((c1.oh * c1.ow + 127) / 128, 1, N), dim3(256), 0, dn_stream(dn), P1);
    const int ph = c1.oh / 2, pw = c1.ow / 2;
    hipLaunchKernelGGL(k_dn_maxpool, dim3(dn_blocks((long long)N * ph * pw * 16)), dim3(256), 0, dn_stream(dn), (const float *)d.conv1, d.pool, N, 64, c1.oh,
                       c1.ow, ph, pw);
    const float *x = d.pool;
    for (int j = 0; j < DN_BLOCKS; j++) {
        const DnBlock &b = dn->blk[j];
        dn_conv(dn, b.li, N, x, nullptr, d.t1[j]);                                      // conv1 + bn1 + relu
        const float *ident = x;
        if (b.down) { dn_conv(dn, b.li + 2, N, x, nullptr, dn->ds); ident = dn->ds; }   // downsample.0 + downsample.1
        dn_conv(dn, b.li + 1, N, d.t1[j], ident, d.out[j]);                             // conv2 + bn2 + identity, relu
        x = d.out[j];
    }
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int dn_decode(tcsfm_depthnet *dn, int N, const float *const sk[5], const DnDecDst &d) {
    tcsfm_ctx *h = dn->h;
    const float *x = sk[4];
    for (int i = 0; i < DN_UPS; i++) {
        dn_conv(dn, dn->up(i), N, x, dn_adds_skip(i) ? sk[3 - i] : nullptr, d.u[i], d.aux[i]);   // ELU(conv3x3_reflect(up2(x)) + b) (+ skip)
        dn_conv(dn, dn->iconv(i), N, d.u[i], nullptr, d.x[i]);                                   // ELU(conv3x3_reflect(.) + b)
        x = d.x[i];
    }
    dn_conv(dn, dn->feat(), N, x, nullptr, d.feat);                                              // feature_convs.0: 32 -> 8, ELU
    const dim3 head_grid(dn_blocks((long long)N * h->H * h->W));
    if (d.scaled_only)
        hipLaunchKernelGGL(k_dn_head<DN_HEAD_SCALED>, head_grid, dim3(256), 0, dn_stream(dn), (const float *)d.feat, (const float *)dn->w->pw, (const float *)dn->w->pb,
                           d.disp, (float *)nullptr, N, h->H, h->W, d.min_disp, d.max_disp);
    else if (d.as_depth && d.scaled)
        hipLaunchKernelGGL(k_dn_head<DN_HEAD_DEPTH_SCALED>, head_grid, dim3(256), 0, dn_stream(dn), (const float *)d.feat, (const float *)dn->w->pw, (const float *)dn->w->pb,
                           d.disp, d.scaled, N, h->H, h->W, d.min_disp, d.max_disp);
    else if (d.as_depth)
        hipLaunchKernelGGL(k_dn_predict<true>, head_grid, dim3(256), 0, dn_stream(dn), (const float *)d.feat, (const float *)dn->w->pw, (const float *)dn->w->pb,
                           d.disp, N, h->H, h->W, d.min_disp, d.max_disp);
    else
        hipLaunchKernelGGL(k_dn_predict<false>, head_grid, dim3(256), 0, dn_stream(dn), (const float *)d.feat, (const float *)dn->w->pw, (const float *)dn->w->pb,
                           d.disp, N, h->H, h->W, 0.f, 0.f);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

// the tensors of a state_dict by name for every layer (names / shapes checked; the error names the key)
struct DnSrc { const float *w = nullptr, *cb = nullptr, *g = nullptr, *be = nullptr, *rm = nullptr, *rv = nullptr; };
int dn_lookup(tcsfm_depthnet *dn, const char *fn, int n, const char *const names[], const float *const ptrs[], const int64_t *shapes,
              std::vector<DnSrc> &src, const float **pw, const float **pb) {
    tcsfm_ctx *h = dn->h;
    const std::string pre = std::string(fn) + ": ";
    if (n < 0 || (n > 0 && (!names || !ptrs || !shapes))) return fail(h, TCSFM_E_ARG, (pre + "NULL argument").c_str());
    for (int i = 0; i < n; i++) {
        if (!names[i]) return fail(h, TCSFM_E_ARG, (pre + "NULL name").c_str());
        if (!strncmp(names[i], "feature_convs.1.", 16) || !strncmp(names[i], "predict_disps.1.", 16)) {
            h->err = pre + names[i] + ": num_scales > 1 is not supported";
            return TCSFM_E_ARG;
        }
    }
    auto find = [&](const std::string &key, std::vector<int64_t> shape, const float **ptr) -> int {
        for (int i = 0; i < n; i++)
            if (key == names[i]) {
                bool ok = ptrs[i] != nullptr;
                for (int d = 0; d < 4; d++) ok = ok && shapes[4 * i + d] == (d < (int)shape.size() ? shape[d] : 0);
                if (!ok) {
                    std::string s = "(";
                    for (size_t d = 0; d < shape.size(); d++) s += (d ? "," : "") + std::to_string(shape[d]);
                    h->err = pre + key + ": missing data or wrong shape (expected " + s + "))";
                    if (key == "predict_disps.0.0.conv.weight" && shapes[4 * i + 1] != 8) h->err += ": num_scales > 1 is not supported";
                    return TCSFM_E_ARG;
                }
                *ptr = ptrs[i];
                return TCSFM_OK;
            }
        h->err = pre + key + ": missing";
        return TCSFM_E_ARG;
    };
    src.assign(dn->L.size(), DnSrc());
    for (size_t li = 0; li < dn->L.size(); li++) {
        const DnLayer &l = dn->L[li];
        DnSrc &p = src[li];
        int rc;
        if ((rc = find(l.wname, {l.cout, l.cin, l.ks, l.ks}, &p.w))) return rc;
        if (!l.bname.empty() && (rc = find(l.bname, {l.cout}, &p.cb))) return rc;
        if (!l.bn.empty()) {
            if ((rc = find(l.bn + ".weight", {l.cout}, &p.g)) || (rc = find(l.bn + ".bias", {l.cout}, &p.be)) ||
                (rc = find(l.bn + ".running_mean", {l.cout}, &p.rm)) || (rc = find(l.bn + ".running_var", {l.cout}, &p.rv))) return rc;
        }
    }
    int rc;
    if ((rc = find("predict_disps.0.0.conv.weight", {1, 8, 3, 3}, pw)) || (rc = find("predict_disps.0.0.conv.bias", {1}, pb))) return rc;
    return TCSFM_OK;
}

int dn_check(tcsfm_depthnet *dn, int N, const char *fn) {
    tcsfm_ctx *h = dn->h;
    if (!dn->loaded) { h->err = std::string(fn) + ": no weights loaded"; return TCSFM_E_ARG; }
    if (N < 1 || N > dn->max_images) { h->err = std::string(fn) + ": N out of range (1 .. max_images)"; return TCSFM_E_ARG; }
    return TCSFM_OK;
}

int dn_check_train(tcsfm_depthnet *dn, int N, const char *fn) {
    tcsfm_ctx *h = dn->h;
    if (!dn->train_loaded) { h->err = std::string(fn) + ": no parameters loaded with tcsfm_depthnet_load_device"; return TCSFM_E_ARG; }
    if (N < 1) { h->err = std::string(fn) + ": N out of range"; return TCSFM_E_ARG; }
    return TCSFM_OK;
}

// Runs f(n, i0, tape, skips) over the groups of at most max_images images [i0, i0 + n) of a training call on N images: the tape laid out
// for all N, `skips` the group's part of the caller's NHWC skip tensors (NULL where the caller passed none).
template <typename P, class F>
int dn_for_groups(tcsfm_depthnet *dn, int dec, int N, const float *tape, P const *skips, F f) {
    const DnTape t = dn_tape_layout(dn, dec, N, const_cast<float *>(tape));
    const size_t hw = (size_t)dn->h->H * dn->h->W;
    for (int i0 = 0; i0 < N; i0 += dn->max_images) {
        P sk[5];
        for (int k = 0; k < 5; k++) sk[k] = skips && skips[k] ? skips[k] + (size_t)i0 * (hw >> (2 * (k + 1))) * DN_SKIP_C[k] : nullptr;
        if (int rc = f(std::min(N - i0, dn->max_images), i0, t, sk)) return rc;
    }
    return TCSFM_OK;
}

// ---- training: device re-fold, data / weight gradients -------------------------------------------------------------------------
int dn_wchunk(int npix) { return npix <= 2048 ? npix : 2048; }     // weight-gradient K chunk (pixels of one image): geometry only
int dn_nchunk(int npix) { const int c = dn_wchunk(npix); return (npix + c - 1) / c; }
size_t dn_cinT(const DnLayer &l) { return l.ks == 7 ? 147 : (size_t)l.cin * l.taps(); }

// the padded virtual grid of a reflect-padded / up-sampled layer (the data gradient's lane grid before k_dnb_fold)
void dn_padded_grid(const DnLayer &l, int &gh, int &gw) { gh = (l.ih << l.up) + 2 * l.pad; gw = (l.iw << l.up) + 2 * l.pad; }

int dn_train_alloc(tcsfm_depthnet *dn) {
    if (dn->train.tbuf) return TCSFM_OK;
    tcsfm_ctx *h = dn->h;
    const size_t N = dn->max_images, hw = (size_t)h->H * h->W;
    size_t tot = 0, part = 0, bpart = 0, gv = 0;
    for (const DnLayer &l : dn->L) {
        tot += l.nw() + 5 * (size_t)l.cout + l.nw() + l.cout;
        const int npix = l.oh * l.ow;
        part = std::max(part, N * dn_nchunk(npix) * l.cout * dn_cinT(l));
        bpart = std::max(bpart, N * dn_nchunk(npix) * l.cout);
        if (l.reflect) { int gh, gw; dn_padded_grid(l, gh, gw); gv = std::max(gv, N * gh * gw * l.cin); }
    }
    tot += DN_HEAD_N;
    DnTrain &t = dn->train;
    hipError_t e = DEV_RESERVE(t.tbuf, tot);
    if (e == hipSuccess) e = DEV_RESERVE(t.part, part);
    if (e == hipSuccess) e = DEV_RESERVE(t.bpart, bpart);
    const int hch = (int)((hw + DNB_HEAD_CHUNK - 1) / DNB_HEAD_CHUNK);
    if (e == hipSuccess) e = DEV_RESERVE(t.hpart, N * hch * DN_HEAD_N);
    for (DevBuf<float> *p : {&t.gA, &t.gB, &t.gC}) if (e == hipSuccess) e = DEV_RESERVE(*p, N * hw * 32);    // the largest activation: H W x 32
    if (e == hipSuccess) e = DEV_RESERVE(t.gD, N * hw * 4);                      // a downsample's input grid
    if (e == hipSuccess) e = DEV_RESERVE(t.gV, gv);
    t.wt4.resize(dn->L.size());
    size_t o = 0;
    for (size_t li = 0; li < dn->L.size(); li++) {
        DnLayer &l = dn->L[li];
        l.raw = dn->train.tbuf + o; o += l.nw() + 5 * (size_t)l.cout;
        l.gw = dn->train.tbuf + o; o += l.nw();
        l.gb = dn->train.tbuf + o; o += l.cout;
        if (l.ks != 7 && e == hipSuccess) {
            const size_t n4 = (size_t)l.taps() * l.coutp * l.cin;      // floats / 4 ... in dn_f4 units: taps * coutp/16 * 4 * cin
            e = DEV_RESERVE(t.wt4[li], n4 / 4);
            l.wt4 = t.wt4[li];
            if (e == hipSuccess) e = hipMemsetAsync(l.wt4, 0, n4 * sizeof(float), h->stream);   // rows of channels >= cout stay zero
        }
        if (e == hipSuccess) e = hipMemsetAsync(dn->w->w4[li], 0, l.w4_count() * sizeof(dn_f4), h->stream);
    }
    dn->train.hacc = dn->train.tbuf + o;
    if (e != hipSuccess) {
        dn_train_free(dn);
        return fail_alloc(h, e, "tcsfm_depthnet_load_device: allocation failed");
    }
    return TCSFM_OK;
}

// data gradient of layer l from dz: direct (input grid, fused adds + derivative) or onto the padded virtual grid (then k_dnb_fold)
void dnb_dgrad(tcsfm_depthnet *dn, int li, int N, const float *dz, float *out, bool direct, const float *add1, const float *add2,
               const float *y, int act) {
    const DnLayer &l = dn->L[li];
    DnDgradParams P;
    P.dz = dz; P.wt4 = l.wt4; P.out = out; P.add1 = add1; P.add2 = add2; P.y = y; P.act = act;
    P.cin = l.cin; P.cout = l.cout; P.coutp = l.coutp; P.oh = l.oh; P.ow = l.ow; P.stride = l.stride; P.direct = direct ? 1 : 0;
    if (direct) { P.gh = l.ih; P.gw = l.iw; P.goff = l.pad; }
    else { dn_padded_grid(l, P.gh, P.gw); P.goff = 0; }
    dn_launch_split<DnDgradKernel>(l.ks, dn_split(P.gh * P.gw, l.cin / 16), P.gh * P.gw, l.cin / 16, N, P, dn->h->stream);
}

// (src + add) * act'(y) elementwise on an [N][h][w][C] map (C % 4 == 0)
void dnb_ew(tcsfm_depthnet *dn, int N, int C, int hh, int ww, const float *src, const float *add, const float *y, int act, float *out,
            float *raw_out = nullptr, int up = 0, int pad = 0, int reflect = 0) {
    DnFoldParams F;
    F.src = src; F.add = add; F.y = y; F.act = act; F.out = out; F.raw_out = raw_out; F.N = N;
    F.C = C; F.ih = hh; F.iw = ww; F.gh = (hh << up) + 2 * pad; F.gw = (ww << up) + 2 * pad; F.up = up; F.pad = pad; F.reflect = reflect;
    hipLaunchKernelGGL(k_dnb_fold, dim3(dn_blocks((long long)N * hh * ww * (C / 4))), dim3(256), 0, dn->h->stream, F);
}

// the same after folding layer li's padded virtual grid (src) back onto its input grid; raw_out: the folded sum before add / act'
void dnb_fold(tcsfm_depthnet *dn, int li, int N, const float *src, const float *add, const float *y, int act, float *out, float *raw_out) {
    const DnLayer &l = dn->L[li];
    dnb_ew(dn, N, l.cin, l.ih, l.iw, src, add, y, act, out, raw_out, l.up, l.pad, l.reflect);
}

// weight (wneed) and bias (bneed) gradients of the folded layer into l.gw / l.gb (accumulate: add to them)
void dnb_wgrad(tcsfm_depthnet *dn, int li, int N, const float *dz, const float *x, bool wneed, bool bneed, int accumulate) {
    DnLayer &l = dn->L[li];
    hipStream_t s = dn->h->stream;
    const int npix = l.oh * l.ow, chunk = dn_wchunk(npix), nch = dn_nchunk(npix), parts = N * nch;
    if (wneed) {
        DnWgradParams P;
        P.dz = dz; P.x = x; P.part = dn->train.part; P.cin = l.cin; P.cout = l.cout; P.ih = l.ih; P.iw = l.iw; P.oh = l.oh; P.ow = l.ow;
        P.stride = l.stride; P.pad = l.pad; P.up = l.up; P.reflect = l.reflect; P.chunk = chunk; P.nchunk = nch;
        if (l.ks == 7) hipLaunchKernelGGL((k_dnb_wgrad<7, 2, true>), dim3(parts, 2, l.coutp / 32), dim3(256), 0, s, P);
        else if (l.ks == 1) hipLaunchKernelGGL((k_dnb_wgrad<1, 2, false>), dim3(parts, l.cin / 16, l.coutp / 32), dim3(256), 0, s, P);
        else if (l.coutp % 32 == 0) hipLaunchKernelGGL((k_dnb_wgrad<9, 2, false>), dim3(parts, l.cin / 16, l.coutp / 32), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((k_dnb_wgrad<9, 1, false>), dim3(parts, l.cin / 16, l.coutp / 16), dim3(256), 0, s, P);
        const long long E = (long long)l.cout * dn_cinT(l);
        hipLaunchKernelGGL(k_dnb_wsum, dim3(dn_blocks(E)), dim3(256), 0, s, (const float *)dn->train.part, l.gw, E, parts, accumulate);
    }
    if (bneed) {
        hipLaunchKernelGGL(k_dnb_bgrad, dim3(parts), dim3(256), 0, s, dz, dn->train.bpart, l.cout, npix, chunk, nch);
        hipLaunchKernelGGL(k_dnb_wsum, dim3(dn_blocks(l.cout)), dim3(256), 0, s, (const float *)dn->train.bpart, l.gb, (long long)l.cout, parts, accumulate);
    }
}

// requested parameter gradients, by layer
struct DnReq {
    float *w = nullptr, *cb = nullptr, *g = nullptr, *be = nullptr;
    bool wneed() const { return w || g; }
    bool bneed() const { return cb || g || be; }
    bool any() const { return w || cb || g || be; }
};

// names -> per-layer requests (decoder: layers >= enc_end and the head; encoder: the others)
int dn_requests(tcsfm_depthnet *dn, const char *fn, bool dec, int n, const char *const names[], float *const grads[],
                std::vector<DnReq> &req, float **hw, float **hb, ArgRanges *ranges = nullptr) {
    tcsfm_ctx *h = dn->h;
    req.assign(dn->L.size(), DnReq());
    *hw = *hb = nullptr;
    if (n < 0 || (n > 0 && (!names || !grads))) return fail(h, TCSFM_E_ARG, (std::string(fn) + ": NULL argument").c_str());
    for (int i = 0; i < n; i++) {
        if (!names[i] || !grads[i]) return fail(h, TCSFM_E_ARG, (std::string(fn) + ": NULL name or gradient buffer").c_str());
        const std::string k = names[i];
        float **slot = nullptr;
        bool mine = false;
        size_t count = 0;
        for (size_t li = 0; li < dn->L.size() && !slot; li++) {
            DnLayer &l = dn->L[li];
            const bool d = (int)li >= dn->enc_end;
            if (k == l.wname) slot = &req[li].w;
            else if (!l.bname.empty() && k == l.bname) slot = &req[li].cb;
            else if (!l.bn.empty() && k == l.bn + ".weight") slot = &req[li].g;
            else if (!l.bn.empty() && k == l.bn + ".bias") slot = &req[li].be;
            else if (!l.bn.empty() && (k == l.bn + ".running_mean" || k == l.bn + ".running_var")) {
                h->err = std::string(fn) + ": " + k + ": running statistics have no gradient";
                return TCSFM_E_ARG;
            }
            if (slot) { mine = d == dec; count = slot == &req[li].w ? l.nw() : (size_t)l.cout; }
        }
        if (!slot && k == "predict_disps.0.0.conv.weight") { slot = hw; mine = dec; count = DN_HEAD_W; }
        if (!slot && k == "predict_disps.0.0.conv.bias") { slot = hb; mine = dec; count = 1; }
        if (!slot || !mine) {
            h->err = std::string(fn) + ": " + k + (slot ? ": not a parameter of this half of the network" : ": unknown parameter");
            return TCSFM_E_ARG;
        }
        *slot = grads[i];
        if (ranges) ranges->out("grads", grads[i], count * sizeof(float), i);
    }
    return TCSFM_OK;
}

// the five skip maps of N images as ranges of a call (include/tcsfm.h: skip k = [N, H >> (k+1), W >> (k+1), C_k]); a null table or entry is skipped
void dn_skip_ranges(const tcsfm_depthnet *dn, int N, const char *name, const float *const sk[5], bool out, ArgRanges &a) {
    for (int k = 0; sk && k < 5; k++)
        a.add(name, k, sk[k], (size_t)N * (dn->h->H >> (k + 1)) * (dn->h->W >> (k + 1)) * DN_SKIP_C[k] * sizeof(float), out);
}

// the chain rule through the fold and the reference layout, for every requested layer
void dn_param_out(tcsfm_depthnet *dn, const std::vector<DnReq> &req, int lo, int hi) {
    for (int li = lo; li < hi; li++) {
        const DnReq &r = req[li];
        if (!r.any()) continue;
        DnLayer &l = dn->L[li];
        const float *w = l.raw, *v = l.raw + l.nw();
        const bool bn = !l.bn.empty();
        hipLaunchKernelGGL(k_dnb_param_grad, dim3(dn_blocks(l.cout)), dim3(256), 0, dn->h->stream, (const float *)l.gw, (const float *)l.gb, w,
                           bn ? v + l.cout : nullptr, v + 3 * l.cout, v + 4 * l.cout, r.w, r.cb, r.g, r.be, l.cout, (int)l.nw() / l.cout);
    }
}

// decoder backward of one image group.  Positions: the decoder's layers in order (up(i), iconv(i), ..., feat()), then the head.
int dn_decode_backward(tcsfm_depthnet *dn, int N, const DnTape &t, int i0, const float *ddisp, float *const dsk[5],
                       const std::vector<DnReq> &req, bool head_req, int accumulate) {
    tcsfm_ctx *h = dn->h;
    const int E = dn->enc_end, F = dn->feat(), HEAD = F + 1, H = h->H, W = h->W;
    // lowest position whose data gradient is needed: below the lowest requested parameter, or where a requested skip's gradient leaves
    int low = HEAD + 1;
    for (int li = E; li <= F; li++) if (req[li].any()) { low = std::min(low, li); break; }
    if (head_req) low = std::min(low, HEAD);
    int skip_src = HEAD + 1;                    // the data gradient of layers >= skip_src must run
    if (dsk[4]) skip_src = E;
    for (int i = 0; dn_adds_skip(i) && skip_src > E; i++) if (dsk[3 - i]) skip_src = std::min(skip_src, dn->iconv(i));
    auto need_dgrad = [&](int pos) { return low < pos || skip_src <= pos; };
    auto at = [&](int e) { return t.at(e, i0); };
    float *f = at(DN_TD_FEAT), *disp = at(DN_TD_DISP);
    if (head_req) {
        const int hch = (H * W + DNB_HEAD_CHUNK - 1) / DNB_HEAD_CHUNK;
        hipLaunchKernelGGL(k_dnb_head_wgrad, dim3(N * hch), dim3(128), 0, h->stream, (const float *)f, (const float *)disp, ddisp, dn->train.hpart, H, W, hch);
        hipLaunchKernelGGL(k_dnb_wsum, dim3(1), dim3(256), 0, h->stream, (const float *)dn->train.hpart, dn->train.hacc, (long long)DN_HEAD_N, N * hch, accumulate);
    }
    if (!need_dgrad(HEAD)) return TCSFM_OK;
    float *cur = dn->train.gA, *nxt = dn->train.gB;
    hipLaunchKernelGGL(k_dnb_head, dim3(dn_blocks((long long)N * H * W)), dim3(256), 0, h->stream, (const float *)f, (const float *)disp, ddisp,
                       (const float *)dn->w->pw, cur, N, H, W);
    for (int li = F; li >= E && need_dgrad(li + 1); li--) {
        const int i = (li - E) / 2;
        const bool feat = li == F, up = !feat && li == dn->up(i);
        // the layer's input: the last iconv's output (features), the previous step's output or skip 4 (up-convolution), u (iconv)
        float *in = feat ? at(dn_td_x(DN_UPS - 1)) : up ? (i ? at(dn_td_x(i - 1)) : at(DN_TD_SKIP4)) : at(dn_td_u(i));
        if (req[li].any()) dnb_wgrad(dn, li, N, cur, in, req[li].wneed(), req[li].bneed(), accumulate);
        if (!need_dgrad(li)) break;
        dnb_dgrad(dn, li, N, cur, dn->train.gV, false, nullptr, nullptr, nullptr, DN_ACT_NONE);
        // through the ELU that made the input; an iconv's input is ELU (+ skip): the folded sum is that skip's gradient
        if (feat || (up && i > 0)) dnb_fold(dn, li, N, dn->train.gV, nullptr, in, DN_ACT_ELU, nxt, nullptr);
        else if (!up) dnb_fold(dn, li, N, dn->train.gV, nullptr, at(dn_td_elu(i)), DN_ACT_ELU, nxt, dn_adds_skip(i) ? dsk[3 - i] : nullptr);
        else dnb_fold(dn, li, N, dn->train.gV, nullptr, nullptr, DN_ACT_NONE, nullptr, dsk[4]);
        std::swap(cur, nxt);
    }
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

// encoder backward of one image group (dsk[k] NULL: no gradient on skip k)
int dn_encode_backward(tcsfm_depthnet *dn, int N, const DnTape &t, int i0, const float *const dsk[5], const std::vector<DnReq> &req, int accumulate) {
    tcsfm_ctx *h = dn->h;
    auto at = [&](int e) { return t.at(e, i0); };
    // is anything requested in blocks < j (or conv1)?
    int before[DN_BLOCKS + 1];
    before[0] = req[0].any();
    for (int j = 0; j < DN_BLOCKS; j++) {
        const DnBlock &B = dn->blk[j];
        before[j + 1] = before[j] || req[B.li].any() || req[B.li + 1].any() || (B.down && req[B.li + 2].any());
    }
    if (!before[DN_BLOCKS]) return TCSFM_OK;
    float *dz2 = dn->train.gA, *dz1 = dn->train.gB, *nx = dn->train.gC;
    const DnLayer &l4 = dn->L[dn->blk[DN_BLOCKS - 1].li + 1];
    dnb_ew(dn, N, l4.cout, l4.oh, l4.ow, dsk[4], nullptr, at(dn_te_out(DN_BLOCKS - 1)), DN_ACT_RELU, dz2);
    for (int j = DN_BLOCKS - 1; j >= 0; j--) {
        const DnBlock &B = dn->blk[j];
        // the block's input: the block before's output -- whose skip's gradient joins its own -- or the pooled map
        const float *hin = at(j ? dn_te_out(j - 1) : DN_TE_POOL), *t1 = at(dn_te_t1(j));
        const int skip_in = j ? dn->blk[j - 1].skip : -1;
        const int c1 = B.li, c2 = B.li + 1, ds = B.li + 2;
        if (req[c2].any()) dnb_wgrad(dn, c2, N, dz2, t1, req[c2].wneed(), req[c2].bneed(), accumulate);
        if (B.down && req[ds].any()) dnb_wgrad(dn, ds, N, dz2, hin, req[ds].wneed(), req[ds].bneed(), accumulate);
        if (!(req[c1].any() || before[j])) break;
        dnb_dgrad(dn, c2, N, dz2, dz1, true, nullptr, nullptr, t1, DN_ACT_RELU);
        if (req[c1].any()) dnb_wgrad(dn, c1, N, dz1, hin, req[c1].wneed(), req[c1].bneed(), accumulate);
        if (!before[j]) break;
        if (B.down) dnb_dgrad(dn, ds, N, dz2, dn->train.gD, true, nullptr, nullptr, nullptr, DN_ACT_NONE);
        dnb_dgrad(dn, c1, N, dz1, nx, true, B.down ? dn->train.gD : dz2, skip_in >= 0 ? dsk[skip_in] : nullptr, hin, j == 0 ? DN_ACT_NONE : DN_ACT_RELU);
        std::swap(dz2, nx);
    }
    if (req[0].any()) {
        // dz2 holds the pooled map's gradient: max-pool backward + skip 0 + ReLU, then conv1's weight gradient from the images
        const DnLayer &c1 = dn->L[0];
        hipLaunchKernelGGL(k_dnb_maxpool, dim3(dn_blocks((long long)N * c1.oh * c1.ow * 16)), dim3(256), 0, h->stream, (const float *)at(DN_TE_CONV1),
                           (const float *)dz2, dsk[0], nx, N, 64, c1.oh, c1.ow, c1.oh / 2, c1.ow / 2);
        dnb_wgrad(dn, 0, N, nx, at(DN_TE_IMAGES), req[0].wneed(), req[0].bneed(), accumulate);
    }
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}
}  // namespace

// ---- entry points (include/tcsfm.h) ---------------------------------------------------------------------------------------------
void tcsfm_depthnet_destroy(tcsfm_depthnet *dn) {
    if (!dn) return;
    DeviceGuard dev_guard(dn->h->device);
    // an attached network (tcsfm_sequence_depthnet) is detached: a sequence call synchronises its stage stream before it returns, so the
    // clone has no work in flight here
    if (dn->h->seq_dn == dn) dn->h->seq_dn = nullptr;
    delete dn;
}

int tcsfm_depthnet_create(tcsfm_handle h, int max_images, tcsfm_depthnet **out) {
    if (!h || !out) return TCSFM_E_ARG;
    *out = nullptr;
    if (max_images < 1 || max_images > 4096) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_create: max_images out of range");
    if (h->H % 32 || h->W % 32 || h->H < 32 || h->W < 32)
        return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_create: the handle's H and W must be multiples of 32 (the decoder's skip additions need them)");
    DeviceGuard dev_guard(h->device);
    tcsfm_depthnet *dn = new tcsfm_depthnet();
    dn->h = h; dn->max_images = max_images;
    dn_layers(dn);
    hipError_t e = hipSuccess;
    dn->own.w4.resize(dn->L.size()); dn->own.bias.resize(dn->L.size());
    for (size_t li = 0; li < dn->L.size(); li++) {
        if (e == hipSuccess) e = DEV_RESERVE(dn->own.w4[li], dn->L[li].w4_count());
        if (e == hipSuccess) e = DEV_RESERVE(dn->own.bias[li], dn->L[li].coutp);
    }
    if (e == hipSuccess) e = DEV_RESERVE(dn->own.pw, DN_HEAD_W);
    if (e == hipSuccess) e = DEV_RESERVE(dn->own.pb, 1);
    if (e == hipSuccess) e = dn_alloc_scratch(dn);
    if (e != hipSuccess) { tcsfm_depthnet_destroy(dn); return fail_alloc(h, e, "tcsfm_depthnet_create: allocation failed"); }
    *out = dn;
    return TCSFM_OK;
}

int tcsfm_depthnet_load(tcsfm_depthnet *dn, int n, const char *const names[], const float *const host_ptrs[], const int64_t *shapes) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    std::vector<DnSrc> src;
    const float *pw = nullptr, *pb = nullptr;
    if (int rc = dn_lookup(dn, "tcsfm_depthnet_load", n, names, host_ptrs, shapes, src, &pw, &pb)) return rc;
    DeviceGuard dev_guard(h->device);
    // fold + lay out every layer on the host (float64 fold, deterministic), then copy
    std::vector<std::vector<float>> w4s(dn->L.size()), biases(dn->L.size());
    for (size_t li = 0; li < dn->L.size(); li++) {
        const DnLayer &l = dn->L[li];
        const float *w = src[li].w, *cb = src[li].cb, *g = src[li].g, *be = src[li].be, *rm = src[li].rm, *rv = src[li].rv;
        std::vector<double> sc(l.cout, 1.0), sh(l.cout, 0.0);
        for (int co = 0; co < l.cout; co++) {
            if (g) { sc[co] = (double)g[co] / sqrt((double)rv[co] + 1e-5); sh[co] = (double)be[co] - (double)rm[co] * sc[co]; }
            if (cb) sh[co] += (double)cb[co] * sc[co];
        }
        auto W = [&](int co, int ci, int ky, int kx) { return (float)((double)w[(((size_t)co * l.cin + ci) * l.ks + ky) * l.ks + kx] * sc[co]); };
        std::vector<float> &o = w4s[li];
        if (l.ks == 7) {        // first layer: (g, kq) -> (ci, ky) = combo 2 g + (kq >> 1), kx = 4 (kq & 1) + t
            o.assign((size_t)11 * 4 * l.coutp * 4, 0.f);
            for (int gq = 0; gq < 44; gq++) {
                const int gg = gq >> 2, kq = gq & 3, combo = 2 * gg + (kq >> 1);
                if (combo >= 21) continue;
                const int ci = combo / 7, ky = combo % 7;
                for (int co = 0; co < l.cout; co++)
                    for (int t = 0; t < 4; t++) {
                        const int kx = 4 * (kq & 1) + t;
                        if (kx < 7) o[((size_t)(gg * 4 + kq) * l.coutp + co) * 4 + t] = W(co, ci, ky, kx);
                    }
            }
        } else {
            const int c16n = l.cin / 16;
            o.assign((size_t)l.ks * l.ks * c16n * 4 * l.coutp * 4, 0.f);
            for (int tap = 0; tap < l.ks * l.ks; tap++)
                for (int c16 = 0; c16 < c16n; c16++)
                    for (int kq = 0; kq < 4; kq++)
                        for (int co = 0; co < l.cout; co++)
                            for (int t = 0; t < 4; t++)
                                o[((size_t)((tap * c16n + c16) * 4 + kq) * l.coutp + co) * 4 + t] = W(co, c16 * 16 + 4 * kq + t, tap / l.ks, tap % l.ks);
        }
        biases[li].assign(l.coutp, 0.f);
        for (int co = 0; co < l.cout; co++) biases[li][co] = (float)sh[co];
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    HIPCHK(h, hipStreamSynchronize(h->stream));     // weights may be in use by earlier calls on the stream
    for (size_t li = 0; li < dn->L.size(); li++) {
        HIPCHK(h, hipMemcpy(dn->w->w4[li], w4s[li].data(), w4s[li].size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(dn->w->bias[li], biases[li].data(), biases[li].size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(dn->w->pw, pw, DN_HEAD_W * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(dn->w->pb, pb, sizeof(float), hipMemcpyHostToDevice));
    dn->loaded = 1;
    dn->train_loaded = 0;               // the training snapshot (tcsfm_depthnet_load_device) no longer matches the weights
    return TCSFM_OK;
}

int tcsfm_depthnet_encode(tcsfm_depthnet *dn, int N, const float *imgs, int flip, float *const skips_out[5]) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_check(dn, N, "tcsfm_depthnet_encode")) return rc;
    if (!imgs || !skips_out) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_encode: NULL argument");
    for (int k = 0; k < 5; k++) if (!skips_out[k]) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_encode: NULL skip buffer");
    {
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 3 * h->H * h->W * sizeof(float));
        dn_skip_ranges(dn, N, "skips_out", skips_out, true, a);
        if (int rc = check_overlap(h, "tcsfm_depthnet_encode", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    return dn_encode(dn, N, imgs, flip, dn_enc_scratch(dn, skips_out));
}

int tcsfm_depthnet_decode(tcsfm_depthnet *dn, int N, const float *const skips_in[5], float *disp_out) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_check(dn, N, "tcsfm_depthnet_decode")) return rc;
    if (!skips_in || !disp_out) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_decode: NULL argument");
    for (int k = 0; k < 5; k++) if (!skips_in[k]) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_decode: NULL skip buffer");
    {
        ArgRanges a;
        dn_skip_ranges(dn, N, "skips_in", skips_in, false, a);
        a.out("disp_out", disp_out, (size_t)N * h->H * h->W * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_depthnet_decode", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    return dn_decode(dn, N, skips_in, dn_dec_scratch(dn, disp_out));
}

int tcsfm_depthnet_forward(tcsfm_depthnet *dn, int N, const float *imgs, int flip, float *disp_out) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_check(dn, N, "tcsfm_depthnet_forward")) return rc;
    if (!imgs || !disp_out) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_forward: NULL argument");
    {
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 3 * h->H * h->W * sizeof(float));
        a.out("disp_out", disp_out, (size_t)N * h->H * h->W * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_depthnet_forward", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = dn_encode(dn, N, imgs, flip, dn_enc_scratch(dn, dn->skip))) return rc;
    return dn_decode(dn, N, dn->skip, dn_dec_scratch(dn, disp_out));
}

int tcsfm_sequence_depthnet(tcsfm_handle h, tcsfm_depthnet *dn) {
    if (!h) return TCSFM_E_ARG;
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!dn) { h->seq_dn = nullptr; return TCSFM_OK; }
    if (dn->h != h || !dn->loaded) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_depthnet: needs a loaded depth network of this handle (or NULL to detach)");
    DeviceGuard dev_guard(h->device);
    if (!dn_sequence_clone(dn)) return fail(h, TCSFM_E_NOMEM, "tcsfm_sequence_depthnet: no memory for the stage's activations");
    h->seq_dn = dn;
    return TCSFM_OK;
}

namespace {
// the two scaled-disparity planes of one group (tcsfm_depthnet::post_l / post_r), allocated on first use
int dn_post_scratch(tcsfm_depthnet *dn, const char *fn) {
    const size_t n = (size_t)dn->max_images * dn->h->H * dn->h->W;
    hipError_t e = DEV_RESERVE(dn->post_l, n);
    if (e == hipSuccess) e = DEV_RESERVE(dn->post_r, n);
    if (e != hipSuccess) return fail_alloc(dn->h, e, (std::string(fn) + ": no memory for the disparity planes").c_str());
    return TCSFM_OK;
}

// helpers.get_disp_for_eigen of ONE group of g <= max_images images on `dn`'s stream: the straight pass (its head stores the scaled
// disparity into post_l -- and, with `depth`, disp_to_depth's depth there: the sequence calls' depth stage), the pass on the mirrored
// images (scaled disparity into post_r, still mirrored), then k_disp_post into `out` [g,H,W] float64.  `ramp`: flip_ramp_device(h).
// The code path of tcsfm_depthnet_disp_for_eigen and of the sequence calls' TCSFM_SEQ_DISP_POST stage alike.
int dn_group_disp_for_eigen(tcsfm_depthnet *dn, int g, const float *imgs, float *depth, float min_disp, float max_disp, const double *ramp, double *out) {
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_encode(dn, g, imgs, 0, dn_enc_scratch(dn, dn->skip))) return rc;
    DnDecDst d = dn_dec_scratch(dn, depth ? depth : dn->post_l);
    d.min_disp = min_disp; d.max_disp = max_disp;
    if (depth) { d.as_depth = 1; d.scaled = dn->post_l; } else d.scaled_only = 1;
    if (int rc = dn_decode(dn, g, dn->skip, d)) return rc;
    if (int rc = dn_encode(dn, g, imgs, 1, dn_enc_scratch(dn, dn->skip))) return rc;
    DnDecDst m = dn_dec_scratch(dn, dn->post_r);
    m.min_disp = min_disp; m.max_disp = max_disp; m.scaled_only = 1;
    if (int rc = dn_decode(dn, g, dn->skip, m)) return rc;
    HIPCHK(h, launch_disp_post(dn_stream(dn), g, h->H, h->W, dn->post_l, dn->post_r, ramp, out));
    return TCSFM_OK;
}

// The depth stage of a sequence call (sequence_host.h: seq_stage_chunk): disp_to_depth(net(imgs), 1 / min_disp, 1 / max_disp)[1] of the n raw frames at
// `imgs` into the planes at `depth`, on `stream`, by the attached network's clone -- groups of max_images images, the same bits per
// image by the network's contract (its work split depends on H x W only).  The head writes the depth: with the disparity stage off
// (disp_mode = TCSFM_SEQ_DISP_OFF) no disparity plane exists.  TCSFM_SEQ_DISP_PLAIN: the same head launch also stores the scaled
// disparity into the float planes at `disp_store`.  TCSFM_SEQ_DISP_POST: get_disp_for_eigen of every frame into the float64 planes at
// `disp_store` (dn_group_disp_for_eigen: a second, mirrored pass and the blend per group; `ramp` and the clone's planes are the caller's
// to have ready).  The depths are the same bits in all three modes: one expression on one value.
int dn_sequence_depths(tcsfm_depthnet *dn, hipStream_t stream, int n, const float *imgs, float *depth, float min_disp, float max_disp,
                       int disp_mode = TCSFM_SEQ_DISP_OFF, void *disp_store = nullptr, const double *ramp = nullptr) {
    tcsfm_depthnet *q = dn->seq_clone.get();
    const size_t hw = (size_t)q->h->H * q->h->W;
    q->stream = stream;
    for (int i0 = 0; i0 < n; i0 += q->max_images) {
        const int g = std::min(n - i0, q->max_images);
        if (disp_mode == TCSFM_SEQ_DISP_POST) {
            if (int rc = dn_group_disp_for_eigen(q, g, imgs + (size_t)i0 * 3 * hw, depth + (size_t)i0 * hw, min_disp, max_disp, ramp,
                                                 (double *)disp_store + (size_t)i0 * hw)) return rc;
            continue;
        }
        if (int rc = dn_encode(q, g, imgs + (size_t)i0 * 3 * hw, 0, dn_enc_scratch(q, q->skip))) return rc;
        DnDecDst d = dn_dec_scratch(q, depth + (size_t)i0 * hw);
        d.as_depth = 1; d.min_disp = min_disp; d.max_disp = max_disp;
        if (disp_mode == TCSFM_SEQ_DISP_PLAIN) d.scaled = (float *)disp_store + (size_t)i0 * hw;
        if (int rc = dn_decode(q, g, q->skip, d)) return rc;
    }
    return TCSFM_OK;
}
}  // namespace

int tcsfm_depthnet_disp_for_eigen(tcsfm_depthnet *dn, const tcsfm_opts *o, int N, const void *imgs, void *out) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    const char *fn = "tcsfm_depthnet_disp_for_eigen";
    if (!dn->loaded) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_disp_for_eigen: no weights loaded");
    if (!o || !imgs || !out || N < 1) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_disp_for_eigen: bad argument");
    if (o->host_ptrs != 0) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_disp_for_eigen: host_ptrs must be 0 (device pointers); a host caller has the sequence calls (tcsfm_sequence_disparity)");
    if (!(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    if (((uintptr_t)imgs & 3) != 0 || ((uintptr_t)out & 7) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_disp_for_eigen: imgs must be aligned for float, out for double");
    const size_t hw = (size_t)h->H * h->W;
    {
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 3 * hw * sizeof(float));
        a.out("out", out, (size_t)N * hw * sizeof(double));
        if (int rc = check_overlap(h, fn, a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = dn_post_scratch(dn, fn)) return rc;
    const double *ramp = flip_ramp_device(h);
    if (!ramp) return TCSFM_E_HIP;
    for (int i0 = 0; i0 < N; i0 += dn->max_images)
        if (int rc = dn_group_disp_for_eigen(dn, std::min(N - i0, dn->max_images), (const float *)imgs + (size_t)i0 * 3 * hw, nullptr, 1.f / o->max_depth,
                                             1.f / o->min_depth, ramp, (double *)out + (size_t)i0 * hw)) return rc;
    return TCSFM_OK;
}

int tcsfm_debug_depthnet_split(tcsfm_depthnet *dn, int layer, int *ks, int *oh, int *ow, int *nb, int *pb, int *kw) {
    if (!dn) return TCSFM_E_ARG;
    if (layer < 0 || layer >= (int)dn->L.size()) return fail(dn->h, TCSFM_E_ARG, "tcsfm_debug_depthnet_split: layer out of range");
    const DnLayer &l = dn->L[layer];
    if (ks) *ks = l.ks;
    if (oh) *oh = l.oh;
    if (ow) *ow = l.ow;
    if (nb) *nb = l.sp.nb;
    if (pb) *pb = l.sp.pb;
    if (kw) *kw = l.sp.kw;
    return TCSFM_OK;
}

int tcsfm_depthnet_load_device(tcsfm_depthnet *dn, int n, const char *const names[], const float *const dev_ptrs[], const int64_t *shapes) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    std::vector<DnSrc> src;
    const float *pw = nullptr, *pb = nullptr;
    if (int rc = dn_lookup(dn, "tcsfm_depthnet_load_device", n, names, dev_ptrs, shapes, src, &pw, &pb)) return rc;
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = dn_train_alloc(dn)) return rc;
    hipStream_t s = h->stream;
    for (size_t li = 0; li < dn->L.size(); li++) {
        DnLayer &l = dn->L[li];
        const DnSrc &p = src[li];
        float *v = l.raw + l.nw();
        HIPCHK(h, hipMemcpyAsync(l.raw, p.w, l.nw() * sizeof(float), hipMemcpyDeviceToDevice, s));
        const float *vs[5] = {p.cb, p.g, p.be, p.rm, p.rv};
        for (int k = 0; k < 5; k++)
            if (vs[k]) HIPCHK(h, hipMemcpyAsync(v + (size_t)k * l.cout, vs[k], l.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        const bool bn = p.g != nullptr;
        hipLaunchKernelGGL(k_dnb_fold_params, dim3(dn_blocks((long long)l.nw())), dim3(256), 0, s, (const float *)l.raw, p.cb ? (const float *)v : nullptr,
                           bn ? (const float *)v + l.cout : nullptr, (const float *)v + 2 * l.cout, (const float *)v + 3 * l.cout,
                           (const float *)v + 4 * l.cout, dn->w->w4[li], l.wt4, dn->w->bias[li], l.cout, l.cin, l.ks, l.coutp);
    }
    HIPCHK(h, hipMemcpyAsync(dn->w->pw, pw, DN_HEAD_W * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(dn->w->pb, pb, sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipGetLastError());
    dn->loaded = 1;
    dn->train_loaded = 1;
    return TCSFM_OK;
}

int tcsfm_depthnet_tape_size(tcsfm_depthnet *dn, int N, int64_t *enc_floats, int64_t *dec_floats) {
    if (!dn) return TCSFM_E_ARG;
    if (N < 1 || !enc_floats || !dec_floats) return fail(dn->h, TCSFM_E_ARG, "tcsfm_depthnet_tape_size: bad argument");
    *enc_floats = (int64_t)dn_tape_layout(dn, 0, N, nullptr).total();
    *dec_floats = (int64_t)dn_tape_layout(dn, 1, N, nullptr).total();
    return TCSFM_OK;
}

int tcsfm_depthnet_encode_train(tcsfm_depthnet *dn, int N, const float *imgs, float *const skips_out[5], float *tape) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_check_train(dn, N, "tcsfm_depthnet_encode_train")) return rc;
    if (!imgs || !skips_out || !tape) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_encode_train: NULL argument");
    for (int k = 0; k < 5; k++) if (!skips_out[k]) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_encode_train: NULL skip buffer");
    {
        ArgRanges a;
        a.in("imgs", imgs, (size_t)N * 3 * h->H * h->W * sizeof(float));
        dn_skip_ranges(dn, N, "skips_out", skips_out, true, a);
        a.out("tape", tape, dn_tape_layout(dn, 0, N, nullptr).total() * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_depthnet_encode_train", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    return dn_for_groups(dn, 0, N, tape, skips_out, [&](int n, int i0, const DnTape &t, float *const sk[5]) -> int {
        const float *x = imgs + (size_t)i0 * t.sz[DN_TE_IMAGES];
        const DnEncDst d = dn_enc_tape(t, i0);
        if (int rc = dn_encode(dn, n, x, 0, d)) return rc;
        auto copy = [&](float *dst, const float *src, int e) { return hipMemcpyAsync(dst, src, (size_t)n * t.sz[e] * sizeof(float), hipMemcpyDeviceToDevice, h->stream); };
        HIPCHK(h, copy(t.at(DN_TE_IMAGES, i0), x, DN_TE_IMAGES));
        HIPCHK(h, copy(sk[0], d.conv1, DN_TE_CONV1));
        for (int j = 0; j < DN_BLOCKS; j++)
            if (dn->blk[j].skip >= 0) HIPCHK(h, copy(sk[dn->blk[j].skip], d.out[j], dn_te_out(j)));
        return TCSFM_OK;
    });
}

int tcsfm_depthnet_decode_train(tcsfm_depthnet *dn, int N, const float *const skips_in[5], float *disp_out, float *tape) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    if (int rc = dn_check_train(dn, N, "tcsfm_depthnet_decode_train")) return rc;
    if (!skips_in || !disp_out || !tape) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_decode_train: NULL argument");
    for (int k = 0; k < 5; k++) if (!skips_in[k]) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_decode_train: NULL skip buffer");
    {
        ArgRanges a;
        dn_skip_ranges(dn, N, "skips_in", skips_in, false, a);
        a.out("disp_out", disp_out, (size_t)N * h->H * h->W * sizeof(float));
        a.out("tape", tape, dn_tape_layout(dn, 1, N, nullptr).total() * sizeof(float));
        if (int rc = check_overlap(h, "tcsfm_depthnet_decode_train", a)) return rc;
    }
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    return dn_for_groups(dn, 1, N, tape, skips_in, [&](int n, int i0, const DnTape &t, const float *const sk[5]) -> int {
        const DnDecDst d = dn_dec_tape(t, i0);
        if (int rc = dn_decode(dn, n, sk, d)) return rc;
        HIPCHK(h, hipMemcpyAsync(t.at(DN_TD_SKIP4, i0), sk[4], (size_t)n * t.sz[DN_TD_SKIP4] * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(disp_out + (size_t)i0 * t.sz[DN_TD_DISP], d.disp, (size_t)n * t.sz[DN_TD_DISP] * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        return TCSFM_OK;
    });
}

int tcsfm_depthnet_decode_backward(tcsfm_depthnet *dn, int N, const float *tape, const float *d_disp, float *const d_skips[5], int n_grads,
                                   const char *const names[], float *const grads[]) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    const char *fn = "tcsfm_depthnet_decode_backward";
    if (int rc = dn_check_train(dn, N, fn)) return rc;
    if (!tape || !d_disp) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_decode_backward: NULL argument");
    std::vector<DnReq> req;
    float *hw_ = nullptr, *hb_ = nullptr;
    ArgRanges a;
    a.in("tape", tape, dn_tape_layout(dn, 1, N, nullptr).total() * sizeof(float));
    a.in("d_disp", d_disp, (size_t)N * h->H * h->W * sizeof(float));
    dn_skip_ranges(dn, N, "d_skips", d_skips, true, a);
    if (int rc = dn_requests(dn, fn, true, n_grads, names, grads, req, &hw_, &hb_, &a)) return rc;
    if (int rc = check_overlap(h, fn, a)) return rc;
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = dn_for_groups(dn, 1, N, tape, d_skips, [&](int n, int i0, const DnTape &t, float *const dsk[5]) {
            return dn_decode_backward(dn, n, t, i0, d_disp + (size_t)i0 * t.sz[DN_TD_DISP], dsk, req, hw_ || hb_, i0 > 0);
        })) return rc;
    dn_param_out(dn, req, dn->enc_end, (int)dn->L.size());
    if (hw_) HIPCHK(h, hipMemcpyAsync(hw_, dn->train.hacc, DN_HEAD_W * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (hb_) HIPCHK(h, hipMemcpyAsync(hb_, dn->train.hacc + DN_HEAD_W, sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}

int tcsfm_depthnet_encode_backward(tcsfm_depthnet *dn, int N, const float *tape, const float *const d_skips[5], int n_grads,
                                   const char *const names[], float *const grads[]) {
    if (!dn) return TCSFM_E_ARG;
    tcsfm_ctx *h = dn->h;
    const char *fn = "tcsfm_depthnet_encode_backward";
    if (int rc = dn_check_train(dn, N, fn)) return rc;
    if (!tape) return fail(h, TCSFM_E_ARG, "tcsfm_depthnet_encode_backward: NULL argument");
    std::vector<DnReq> req;
    float *hw_ = nullptr, *hb_ = nullptr;
    ArgRanges a;
    a.in("tape", tape, dn_tape_layout(dn, 0, N, nullptr).total() * sizeof(float));
    dn_skip_ranges(dn, N, "d_skips", d_skips, false, a);
    if (int rc = dn_requests(dn, fn, false, n_grads, names, grads, req, &hw_, &hb_, &a)) return rc;
    if (int rc = check_overlap(h, fn, a)) return rc;
    if (int rc_q = drain_queued(h)) return rc_q;
    DeviceGuard dev_guard(h->device);
    if (int rc = dn_for_groups(dn, 0, N, tape, d_skips, [&](int n, int i0, const DnTape &t, const float *const dsk[5]) {
            return dn_encode_backward(dn, n, t, i0, dsk, req, i0 > 0);
        })) return rc;
    dn_param_out(dn, req, 0, dn->enc_end);
    HIPCHK(h, hipGetLastError());
    return TCSFM_OK;
}
