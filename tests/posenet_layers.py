"""Float64 references, rounding bounds, parameter sets and the case table of the layer-by-layer PoseNet tests
(tests/test_posenet_layers_cpu.py, tests/test_gpu_posenet_layers.py).

CHAINED reference: standins.PoseNetTwin(...).double() stepped layer by layer -- all seven raw convolution outputs, the GroupNorm
(scale, shift) pairs  scale = rstd gamma, shift = beta - mean scale  the consumer applies, and the pose.

ISOLATED reference of layer l: the layer alone, in float64, on the operand the library itself consumed -- relu(raw * scale + shift)
of the library's OWN fp32 raw[l-1] and scsh[l-1] (layer 1: (img - 0.45f) / 0.22 of the images; 0.45f is the fp32 constant the
reference's own fp32 program subtracts, so that a frame of 0.45f is a frame of zeros, as it is for the reference).  No error is
inherited from the layers before, so a fault shows in the layer that has it.

BOUND, per output:  (K + 8) 2^-24 (|a| conv |w| + |bias|),  K = cin k k.  A K-term fp32 dot product summed in ANY order is within
K u sum |a_i w_i| of the exact one (u = 2^-24; Higham, Accuracy and Stability of Numerical Algorithms, 3.1) -- the K split, the
permuted K order of the matrix-core layout and the bias add are all inside it.  The 8 u cover the operands: the weights standardised
in fp32 (mean, subtraction, reciprocal deviation, product: 4 roundings) and the fp32 normalise + ReLU of the activation (multiply,
add: 2, with slack for a fused multiply-add).  Where  raw scale + shift  cancels, the activation's rounding is relative to |raw scale|
+ |shift| rather than to |a|; with K >= 288 behind the sum and the parameter sets below (|raw scale| + |shift| <= ~25 where E|a| ~
0.4) that stays under a third of the bound even if every term erred the same way.  Derived, not measured: torch's own fp32
convolution uses 0.02 of it (test_posenet_layers_cpu.py), one zeroed tap leaves it.

SCALE / SHIFT tolerance (scsh_tolerance): the convolutions' epilogues sum a channel's values and squares over a workgroup's n pixels in
fp32 (n = 128 in layer 1, 64 PB elsewhere), k_pn_stats adds those partial sums in double and forms  var = E[x^2] - mean^2  in double;
K-split layers sum the values themselves in double (n = 0).  A fp32 sum of n terms: |dS1| <= n u sum |x|, |dS2| <= (n + 1) u sum x^2
(one more rounding for each square).  Hence  dmean <= n u E|x|,  dvar <= (n + 1) u E[x^2] + 2 |mean| dmean <= 3 (n + 1) u (var + mean^2),
drstd / rstd <= dvar / (2 (var + eps)),  and with the fp32 roundings of rstd, its product with gamma, the mean, its product and the
subtraction (4 u each way):
    |dscale| <= |scale| (dvar / (2 (var + eps)) + 4 u),    |dshift| <= |scale| dmean + |mean| |dscale| + 4 u (|beta| + |mean scale|).
The double-precision sums contribute 2^-40 relative (a million terms at 2^-53 with room), added to both.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import standins

CHANS = [6, 16, 32, 64, 128, 256, 256, 256]
KSZ = [7, 5, 3, 3, 3, 3, 3]
U = 2.0 ** -24
EPS = 1e-5
MARGIN = 4.0                    # the operator tests' rule: error <= max(floor, MARGIN * the fp32 CPU twin's error)
FLOOR_REL_L2 = 8 * U            # below a few ulps of the format the ratio of two fp32 errors says nothing
FLOOR_MAX_RMS = 64 * U          # the same for the largest error over the RMS (a maximum over 1e4..1e6 values sits ~8 x above the L2 figure)
FLOOR_POSE = 8 * U


# ---- work-split selection: the rule of tcsfm_posenet_create / pn_run, restated (the GPU tests assert the library's own read-out) ----
def selection_table(H, W):
    """per layer 1..7: dict(oh, ow, few=(nb, ks, pb), many=(nb, ks, pb))"""
    ih, iw, out = H, W, []
    for l in range(7):
        cin, cout, k = CHANS[l], CHANS[l + 1], KSZ[l]
        pad = (k - 1) // 2
        oh, ow = (ih + 2 * pad - k) // 2 + 1, (iw + 2 * pad - k) // 2 + 1
        kg = 21 if l == 0 else k * k * cin // 16
        pxb, cb = (oh * ow + 15) // 16, cout // 16
        nb, ks = min(cb, 4), 1
        while nb > 1 and pxb * (cb // nb) * 2 < 768:
            nb //= 2
        while ks < 16 and pxb * (cb // nb) * 2 * ks < 768 and kg // (2 * ks) >= 8:
            ks *= 2
        few = (1, 1, 1) if l == 0 else (nb, ks, 1)
        nb1 = 4 if cout >= 64 else cb
        ks1 = min(16, (kg + 23) // 24) if oh * ow <= 512 else 1
        pb = 2 if (l > 0 and nb1 >= 2 and oh * ow >= 64) else 1
        out.append(dict(oh=oh, ow=ow, few=few, many=(nb1, ks1, pb)))
        ih, iw = oh, ow
    return out


# (layer, nb, ks, pb) that no test launched before these: the sizes of tests/test_gpu_posenet.py reach none of them
NEEDED_FEW = {(2, 1, 1, 1), (3, 2, 1, 1), (3, 4, 1, 1), (4, 1, 1, 1), (4, 2, 1, 1), (5, 1, 1, 1), (5, 1, 2, 1), (6, 1, 4, 1), (6, 1, 8, 1)}
NEEDED_MANY = {(2, 2, 2, 1), (3, 4, 1, 1), (4, 4, 1, 2), (6, 4, 6, 2)}

# (H, W, N, max_images, the (layer, nb, ks, pb) the case is there for).  Every size once with N <= 4 and once with N > 4.
CASES = [
    (5, 9, 1, 1, ((2, 1, 2, 1), (7, 1, 16, 1))),                      # one pixel from layer 4 on
    (5, 9, 7, 7, ((2, 2, 2, 1), (3, 4, 1, 1))),
    (17, 33, 2, 2, ((3, 1, 2, 1), (4, 1, 4, 1))),
    (17, 33, 5, 5, ((2, 2, 2, 1), (3, 4, 1, 1))),
    (37, 53, 4, 4, ((5, 1, 8, 1), (6, 1, 16, 1))),
    (37, 53, 7, 12, ((3, 4, 1, 1), (2, 2, 2, 2))),                    # max_images above N
    (64, 64, 1, 1, ((2, 1, 2, 1), (3, 1, 2, 1))),
    (64, 64, 5, 5, ((3, 4, 1, 2), (4, 4, 2, 1))),                     # layer 3: exactly 64 pixels, the smallest with two pixel blocks
    (100, 333, 2, 3, ((1, 1, 1, 1), (2, 1, 2, 1))),                   # OW = 167: ragged conv1 chunk; max_images above N
    (100, 333, 5, 5, ((2, 2, 1, 2), (4, 4, 2, 2))),
    (128, 416, 4, 4, ((2, 1, 1, 1), (4, 1, 4, 1))),
    (128, 416, 5, 5, ((4, 4, 2, 2), (5, 4, 3, 1))),
    (192, 640, 2, 2, ((2, 2, 1, 1), (3, 1, 1, 1))),
    (192, 640, 7, 7, ((3, 4, 1, 2), (5, 4, 3, 2))),
    (240, 320, 1, 1, ((2, 1, 1, 1), (5, 1, 8, 1))),
    (240, 320, 5, 5, ((4, 4, 2, 2), (6, 4, 6, 1))),
    (256, 448, 2, 2, ((3, 1, 1, 1), (5, 1, 4, 1))),
    (256, 448, 5, 8, ((5, 4, 3, 2), (7, 4, 6, 1))),
    (320, 1024, 2, 2, ((3, 2, 1, 1), (4, 1, 1, 1), (5, 1, 2, 1), (6, 1, 8, 1))),
    (320, 1024, 5, 5, ((4, 4, 1, 2), (6, 4, 6, 2))),
    (375, 1242, 1, 1, ((3, 4, 1, 1), (4, 2, 1, 1), (5, 1, 1, 1), (6, 1, 4, 1))),   # raw KITTI: odd extents, ten conv1 chunks, the last ragged
    (375, 1242, 5, 5, ((4, 4, 1, 2), (6, 4, 6, 2))),
    (33, 2050, 2, 2, ((2, 1, 1, 1), (6, 1, 8, 1))),                   # 17 conv1 chunks, OH = 17: one output row pair past the end
    (33, 2050, 5, 5, ((2, 2, 1, 2), (4, 4, 2, 2))),
]
CASE_IDS = [f"{H}x{W}-N{N}of{M}" for H, W, N, M, _ in CASES]
SIZES = sorted({(H, W) for H, W, *_ in CASES})


# ---- parameter sets (standins.posenet_params' random stream is the golden fixture's: untouched) ---------------------------------
def ws64(w):
    """conv2d_wn's standardisation (pose_models.py:17-23) in float64"""
    w = torch.as_tensor(w).double()
    w = w - w.mean(dim=(1, 2, 3), keepdim=True)
    return w / (w.flatten(1).std(dim=1).view(-1, 1, 1, 1) + 1e-5)


@functools.lru_cache(maxsize=None)
def _layer_rms(seed):
    """RMS of every layer's raw output under posenet_params(seed), from the float64 twin on one 64 x 96 batch"""
    x = torch.tensor(np.random.default_rng(11).uniform(0, 1, size=(2, 6, 64, 96)))
    return tuple(float(r.pow(2).mean().sqrt()) for r in chained64(standins.posenet_params(seed), x)["raw"])


def posenet_params_offset(seed=0):
    """posenet_params(seed) with convolution biases that put every GroupNorm group's mean at 3 to 10 of the layer's output RMS (one
    value per group, either sign): var = E[x^2] - mean^2 then cancels 10 to 100 times its own size.  GroupNorm removes a group-wide
    offset, so the layers downstream see the activations of the base set."""
    sd = {k: np.array(v) for k, v in standins.posenet_params(seed).items()}
    rng = np.random.default_rng(9100 + seed)
    for i, rms in enumerate(_layer_rms(seed)):
        cout = CHANS[i + 1]
        off = rng.uniform(3.0, 10.0, size=16) * rng.choice([-1.0, 1.0], size=16) * rms
        sd[f"conv{i + 1}.0.bias"] = (sd[f"conv{i + 1}.0.bias"] + np.repeat(off, cout // 16)).astype(np.float32)
    return sd


def posenet_params_gamma(seed=0):
    """posenet_params(seed) with GroupNorm gamma near zero on every fourth channel and negative on every fourth"""
    sd = {k: np.array(v) for k, v in standins.posenet_params(seed).items()}
    rng = np.random.default_rng(9200 + seed)
    for i in range(7):
        g = sd[f"conv{i + 1}.1.weight"].astype(np.float64)
        c = np.arange(g.size)
        g[c % 4 == 1] = 1e-3 * rng.normal(size=int((c % 4 == 1).sum()))
        g[c % 4 == 2] *= -1.0
        sd[f"conv{i + 1}.1.weight"] = g.astype(np.float32)
    return sd


PARAM_SETS = {"base": standins.posenet_params, "offset": posenet_params_offset, "gamma": posenet_params_gamma}


def images(H, W, N, seed):
    """[N,6,H,W] fp32 in [0,1]: a smooth ramp per item and channel plus noise -- no two items, channels or pixels alike"""
    rng = np.random.default_rng(1000 * seed + H * W + N)
    yy, xx = np.mgrid[0:H, 0:W]
    ph = rng.uniform(0, 2 * np.pi, size=(N, 6, 1, 1))
    fx, fy = rng.uniform(0.5, 3.0, size=(2, N, 6, 1, 1))
    x = 0.5 + 0.25 * np.sin(ph + fx * xx / max(W, 8) * 6.0 + fy * yy / max(H, 8) * 6.0) + rng.uniform(-0.25, 0.25, size=(N, 6, H, W))
    return torch.tensor(np.clip(x, 0.0, 1.0).astype(np.float32))


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def gn_scsh64(raw, gamma, beta):
    """GroupNorm(16) of raw [N,C,h,w] (float64) as (scale, shift) [N,C,2] + the per-group (mean, var) [N,16]"""
    N, Cn = raw.shape[:2]
    g = raw.reshape(N, 16, -1)
    mean, var = g.mean(2), g.var(2, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    cg = Cn // 16
    sc = rstd.repeat_interleave(cg, 1) * torch.as_tensor(gamma).double()
    sh = torch.as_tensor(beta).double() - mean.repeat_interleave(cg, 1) * sc
    return torch.stack([sc, sh], 2), mean, var


def operand64(l, imgs=None, raw=None, scsh=None):
    """the float64 operand of layer l (1..7): the normalised images, or relu(raw * scale + shift) of layer l - 1's outputs"""
    if l == 1:
        return (imgs.double() - float(np.float32(0.45))) / 0.22
    sc, sh = scsh.double()[:, :, 0, None, None], scsh.double()[:, :, 1, None, None]
    return torch.relu(raw.double() * sc + sh)


def isolated64(sd, l, a64, w64=None):
    """layer l alone on operand a64 -> (raw output, rounding bound), both float64 [N,cout,oh,ow]"""
    w = ws64(sd[f"conv{l}.0.weight"]) if w64 is None else w64
    b = torch.as_tensor(sd[f"conv{l}.0.bias"]).double()
    k = w.shape[-1]
    y = F.conv2d(a64, w, b, 2, (k - 1) // 2)
    mag = F.conv2d(a64.abs(), w.abs(), None, 2, (k - 1) // 2) + b.abs().view(1, -1, 1, 1)
    return y, (w[0].numel() + 8) * U * mag


def chained(sd, imgs, dtype=torch.float64):
    """standins.PoseNetTwin in `dtype`, layer by layer: dict(raw[7], act[7], scsh[7] (float64 GroupNorm of that raw), pose)"""
    net = standins.PoseNetTwin(sd).to(dtype).eval()
    out = dict(raw=[], act=[], scsh=[])
    with torch.no_grad():
        x = (imgs.to(dtype) - 0.45) / 0.22 if dtype != torch.float64 else operand64(1, imgs)
        for i in range(7):
            seq = getattr(net, f"conv{i + 1}")
            raw = seq[0](x)
            x = seq[2](seq[1](raw))
            out["raw"].append(raw); out["act"].append(x)
            out["scsh"].append(gn_scsh64(raw.double(), sd[f"conv{i + 1}.1.weight"], sd[f"conv{i + 1}.1.bias"])[0])
        out["pose"] = 0.01 * net.pose_pred(x).mean(3).mean(2).view(-1, 6)
    return out


def chained64(sd, imgs):
    return chained(sd, imgs, torch.float64)


def scsh_tolerance(raw, gamma, beta, n):
    """(reference scale/shift [N,C,2], tolerance [N,C,2]) of a fp32 raw output whose statistics were summed in fp32 over n values
    at a time and in double beyond (module docstring); n = 0: summed in double throughout"""
    raw = raw.double()
    ref, mean, var = gn_scsh64(raw, gamma, beta)
    N, Cn = raw.shape[:2]
    cg = Cn // 16
    g = raw.reshape(N, 16, -1)
    e1, e2 = g.abs().mean(2), g.pow(2).mean(2)
    dbl = 2.0 ** -40
    dmean = (n * U + dbl) * e1
    dvar = (n + 1 if n else 0) * U * e2 + 2 * mean.abs() * dmean + dbl * e2
    rel = dvar / (2 * (var + EPS)) + 4 * U
    rep = lambda t: t.repeat_interleave(cg, 1)
    sc = ref[:, :, 0].abs()
    dsc = sc * rep(rel)
    dsh = sc * rep(dmean) + rep(mean.abs()) * dsc + 4 * U * (torch.as_tensor(beta).double().abs() + rep(mean.abs()) * sc)
    return ref, torch.stack([dsc, dsh], 2)


def stats_group_size(layer, nb, ks, pb):
    """how many values of a channel the convolution's epilogue sums in fp32 before k_pn_stats takes over in double"""
    if ks > 1:
        return 0
    return 128 if layer == 1 else 64 * pb


def rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).pow(2).sum().sqrt() / ref.pow(2).sum().sqrt().clamp_min(1e-300))


def max_over_rms(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-300))


def hold(floor, e32):
    return max(floor, MARGIN * e32)
