"""Float64 references, rounding bounds, parameter sets and the case table of the layer-by-layer tests of the depth network's forward
(tests/test_depthnet_layers_cpu.py, tests/test_gpu_depthnet_layers.py).  The statistical rule (U, MARGIN, the floors, rel_l2,
max_over_rms, hold) is tests/posenet_layers.py's.

LAUNCHES: the forward is 33 launches -- conv1, the max pool, 16 BasicBlock convolutions and 3 1x1 downsamples, 5 up-convolutions,
5 iconvs, feature_convs.0 and the sigmoid head.  The training forward (tcsfm_depthnet_encode_train / _decode_train) runs the same
kernels and leaves every launch's input and output in its tapes (depthnet_host.h dn_tape_layout), except a downsample's output, which
only the block's second convolution reads.  checks() pairs every launch with the tape entries it read and wrote.

ISOLATED reference of a launch: the layer alone, in float64, on the library's OWN fp32 tape entry, with BatchNorm folded in float64
(w' = w gamma / sqrt(var + 1e-5), b' = beta - mean gamma / sqrt(var + 1e-5); decoder: the convolution's own bias).  No error is
inherited, so a fault shows in the launch that has it.  A down block's output is checked as  relu(conv2(t1) + downsample(x))  from the
two entries it reads.  conv1's operand is (img - 0.45f) / 0.22 (posenet_layers.operand64).

BOUND, per output element:  g(K + c) (|a| conv |w'| + |b'| + |residual or skip|),  g(n) = n u / (1 - n u), u = 2^-24, K = cin ks ks.
A K-term fp32 dot product summed in ANY order is within g(K) sum |a_i w_i| of the exact one (Higham, Accuracy and Stability of
Numerical Algorithms, 3.1): the matrix-core K order, the K split over four waves and its LDS reduction are inside it.  c counts the
other roundings, each relative to a quantity no larger than the bracket:
    3   every convolution: fp32 rounding of the folded weight, of the folded bias, and the bias add
  + 1   residual add (BasicBlock conv2) or skip add (up-convolutions 0..3)
  + 3   conv1: the subtraction, the division, and 0.22f for 0.22
  + 4   ELU: expm1f (a few ulps; |expm1(v)| <= |v|)
ReLU and ELU are 1-Lipschitz, so the bound of the pre-activation holds on the taped output.  A down block adds the downsample's own
bound twice: once as the error of the residual the library added, once (times g) as that residual's magnitude.  The head's pre-sigmoid
sum has K = 72 and one bias add; sigmoid' <= 1/4, and expf, 1 + e and the reciprocal are relative to the output:
bound = g(K + 1) (|a| conv |w| + |b|) / 4 + 6 u sigmoid.  The max pool is exact: bit for bit against F.max_pool2d.
Derived, not measured; what torch's own fp32 convolution uses of it is recorded in tests/test_depthnet_layers_cpu.py.

STATISTICAL criterion, per launch: relative L2 and max error / RMS of HIP against the isolated float64 <= hold(floor, e32), e32 the same
figure for torch's fp32 CPU convolution of the same fp32 operand with the fp32-rounded folded parameters.  This is what
sees one wrong term that a worst-case K-term bound lets through.

CHAINED reference: depthnet_twin.forward in float64 end to end, subtracting 0.45f as the library does (twin_tapes); disparity and skips under the same rule against the fp32 CPU twin.
Skip elements whose ReLU decided differently (one side zero, the other positive) are left out of that comparison only, at most
operator_inputs.decision_cap of a tensor."""
import functools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import depthnet_twin as dt
from operator_inputs import decision_cap                                                          # noqa: F401  (re-exported)
from posenet_layers import FLOOR_MAX_RMS, FLOOR_REL_L2, MARGIN, U, hold, max_over_rms, rel_l2     # noqa: F401  (re-exported)

ENC = dt.ENC
PLANES = dt.PLANES
SKIP_ENTRY = (1, 6, 10, 14, 18)            # encoder tape entries of skips 0..4
C_CONV, C_ADD, C_CONV1, C_ELU = 3, 1, 3, 4
FLOOR_DISP = 8 * U


def gamma_n(n):
    return n * U / (1.0 - n * U)


# ---- the convolutions in the library's order (dn_layers) and the work split rule (dn_split), restated --------------------------------
def layers(H, W):
    """the 31 convolutions of depthnet_host.h dn_layers, in its order: dicts(name, kind, cin, cout, ks, stride, up, reflect, ih, iw, oh,
    ow, w, b (conv bias key or None), bn (BatchNorm prefix or None))"""
    out = []

    def add(name, kind, cin, cout, ks, stride, ih, iw, up, reflect, w, b, bn):
        pad = (ks - 1) // 2
        oh, ow = ((ih << up) + 2 * pad - ks) // stride + 1, ((iw << up) + 2 * pad - ks) // stride + 1
        out.append(dict(name=name, kind=kind, cin=cin, cout=cout, ks=ks, stride=stride, up=up, reflect=reflect, ih=ih, iw=iw, oh=oh,
                        ow=ow, w=w, b=b, bn=bn))
        return oh, ow
    add("conv1", "conv1", 3, 64, 7, 2, H, W, 0, 0, f"{ENC}conv1.weight", None, f"{ENC}bn1")
    h, w = H // 4, W // 4
    for p, ci, co, s, ds in dt._blocks():
        short = p[len(ENC):]
        oh, ow = add(short + "conv1", "stride2" if s == 2 else "plain", ci, co, 3, s, h, w, 0, 0, p + "conv1.weight", None, p + "bn1")
        add(short + "conv2", "residual", co, co, 3, 1, oh, ow, 0, 0, p + "conv2.weight", None, p + "bn2")
        if ds:
            add(short + "downsample", "down1x1", ci, co, 1, 2, h, w, 0, 0, p + "downsample.0.weight", None, p + "downsample.1")
        h, w = oh, ow
    for i in range(5):
        u, ic = f"depth_upconvs.{i}.1.conv.", f"iconvs.{i}.0.conv."
        add(f"depth_upconvs.{i}", "up+skip" if i < 4 else "up", PLANES[i], PLANES[i + 1], 3, 1, h, w, 1, 1, u + "weight", u + "bias", None)
        h, w = 2 * h, 2 * w
        add(f"iconvs.{i}", "reflect", PLANES[i + 1], PLANES[i + 1], 3, 1, h, w, 0, 1, ic + "weight", ic + "bias", None)
    add("feature_convs.0", "cout8", 32, 8, 3, 1, h, w, 0, 1, "feature_convs.0.0.conv.weight", "feature_convs.0.0.conv.bias", None)
    return out


def split(npix, cout):
    """dn_split: (nb, pb, kw) of a layer of npix output pixels per image"""
    cb = (cout + 15) // 16
    if npix >= 4096:
        return min(4, cb), 2, 1
    if npix >= 1024:
        return min(2, cb), 1, 4
    return 1, 1, 4


def selection_table(H, W):
    """per convolution, in the library's order: (ks, nb, pb, kw, npix, partial_workgroup, partial_wave).  A workgroup covers
    16 pb (4 / kw) pixels, a wave 16 pb; conv1 runs k_dn_conv1<2> (128 and 32) whatever its nb / pb / kw say"""
    out = []
    for i, L in enumerate(layers(H, W)):
        npix = L["oh"] * L["ow"]
        nb, pb, kw = split(npix, L["cout"])
        wave = 32 if i == 0 else 16 * pb
        wg = 128 if i == 0 else wave * (4 // kw)
        out.append((L["ks"], nb, pb, kw, npix, npix % wg != 0, npix % wave != 0))
    return out


def reached(H, W):
    """{(kind, ks, nb, pb, kw)} of the k_dn_conv launches at H x W, and {(kw, 'workgroup' | 'wave')} of those that run partly filled"""
    inst, part = set(), set()
    for L, (ks, nb, pb, kw, npix, pwg, pwave) in list(zip(layers(H, W), selection_table(H, W)))[1:]:
        inst.add((L["kind"], ks, nb, pb, kw))
        if pwg:
            part.add((kw, "workgroup"))
        if pwave:
            part.add((kw, "wave"))
    return inst, part


INSTANCES = {(3, 4, 2, 1), (3, 2, 2, 1), (3, 1, 2, 1), (3, 2, 1, 4), (3, 1, 1, 4), (1, 4, 2, 1), (1, 2, 1, 4), (1, 1, 1, 4)}
# every (layer kind, KS, NB, PB, KW) any H, W <= 352 x 1216 reaches (test_depthnet_layers_cpu.py enumerates them), and the partly
# filled workgroups / waves per KW
NEEDED = {
    ("plain", 3, 4, 2, 1), ("plain", 3, 2, 1, 4), ("plain", 3, 1, 1, 4),
    ("residual", 3, 4, 2, 1), ("residual", 3, 2, 1, 4), ("residual", 3, 1, 1, 4),
    ("stride2", 3, 4, 2, 1), ("stride2", 3, 2, 1, 4), ("stride2", 3, 1, 1, 4),
    ("down1x1", 1, 4, 2, 1), ("down1x1", 1, 2, 1, 4), ("down1x1", 1, 1, 1, 4),
    ("up+skip", 3, 4, 2, 1), ("up+skip", 3, 2, 1, 4), ("up+skip", 3, 1, 1, 4),
    ("up", 3, 2, 2, 1), ("up", 3, 2, 1, 4),
    ("reflect", 3, 4, 2, 1), ("reflect", 3, 2, 2, 1), ("reflect", 3, 2, 1, 4), ("reflect", 3, 1, 1, 4),
    ("cout8", 3, 1, 2, 1), ("cout8", 3, 1, 1, 4),
}
NEEDED_PARTIAL = {(1, "workgroup"), (1, "wave"), (4, "workgroup"), (4, "wave")}

# (H, W, N, max_images, parameter set, inputs).  N = 3 over max_images = 2: image groups 2 + 1 go through the tape offsets.
#   32x32     layer4 is 1 x 1, the decoder reflect-pads a 2 x 2 map
#   32x96, 96x32   deep maps one pixel high / wide
#   160x224   odd deep maps (5 x 7)
#   192x640   the KITTI size of the other tests
#   160x416   H/4: 4160 = 32 * 128 + 64 pixels -- KW = 1 with a half-empty last workgroup (layer1.*, up2, ic2)
#   320x1024  layer2.* in <3,4,2,1>, its downsample in <1,4,2,1>, layer3.* / up0 / ic0 in <3,2,1,4>, layer3's downsample <1,2,1,4>
#   352x1184  those with partial workgroups: H/8 6512 = 50 * 128 + 112 (the last wave has 16 of 32 pixels), H/16 1628 = 101 * 16 + 12
CASES = [
    (32, 32, 3, 2, "base", "sample"),
    (32, 96, 3, 2, "base", "sample"),
    (96, 32, 3, 2, "hard", "sample"),
    (160, 224, 3, 2, "base", "sample"),
    (160, 224, 3, 2, "hard", "special"),
    (192, 640, 3, 2, "base", "sample"),
    (160, 416, 3, 2, "base", "special"),
    (160, 416, 3, 2, "hard", "sample"),
    (320, 1024, 1, 1, "base", "sample"),
    (352, 1184, 1, 1, "base", "sample"),
    (352, 1184, 1, 1, "hard", "sample"),
]
CASE_IDS = [f"{H}x{W}-N{N}of{M}-{p}-{x}" for H, W, N, M, p, x in CASES]
SIZES = sorted({(H, W) for H, W, *_ in CASES})
OLD_SIZES = [(64, 192), (192, 640), (256, 448), (96, 320), (32, 32), (320, 96), (128, 128), (160, 224), (96, 128)]


# ---- inputs and parameter sets -----------------------------------------------------------------------------------------------------
def images(H, W, N, kind, seed=0):
    """[N,3,H,W] fp32.  'sample': depthnet_twin.sample_images, all images different.  'special': image 0 is exactly 0.45f everywhere
    (normalises to zero: every conv1 output is relu(b')), image 1 is 0.45f except its two outermost rows and columns (padding and
    reflection errors undiluted), the rest are samples"""
    x = dt.sample_images(9000 + seed + H + W, N, H, W)
    if kind == "special":
        c = np.float32(0.45)
        x[0] = c
        if N > 1:
            edge = x[1].copy()
            x[1] = c
            for sl in ((slice(None), slice(0, 2)), (slice(None), slice(H - 2, H)), (slice(None), slice(None), slice(0, 2)),
                       (slice(None), slice(None), slice(W - 2, W))):
                x[1][sl] = edge[sl]
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def params(pset, seed=3):
    return {"base": dt.depthnet_params, "hard": depthnet_params_hard}[pset](seed)


def depthnet_params_hard(seed=3):
    """depthnet_params(seed) with, in every BatchNorm: gamma negated on channels c % 4 == 2; the running variance of channels
    c % 8 == 3 multiplied by 1e-3 .. 1e-1 (fold factors up to 30 x their neighbours'); the running mean of channels c % 4 == 1 moved
    2 .. 5 standard deviations either way; then gamma and beta of the layer scaled by ONE factor so that the layer's output RMS on
    the calibration images is the base set's (activations stay O(1) through 20 layers).  Decoder: the bias of every third channel
    of the up-convolutions and iconvs is -3 .. -6 (those channels sit on the ELU's saturated side)."""
    base = dt.depthnet_params(seed)
    sd = OrderedDict((k, v.double().clone()) for k, v in base.items())
    rng = np.random.default_rng(7700 + seed)
    x = torch.from_numpy(dt.sample_images(7000 + seed, 2, 64, 192)).double()
    base64 = {k: v.double() for k, v in base.items()}
    want = {}

    def record(t, p):
        y = dt._bn_eval(base64)(t, p)
        want[p] = float(y.pow(2).mean().sqrt())
        return y

    def harden(t, p):
        n = t.shape[1]
        c = np.arange(n)
        g, var, mean = sd[f"{p}.weight"].numpy(), sd[f"{p}.running_var"].numpy(), sd[f"{p}.running_mean"].numpy()
        g[c % 4 == 2] *= -1.0
        var[c % 8 == 3] *= 10.0 ** rng.uniform(-3, -1, size=int((c % 8 == 3).sum()))
        m = c % 4 == 1
        mean[m] += rng.uniform(2, 5, size=int(m.sum())) * rng.choice([-1.0, 1.0], size=int(m.sum())) * np.sqrt(var[m])
        y = dt._bn_eval(sd)(t, p)
        r = want[p] / float(y.pow(2).mean().sqrt())
        sd[f"{p}.weight"] *= r
        sd[f"{p}.bias"] *= r
        return y * r
    with torch.no_grad():
        dt._encode(base64, x, record, lambda z, e: F.relu(z), lambda h: F.max_pool2d(h, 3, 2, 1))
        dt._encode(sd, x, harden, lambda z, e: F.relu(z), lambda h: F.max_pool2d(h, 3, 2, 1))
    for i in range(5):
        for k in (f"depth_upconvs.{i}.1.conv.bias", f"iconvs.{i}.0.conv.bias"):
            b = sd[k].numpy()
            m = np.arange(b.size) % 3 == 0
            b[m] = -rng.uniform(3, 6, size=int(m.sum()))
    return OrderedDict((k, v.float()) for k, v in sd.items())


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def fold64(sd, L):
    """(w', b') of convolution L in float64"""
    w = torch.as_tensor(sd[L["w"]]).double()
    if L["bn"]:
        g, be, rm, rv = (torch.as_tensor(sd[f"{L['bn']}.{k}"]).double() for k in ("weight", "bias", "running_mean", "running_var"))
        sc = g / torch.sqrt(rv + 1e-5)
        return w * sc.view(-1, 1, 1, 1), be - rm * sc
    return w, torch.as_tensor(sd[L["b"]]).double()


def nchw(t):
    """a tape entry [N,h,w,C] as [N,C,h,w]"""
    return t.permute(0, 3, 1, 2)


def gather(L, a, shift_up=0, reflect_off=0):
    """the convolution's operand grid: nearest x2 up-sampling, then reflect padding (zero padding is left to conv2d).  shift_up /
    reflect_off build the faulty kernels of the CPU tests: up-sampling shifted by one, the far-edge reflection index off by one"""
    if L["up"]:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
        if shift_up:
            a = torch.cat([a[..., :1], a[..., :-1]], -1)
    if L["reflect"]:
        a = F.pad(a, (1, 1, 1, 1), mode="reflect")
        if reflect_off:     # column vw (index 2 vw - 2 - vw = vw - 2) read as vw - 1; the same for the last row
            a = a.clone()
            a[..., -1] = a[..., -2]
            a[..., -1, :] = a[..., -2, :]
    return a


def conv(L, a, w, b, **fault):
    """convolution L on its operand a [N,cin,ih,iw] in a's dtype: the pre-activation"""
    return F.conv2d(gather(L, a, **fault), w, b, L["stride"], 0 if L["reflect"] else (L["ks"] - 1) // 2)


def conv_bound(L, a64, w64, b64, extra_c=0, extra_mag=None):
    """g(K + 3 + extra_c) (|a| conv |w'| + |b'| + extra_mag)"""
    mag = conv(L, a64.abs(), w64.abs(), b64.abs())
    if extra_mag is not None:
        mag = mag + extra_mag
    return gamma_n(L["cin"] * L["ks"] ** 2 + C_CONV + extra_c) * mag


def conv1_operand(imgs, dtype=torch.float64, c045=float(np.float32(0.45))):
    """(img - 0.45f) / 0.22: the fp32 constant the library (and the reference's fp32 program) subtracts, so that a frame of 0.45f is a
    frame of zeros.  The float64 twin subtracts the double 0.45 (c045=0.45: the CPU test that chains the references to it)"""
    if dtype == torch.float64:
        return (imgs.double() - c045) / 0.22
    return (imgs - 0.45) / 0.22


def elu(v):
    return torch.where(v > 0, v, torch.expm1(v.clamp(max=0)))


def _fp32(L, sd):
    w, b = fold64(sd, L)
    return w.float(), b.float()


HEAD = dict(up=0, reflect=1, stride=1, ks=3, cin=8)


def checks(sd, H, W, enc, dec, want_fp32=True, fault=None, c045=float(np.float32(0.45))):
    """Every launch against its isolated reference.  enc / dec: the tapes' entries ([N, ...] fp32 CPU tensors; encoder entries as
    depthnet_twin.encoder_tape_entries gives them, decoder entries as decoder_tape_entries).  Yields dicts(name, layer (index into
    layers(), None for the pool and the head), out (the taped fp32 output, NCHW), ref, bound (float64; None: bit for bit), f32 (the same
    launch by torch's fp32 CPU convolution on the same operand, or None)).
    fault = (layer index or "head", dict(wfn=..., shift_up=..., reflect_off=...)): the launches that run that convolution also carry
    `faulty`, the fp32 result of a kernel with that fault (a weight image changed by wfn, or a gather fault of gather()), to be judged
    in place of `out` against the TRUE reference and the TRUE fp32 baseline -- the situation of a faulty kernel on the GPU."""
    LS = layers(H, W)

    def cv(dtype, faulty=False):
        def run(li, a32):
            L = HEAD if li == "head" else LS[li]
            if li == "head":
                w, b = (torch.as_tensor(sd[f"predict_disps.0.0.conv.{k}"]).to(dtype) for k in ("weight", "bias"))
            else:
                w, b = fold64(sd, L) if dtype == torch.float64 else _fp32(L, sd)
            kw = dict(fault[1]) if (faulty and fault[0] == li) else {}
            wfn = kw.pop("wfn", None)
            return conv(L, a32.to(dtype), wfn(w.clone()) if wfn else w, b, **kw)
        run.dtype = dtype
        return run

    def item(name, layer, out, make, bound, also=None, exact=None):
        """make(conv function) -> the launch's output from its convolutions; evaluated in float64, in fp32, and in fp32 with the fault"""
        hit = fault is not None and fault[0] in (layer, also)
        return dict(name=name, layer=layer, also=also, out=out, ref=make(cv(torch.float64)), bound=bound, exact=exact,
                    f32=make(cv(torch.float32)) if want_fp32 else None, faulty=make(cv(torch.float32, True)) if hit else None)

    def bound_conv(li, a32, extra_c=0, extra_mag=None):
        w, b = fold64(sd, LS[li])
        return conv_bound(LS[li], a32.double(), w, b, extra_c, extra_mag)

    with torch.no_grad():
        # conv1 and the max pool
        a64, a32 = conv1_operand(enc[0], c045=c045), conv1_operand(enc[0], torch.float32)
        yield item("conv1", 0, nchw(enc[1]), lambda c: F.relu(c(0, a64 if c.dtype == torch.float64 else a32)),
                   conv_bound(LS[0], a64, *fold64(sd, LS[0]), C_CONV1))
        yield dict(name="maxpool", layer=None, out=nchw(enc[2]), ref=F.max_pool2d(nchw(enc[1]), 3, 2, 1), bound=None, f32=None, faulty=None)
        li, e, h_e = 1, 3, 2
        for p, ci, co, s, ds in dt._blocks():
            x, t1 = nchw(enc[h_e]), nchw(enc[e])
            yield item(LS[li]["name"], li, t1, lambda c, li=li, x=x: F.relu(c(li, x)), bound_conv(li, x))
            if ds:
                idn, b_ds = cv(torch.float64)(li + 2, x), bound_conv(li + 2, x)
                yield item(LS[li + 1]["name"] + "+downsample", li + 1, nchw(enc[e + 1]),
                           lambda c, li=li, x=x, t1=t1: F.relu(c(li + 1, t1) + c(li + 2, x)),
                           bound_conv(li + 1, t1, C_ADD, idn.abs() + b_ds) + b_ds, also=li + 2)
            else:
                yield item(LS[li + 1]["name"], li + 1, nchw(enc[e + 1]),
                           lambda c, li=li, x=x, t1=t1: (lambda y: F.relu(y + x.to(y.dtype)))(c(li + 1, t1)),
                           bound_conv(li + 1, t1, C_ADD, x.double().abs()))
            li += 3 if ds else 2
            h_e = e + 1
            e += 2
        # decoder: entry 0 = skip 4; i < 4: (ELU before the skip add, up-convolution output, iconv output); i = 4: (up, iconv); features; disparity
        x, d = nchw(dec[0]), 1
        for i in range(5):
            if i < 4:
                skip = nchw(enc[SKIP_ENTRY[3 - i]])
                yield item(LS[li]["name"] + " (ELU)", li, nchw(dec[d]), lambda c, li=li, x=x: elu(c(li, x)), bound_conv(li, x, C_ELU))
                yield item(LS[li]["name"] + " (+skip)", li, nchw(dec[d + 1]),
                           lambda c, li=li, x=x, skip=skip: (lambda y: y + skip.to(y.dtype))(elu(c(li, x))),
                           bound_conv(li, x, C_ELU + C_ADD, skip.double().abs()), exact=nchw(dec[d]) + skip)
                d += 1
            else:
                yield item(LS[li]["name"], li, nchw(dec[d]), lambda c, li=li, x=x: elu(c(li, x)), bound_conv(li, x, C_ELU))
            u = nchw(dec[d])
            yield item(LS[li + 1]["name"], li + 1, nchw(dec[d + 1]), lambda c, li=li, u=u: elu(c(li + 1, u)), bound_conv(li + 1, u, C_ELU))
            x = nchw(dec[d + 1])
            d += 2
            li += 2
        yield item(LS[li]["name"], li, nchw(dec[d]), lambda c, li=li, x=x: elu(c(li, x)), bound_conv(li, x, C_ELU))
        f = nchw(dec[d])
        hw_, hb_ = (torch.as_tensor(sd[f"predict_disps.0.0.conv.{k}"]).double() for k in ("weight", "bias"))
        sig = torch.sigmoid(conv(HEAD, f.double(), hw_, hb_))
        mag = conv(HEAD, f.double().abs(), hw_.abs(), hb_.abs())
        it = item("predict_disps.0", "head", None, lambda c: torch.sigmoid(c("head", f)), gamma_n(72 + 1) * mag / 4 + 6 * U * sig)
        yield dict(it, layer=None, out=dec[d + 1].view(sig.shape))


def decoder_tape_shapes(H, W):
    """per-image shapes of the decoder tape's entries (dn_tape_layout, NHWC)"""
    LS = layers(H, W)
    up = [L for L in LS if L["kind"] in ("up+skip", "up")]
    shp = [(up[0]["ih"], up[0]["iw"], up[0]["cin"])]
    for i, L in enumerate(up):
        shp += [(L["oh"], L["ow"], L["cout"])] * (3 if i < 4 else 2)
    return shp + [(H, W, 8), (H, W)]


def encoder_tape_shapes(H, W):
    """the same from layers(): images, conv1's output, the pooled map, then each block's two outputs"""
    LS = layers(H, W)
    shp = [(3, H, W), (LS[0]["oh"], LS[0]["ow"], 64), (LS[0]["oh"] // 2, LS[0]["ow"] // 2, 64)]
    for L in LS[1:]:
        if L["kind"] in ("plain", "stride2", "residual"):
            shp.append((L["oh"], L["ow"], L["cout"]))
    return shp


def decoder_tape_entries(tape, N, H, W):
    shp = decoder_tape_shapes(H, W)
    assert tape.dim() == 1 and tape.numel() == N * sum(int(np.prod(s)) for s in shp)
    out, o = [], 0
    for s in shp:
        n = N * int(np.prod(s))
        out.append(tape[o:o + n].view(N, *s))
        o += n
    return out


def twin_tapes(sd, x, dtype=torch.float64, c045=float(np.float32(0.45))):
    """(encoder entries, decoder entries, disparity, skips) of the plain twin in `dtype`, laid out as the library's tapes (NHWC).  The
    twin normalises with (x - 0.45) / 0.22; in fp32 that constant is 0.45f, the library's.  In float64 the images are moved by
    0.45 - c045 first, so that the float64 chain subtracts c045 = 0.45f as the library and the fp32 twin do, and the chained
    comparison carries no common offset of (0.45f - 0.45) / 0.22 = 5e-8 (c045=0.45: depthnet_twin.forward itself)"""
    p = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    enc = dt.twin_tape_entries(p, x.double() - (c045 - 0.45) if dtype == torch.float64 else x)
    enc[0] = x
    skips = [nchw(enc[e]) for e in SKIP_ENTRY]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    dec = [nhwc(skips[4])]
    with torch.no_grad():
        h = skips[4]
        for i in range(5):
            u = F.elu(dt._conv_refl(F.interpolate(h, scale_factor=2, mode="nearest"), p[f"depth_upconvs.{i}.1.conv.weight"],
                                    p[f"depth_upconvs.{i}.1.conv.bias"]))
            if i < 4:
                dec.append(nhwc(u))
                u = u + skips[3 - i]
            dec.append(nhwc(u))
            h = F.elu(dt._conv_refl(u, p[f"iconvs.{i}.0.conv.weight"], p[f"iconvs.{i}.0.conv.bias"]))
            dec.append(nhwc(h))
        f = F.elu(dt._conv_refl(h, p["feature_convs.0.0.conv.weight"], p["feature_convs.0.0.conv.bias"]))
        disp = torch.sigmoid(dt._conv_refl(f, p["predict_disps.0.0.conv.weight"], p["predict_disps.0.0.conv.bias"]))
    dec += [nhwc(f), disp[:, 0]]
    return enc, dec, disp, skips


def judge(c):
    """one checks() item -> dict(name, frac (largest error over bound; for a bit-for-bit check 0.0 or inf), rel, rel32, mx, mx32,
    ok_bound, ok_hold, ok = both and the exact check)"""
    out, ref = c["out"], c["ref"]
    assert out.shape == ref.shape, (c["name"], out.shape, ref.shape)
    if c["bound"] is None:
        same = torch.equal(out, ref)
        return dict(name=c["name"], frac=0.0 if same else float("inf"), rel=0.0, rel32=0.0, mx=0.0, mx32=0.0, ok_bound=same, ok_hold=True, ok=same)
    finite = bool(torch.isfinite(out).all())
    frac = float(((out.double() - ref).abs() / c["bound"].clamp_min(1e-300)).max()) if finite else float("inf")
    r = dict(name=c["name"], frac=frac, rel=rel_l2(out, ref), mx=max_over_rms(out, ref), rel32=float("nan"), mx32=float("nan"))
    r["ok_bound"], r["ok_hold"] = finite and frac <= 1.0, True
    if c["f32"] is not None:
        r["rel32"], r["mx32"] = rel_l2(c["f32"], ref), max_over_rms(c["f32"], ref)
        r["ok_hold"] = finite and r["rel"] <= hold(FLOOR_REL_L2, r["rel32"]) and r["mx"] <= hold(FLOOR_MAX_RMS, r["mx32"])
    r["ok"] = r["ok_bound"] and r["ok_hold"] and (c.get("exact") is None or torch.equal(out, c["exact"]))
    return r


def relu_flips(a, b):
    """elements of two post-ReLU tensors where one is zero and the other positive"""
    return (a > 0) != (b > 0)
