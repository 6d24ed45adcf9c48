"""GPU: the depth network's backward pass (csrc/depthnet_grad_kernel.h, tcsfm_depthnet_*_train / *_backward) at fp32 accuracy.

The encoder's gradients are compared with float64 autograd through tests/depthnet_twin.py forward_pinned: the twin's network with
the HIP training forward's own ReLU masks and max-pool argmaxes, read from a tape of tcsfm_depthnet_encode_train.  With the
decisions fixed the backward is linear in the cotangent, so what remains is fp32 rounding, and every tensor is held to a bound
at most about 10x its worst measured error instead of test_gpu_depthnet_grad.py's 1e-2 (there fp32 and float64 may decide a ReLU
differently).  Each tensor is checked two ways: relative L2, and its largest elementwise error over the reference's RMS element.

Measured on an MI355X over every case below (worst value; bound):
  encoder (60 tensors), relative L2 ........ 1.4e-5 (layer4.1.bn1.weight, KITTI size, disparity cotangent); 1e-4
  encoder, max error / RMS ................. 2.7e-4 (layer4.0.conv2.weight, the same case); 2e-3
  decoder skip gradients, relative L2 ...... 4.1e-6 (skip 4, KITTI size); 4e-5
  decoder skip gradients, max error / RMS .. 6.3e-5 (skip 0, border-only cotangent); 5e-4
  decoder parameters, relative L2 .......... 5.7e-6 (iconvs.4.0.conv.bias); 5e-5
  decoder parameters, max error / RMS ...... 5.1e-5 (depth_upconvs.0.1.conv.weight); 5e-4
The BatchNorm weight gradients (sum_k dw' w - db' mean) / sqrt(var + eps) show no cancellation beyond the rest: their worst relative
error is that of the convolution weights (1.3e-5) and the BatchNorm biases (1.4e-5).  The elementwise errors are largest in
layer 4, whose weight gradients sum over the fewest pixels.
The decoder's skip gradients (d_skips, what the reference's bottleneck-value tuning optimises) need no pinning: the decoder has
no ReLU.  Gradients that must be zero (parameters above the only skip with a cotangent) are checked to be exactly zero.

The last test checks the pruning of unrequested work (dn_encode_backward's `before[]`, dn_decode_backward's `low` / `skip_src` /
head request): a gradient requested alone has the bits of the same gradient from a run that requests everything."""
import ctypes as C
import math
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depthnet_twin as dt  # noqa: E402

SKIP_C = (64, 64, 128, 256, 512)
SKIP_ENTRY = (1, 6, 10, 14, 18)            # tape entries of skips 0..4: conv1's output, then the output of layerK.1
ENC_REL, ENC_ELEM = 1e-4, 2e-3             # encoder tensors: relative L2, max error / RMS (measured values: module docstring)
SKIP_REL, SKIP_ELEM = 4e-5, 5e-4           # decoder skip gradients
DEC_REL, DEC_ELEM = 5e-5, 5e-4             # decoder parameters (skips as leaves)

# (N, H, W, max_images): the smallest legal size (layer 4 is 1 x 1, the decoder reflect-pads 2 x 2 maps); tall; square in two
# groups; odd deep maps (layer 4 is 5 x 7) with conv1's 8960 pixels not a multiple of the weight gradient's 2048-pixel chunk;
# groups of 2 + 2 + 1; the KITTI size
SHAPES = [(1, 32, 32, 1), (2, 320, 96, 2), (2, 128, 128, 1), (3, 160, 224, 2), (5, 96, 320, 2), (2, 192, 640, 6)]
EDGE = (3, 160, 224, 2)                    # the shape of the per-skip and border-only cases


def _module(seed=0, max_images=6):
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    return DepthNetModule(dt.depthnet_params(seed), max_images=max_images).cuda()


def _imgs(seed, N, H, W):
    return torch.from_numpy(dt.sample_images(seed, N, H, W)).cuda()


def _border(t):
    """t with only its first and last rows and columns kept"""
    m = torch.zeros_like(t)
    m[..., 0, :] = m[..., -1, :] = m[..., :, 0] = m[..., :, -1] = 1
    return t * m


def cotangents(seed, N, H, W, disp=True, skips=(0, 1, 2, 3, 4), border=False):
    """(R [N,1,H,W] or None, [R_k [N,C,h,w] or None]): float64 values that are exact in float32, on the GPU"""
    g = torch.Generator().manual_seed(seed)

    def draw(shape):
        r = torch.randn(shape, generator=g, dtype=torch.float32).double().cuda()
        return _border(r) if border else r
    R = draw((N, 1, H, W)) if disp else None
    Rs = [draw((N, c, H >> (k + 1), W >> (k + 1))) if k in skips else None for k, c in enumerate(SKIP_C)]
    return R, Rs


def _loss(disp, skips, R, Rs):
    dt_ = skips[0].dtype
    loss = (disp * R.to(dt_)).sum() if R is not None else 0
    for s, r in zip(skips, Rs):
        if r is not None:
            loss = loss + (s * r.to(dt_)).sum()
    return loss


def tape_entries(mod, x):
    """the encoder tape of the module's training forward on x (tcsfm_depthnet_encode_train into a tape this test owns), split by
    depthnet_twin.encoder_tape_entries after checking its size against tcsfm_depthnet_tape_size and its images and skips"""
    nat = mod._native_for(x)
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    e, d = C.c_int64(), C.c_int64()
    nat.eng._call(nat.lib.tcsfm_depthnet_tape_size(nat.dn, N, C.byref(e), C.byref(d)))
    assert int(e.value) == N * sum(math.prod(s) for s in dt.encoder_tape_shapes(H, W))
    tape = torch.full((int(e.value),), float("nan"), device=x.device)
    sk = [torch.empty((N, H >> (k + 1), W >> (k + 1), c), device=x.device) for k, c in enumerate(SKIP_C)]
    nat.eng._bind()
    nat.eng._call(nat.lib.tcsfm_depthnet_encode_train(nat.dn, N, nat.eng._p(x), C.cast(nat.ptrs(sk), C.c_void_p), nat.eng._p(tape)))
    entries = dt.encoder_tape_entries(tape, N, H, W)
    assert bool(torch.isfinite(tape).all()), "the training forward left part of the tape unwritten"
    assert torch.equal(entries[0].reshape(x.shape), x)
    for k, ei in enumerate(SKIP_ENTRY):
        assert torch.equal(entries[ei], sk[k]), k
    return entries


def _ref_params(seed, want):
    sd = {k: v.double().cuda() for k, v in dt.depthnet_params(seed).items()}
    for k, v in sd.items():
        v.requires_grad_(want(k) and not k.endswith(("running_mean", "running_var")))
    return sd


def _errs(g, ref):
    """(relative L2, max |error| / RMS of ref); a reference that is zero (or None: no path) needs exactly zero"""
    g = g.double()
    if ref is None or not bool(ref.any()):
        return (0.0, 0.0) if not bool(g.any()) else (math.inf, math.inf)
    d = g - ref
    rms = ref.norm() / math.sqrt(ref.numel())
    return float(d.norm() / ref.norm()), float(d.abs().max() / rms)


def encoder_errors(N, H, W, max_images, R, Rs, seed=0):
    """name -> (relative L2, max error / RMS) of the module's 60 encoder gradients against float64 autograd through
    forward_pinned on the module's own tape"""
    mod = _module(seed, max_images)
    x = _imgs(100 + N + H + W, N, H, W)
    entries = tape_entries(mod, x)
    disps, skips = mod(x, return_disp=R is not None)
    for k, ei in enumerate(SKIP_ENTRY):
        assert torch.equal(skips[k].detach().permute(0, 2, 3, 1), entries[ei]), k
    _loss(disps[0] if R is not None else None, skips, R, Rs).backward()
    hip = {k: p.grad for k, p in mod.named_parameters() if k.startswith(dt.ENC)}
    assert len(hip) == 60 and all(g is not None for g in hip.values())
    sd = _ref_params(seed, lambda k: k.startswith(dt.ENC))
    disp, sk = dt.forward_pinned(sd, x.double(), entries)
    _loss(disp if R is not None else None, sk, R, Rs).backward()
    return {k: _errs(g, sd[k].grad) for k, g in hip.items()}


def decoder_errors(N, H, W, max_images, R, dec_on, seed=0):
    """skip k -> errors of the module's d_skips (skips as leaves), and with dec_on each decoder parameter's, against float64
    autograd of _decode on the same skip values"""
    mod = _module(seed, max_images)
    x = _imgs(200 + N + H + W, N, H, W)
    with torch.no_grad():
        _, sk = mod(x, return_disp=False)
    for k, p in mod.named_parameters():
        p.requires_grad_(dec_on and not k.startswith(dt.ENC))
    leaves = [s.clone().requires_grad_(True) for s in sk]
    (mod(None, skips=leaves)[0][0] * R.float()).sum().backward()
    sd = _ref_params(seed, lambda k: dec_on and not k.startswith(dt.ENC))
    ref_leaves = [s.detach().double().requires_grad_(True) for s in sk]
    (dt._decode(sd, ref_leaves) * R).sum().backward()
    out = {f"skip{k}": _errs(a.grad, b.grad) for k, (a, b) in enumerate(zip(leaves, ref_leaves))}
    if dec_on:
        for k, p in mod.named_parameters():
            if not k.startswith(dt.ENC):
                out[k] = _errs(p.grad, sd[k].grad)
    return out


def _over(errs, rel, elem):
    return {k: e for k, e in errs.items() if not (e[0] <= rel and e[1] <= elem)}


# ---- a. encoder gradients against the pinned float64 reference ------------------------------------------------------------

@pytest.mark.parametrize("with_skips", [False, True], ids=["disp", "disp+skips"])
@pytest.mark.parametrize("N,H,W,mi", SHAPES)
def test_encoder_gradients_pinned(N, H, W, mi, with_skips):
    R, Rs = cotangents(N + H + W, N, H, W, skips=(0, 1, 2, 3, 4) if with_skips else ())
    bad = _over(encoder_errors(N, H, W, mi, R, Rs), ENC_REL, ENC_ELEM)
    assert not bad, bad


@pytest.mark.parametrize("k", range(5))
def test_encoder_gradients_pinned_single_skip(k):
    """a cotangent on skip k alone: its injection point (skip 0: k_dnb_maxpool; 1-3: the down-block's data-gradient epilogue;
    4: dnb_ew) is the only source, and every parameter above it gets exactly zero"""
    N, H, W, mi = EDGE
    R, Rs = cotangents(40 + k, N, H, W, disp=False, skips=(k,))
    errs = encoder_errors(N, H, W, mi, R, Rs)
    bad = _over(errs, ENC_REL, ENC_ELEM)
    assert not bad, bad
    assert sum(e == (0.0, 0.0) for e in errs.values()) == (57, 45, 30, 15, 0)[k]


def test_encoder_gradients_pinned_border_only():
    """cotangents only on the first and last rows and columns of the disparity and of every skip: edge handling errors are not
    diluted by interior pixels"""
    N, H, W, mi = EDGE
    R, Rs = cotangents(50, N, H, W, border=True)
    bad = _over(encoder_errors(N, H, W, mi, R, Rs), ENC_REL, ENC_ELEM)
    assert not bad, bad


# ---- b. decoder skip gradients against float64 autograd --------------------------------------------------------------------

def _decoder_over(errs):
    return {**_over({k: e for k, e in errs.items() if k.startswith("skip")}, SKIP_REL, SKIP_ELEM),
            **_over({k: e for k, e in errs.items() if not k.startswith("skip")}, DEC_REL, DEC_ELEM)}


@pytest.mark.parametrize("dec_on", [False, True], ids=["frozen", "decoder"])
@pytest.mark.parametrize("N,H,W,mi", SHAPES)
def test_decoder_skip_gradients(N, H, W, mi, dec_on):
    R, _ = cotangents(60 + N + H + W, N, H, W, skips=())
    bad = _decoder_over(decoder_errors(N, H, W, mi, R, dec_on))
    assert not bad, bad


def test_decoder_skip_gradients_border_only():
    N, H, W, mi = EDGE
    R, _ = cotangents(70, N, H, W, skips=(), border=True)
    bad = _decoder_over(decoder_errors(N, H, W, mi, R, True))
    assert not bad, bad


# ---- c. pruning: a gradient requested alone has the bits of a run that requests everything -------------------------------

ENC_ALONE = ["conv1.weight", "bn1.weight", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight", "layer2.0.downsample.1.bias",
             "layer3.1.bn2.weight", "layer4.1.conv2.weight"]
DEC_ALONE = ["predict_disps.0.0.conv.", "feature_convs.", "depth_upconvs.0."]


def test_pruned_requests_return_the_same_bits():
    N, H, W, mi = 3, 96, 128, 2
    mod = _module(1, mi)
    x = _imgs(80, N, H, W)
    R, Rs = cotangents(81, N, H, W)
    names = [k for k, _ in mod.named_parameters()]

    def run(want, leaves=None):
        mod.zero_grad(set_to_none=True)
        for k, p in mod.named_parameters():
            p.requires_grad_(want(k))
        if leaves is None:
            disps, skips = mod(x)
        else:
            for s in leaves:
                s.grad = None
            disps, skips = mod(None, skips=leaves)
        _loss(disps[0], skips, R, Rs if leaves is None else [None] * 5).backward()
        return {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None}

    full = run(lambda k: True)
    assert sorted(full) == sorted(names)
    for name in ENC_ALONE:
        got = run(lambda k: k == dt.ENC + name)
        assert sorted(got) == [dt.ENC + name]
        assert torch.equal(got[dt.ENC + name], full[dt.ENC + name]), name
    for pre in DEC_ALONE:
        got = run(lambda k: k.startswith(pre))
        assert sorted(got) == sorted(k for k in names if k.startswith(pre)) and got, pre
        for k, g in got.items():
            assert torch.equal(g, full[k]), k
    # skips as leaves: all of them and the decoder, then each leaf alone with the decoder frozen
    with torch.no_grad():
        _, sk = mod(x, return_disp=False)
    leaves = [s.clone().requires_grad_(True) for s in sk]
    dec = run(lambda k: not k.startswith(dt.ENC), leaves)
    for k, g in dec.items():
        assert torch.equal(g, full[k]), k
    all_leaf = [s.grad.clone() for s in leaves]
    for j in range(5):
        one = [s.clone().requires_grad_(i == j) for i, s in enumerate(sk)]
        assert run(lambda k: False, one) == {}
        assert all(s.grad is None for i, s in enumerate(one) if i != j)
        assert torch.equal(one[j].grad, all_leaf[j]), j
