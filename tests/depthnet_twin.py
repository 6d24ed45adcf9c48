"""Depth-network test twin: a seeded parameter set under the reference module's state_dict names (depthnet_params) and a plain
torch.nn.functional restatement of the network (DepthNetTwin: ResNet18 encoder with BatchNorm in evaluation mode, U-Net decoder of
models/depth_w_access.py with num_scales = 1).  Used by the CPU tests, the GPU tests and scripts/depthnet_timing.py.  forward_pinned
is the same network with the ReLU and max-pool decisions of a recorded encoder tape (encoder_tape_entries), the float64 reference
of the HIP backward's exactness tests."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ENC = "encoder.encoder."
PLANES = [512, 256, 128, 64, 64, 32]


def _blocks():
    """(prefix, cin, cout, stride, has_downsample) of the eight BasicBlocks"""
    out, c = [], 64
    for li in range(1, 5):
        co = {1: 64, 2: 128, 3: 256, 4: 512}[li]
        for b in range(2):
            s = 2 if (b == 0 and li > 1) else 1
            out.append((f"{ENC}layer{li}.{b}.", c, co, s, s == 2))
            c = co
    return out


def param_shapes():
    """state_dict names and shapes of the reference depth_model (num_scales = 1) without fc.* and num_batches_tracked, in module order"""
    sh = OrderedDict()

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{p}.{k}"] = (c,)
    sh[f"{ENC}conv1.weight"] = (64, 3, 7, 7)
    bn(f"{ENC}bn1", 64)
    for p, ci, co, s, ds in _blocks():
        sh[f"{p}conv1.weight"] = (co, ci, 3, 3)
        bn(f"{p}bn1", co)
        sh[f"{p}conv2.weight"] = (co, co, 3, 3)
        bn(f"{p}bn2", co)
        if ds:
            sh[f"{p}downsample.0.weight"] = (co, ci, 1, 1)
            bn(f"{p}downsample.1", co)
    for i in range(5):
        sh[f"depth_upconvs.{i}.1.conv.weight"] = (PLANES[i + 1], PLANES[i], 3, 3)
        sh[f"depth_upconvs.{i}.1.conv.bias"] = (PLANES[i + 1],)
    for i in range(5):
        sh[f"iconvs.{i}.0.conv.weight"] = (PLANES[i + 1], PLANES[i + 1], 3, 3)
        sh[f"iconvs.{i}.0.conv.bias"] = (PLANES[i + 1],)
    sh["feature_convs.0.0.conv.weight"] = (8, 32, 3, 3)
    sh["feature_convs.0.0.conv.bias"] = (8,)
    sh["predict_disps.0.0.conv.weight"] = (1, 8, 3, 3)
    sh["predict_disps.0.0.conv.bias"] = (1,)
    return sh


def sample_images(seed: int, N: int, H: int, W: int) -> np.ndarray:
    """[N,3,H,W] float32 images in [0, 1]: smooth colour ramps + blobs + noise (numpy RandomState: stable across versions)"""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.empty((N, 3, H, W), dtype=np.float64)
    for n in range(N):
        for c in range(3):
            a, b, ph = rs.uniform(1, 6, 2), rs.uniform(0, 1), rs.uniform(0, 2 * np.pi)
            img = 0.5 + 0.25 * np.sin(a[0] * np.pi * x + ph) * np.cos(a[1] * np.pi * y) + 0.2 * (b - 0.5) * (x - y)
            out[n, c] = img + 0.08 * rs.standard_normal((H, W))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def _conv_refl(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)


def _encode(sd, x, bn, relu, pool):
    """the encoder's skips; relu(z, e) is the ReLU whose output is encoder tape entry e (encoder_tape_entries), pool the max pool"""
    x = (x - 0.45) / 0.22
    h = relu(bn(F.conv2d(x, sd[f"{ENC}conv1.weight"], None, 2, 3), f"{ENC}bn1"), 1)
    skips = [h]
    h = pool(h)
    for j, (p, ci, co, s, ds) in enumerate(_blocks()):
        o = relu(bn(F.conv2d(h, sd[f"{p}conv1.weight"], None, s, 1), f"{p}bn1"), 3 + 2 * j)
        o = bn(F.conv2d(o, sd[f"{p}conv2.weight"], None, 1, 1), f"{p}bn2")
        idn = bn(F.conv2d(h, sd[f"{p}downsample.0.weight"], None, s, 0), f"{p}downsample.1") if ds else h
        h = relu(o + idn, 4 + 2 * j)
        if p.endswith(".1."):
            skips.append(h)
    return skips


def _bn_eval(sd):
    return lambda t, p: F.batch_norm(t, sd[f"{p}.running_mean"], sd[f"{p}.running_var"], sd[f"{p}.weight"], sd[f"{p}.bias"], False,
                                     0.0, 1e-5)


def forward(sd, x, calibrate: bool = False, return_skips: bool = False):
    """the network on images x [N,3,H,W] with parameters sd (tensors of x's dtype / device).  calibrate: every BatchNorm's running
    statistics are first SET to the batch statistics of its input (used once by depthnet_params)."""
    def bn(t, p):
        if calibrate:
            sd[f"{p}.running_mean"] = t.mean((0, 2, 3)).detach().clone()
            sd[f"{p}.running_var"] = t.var((0, 2, 3)).detach().clone()
        return _bn_eval(sd)(t, p)

    skips = _encode(sd, x, bn, lambda z, e: F.relu(z), lambda h: F.max_pool2d(h, 3, 2, 1))
    disp = _decode(sd, skips)
    return (disp, skips) if return_skips else disp


def encoder_tape_shapes(H: int, W: int):
    """per-image shapes of the encoder tape's entries (depthnet_host.h dn_tape_layout): images [3,H,W], conv1's output (skip 0)
    [H/2,W/2,64], the max-pooled map [H/4,W/4,64], then for each of the eight BasicBlocks its conv1 output and its block output,
    [h,w,c] each (NHWC, both after their ReLU)"""
    shp = [(3, H, W), (H // 2, W // 2, 64), (H // 4, W // 4, 64)]
    h, w = H // 4, W // 4
    for p, ci, co, s, ds in _blocks():
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        shp += [(h, w, co), (h, w, co)]
    return shp


def encoder_tape_entries(tape, N: int, H: int, W: int):
    """a flat encoder tape of N images split into its entries (views, in tape order), each [N, *encoder_tape_shapes(H, W)[e]]: the
    tape is entry-major, every entry [N][per-image size]"""
    shp = encoder_tape_shapes(H, W)
    total = N * sum(int(np.prod(s)) for s in shp)
    if tape.dim() != 1 or tape.numel() != total:
        raise ValueError(f"encoder tape of {tuple(tape.shape)} floats: expected {total} for N={N}, {H} x {W}")
    out, o = [], 0
    for s in shp:
        n = N * int(np.prod(s))
        out.append(tape[o:o + n].view(N, *s))
        o += n
    return out


def twin_tape_entries(sd, x):
    """the encoder tape entries (encoder_tape_entries' list, NHWC) of the plain forward on parameters sd: every ReLU output and the
    pooled map as the forward computes them, in sd's dtype"""
    ent = {0: x}

    def relu(z, e):
        ent[e] = F.relu(z)
        return ent[e]

    def pool(h):
        ent[2] = F.max_pool2d(h, 3, 2, 1)
        return ent[2]
    with torch.no_grad():
        _encode(sd, x.to(sd[f"{ENC}conv1.weight"].dtype), _bn_eval(sd), relu, pool)
    return [ent[e] if e == 0 else ent[e].permute(0, 2, 3, 1).contiguous() for e in range(len(ent))]


def maxpool_argmax(a):
    """argmax of every window of max_pool2d(a, 3, 2, 1) on a [N,C,h,w], as flat indices into h * w (torch's return_indices
    convention): the first strict maximum in row-major window order, padding excluded -- k_dnb_maxpool's rule"""
    N, C, h, w = a.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    best = a.new_full((N, C, oh, ow), float("-inf"))
    idx = torch.full((N, C, oh, ow), -1, dtype=torch.long, device=a.device)
    oy, ox = torch.arange(oh, device=a.device), torch.arange(ow, device=a.device)
    for ky in range(3):
        iy = 2 * oy - 1 + ky
        for kx in range(3):
            ix = 2 * ox - 1 + kx
            valid = ((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < w))[None, :]
            cy, cx = iy.clamp(0, h - 1), ix.clamp(0, w - 1)
            v = a[:, :, cy][:, :, :, cx]
            take = valid & ((v > best) | (idx < 0))
            best = torch.where(take, v, best)
            idx = torch.where(take, (cy[:, None] * w + cx[None, :]).expand_as(idx), idx)
    return idx


def forward_pinned(sd, x, entries):
    """(disp, skips): the forward in the parameters' dtype with the ReLU and max-pool decisions of a recorded encoder tape
    (encoder_tape_entries; e.g. the HIP training forward's): every ReLU is z * [tape output > 0] and the max pool gathers at
    maxpool_argmax of the tape's conv1 output.  For fixed decisions the network is smooth, so float64 autograd through it is the
    exact gradient the fp32 backward approximates.  The decoder is _decode."""
    dt = sd[f"{ENC}conv1.weight"].dtype

    def relu(z, e):
        return z * (entries[e] > 0).permute(0, 3, 1, 2).to(dt)

    idx = maxpool_argmax(entries[1].permute(0, 3, 1, 2))

    def pool(h):
        return h.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    skips = _encode(sd, x.to(dt), _bn_eval(sd), relu, pool)
    return _decode(sd, skips), skips


def depthnet_params(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """seeded float32 state_dict under the reference names: He-scaled convolutions, non-trivial BatchNorm affine parameters, running
    statistics calibrated (float64) on seeded images so that activations stay O(1); the head is scaled so the sigmoid is not saturated"""
    rs = np.random.RandomState(1000 + seed)
    sd = OrderedDict()
    for k, s in param_shapes().items():
        if k.endswith(".weight") and len(s) == 4:
            v = rs.standard_normal(s) * np.sqrt(2.0 / np.prod(s[1:]))
        elif k.endswith("running_var"):
            v = np.ones(s)
        elif k.endswith("running_mean"):
            v = np.zeros(s)
        elif ".bn" in k or "downsample.1" in k:
            v = rs.uniform(0.6, 1.4, s) if k.endswith(".weight") else rs.uniform(-0.3, 0.3, s)
        else:                                                         # convolution biases of the decoder
            v = rs.uniform(-0.1, 0.1, s)
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float64))
    # decoder scale: 1 / sqrt(2) per skip addition keeps the sums O(1); the head makes a disparity spread of a few tenths
    for i in range(4):
        sd[f"depth_upconvs.{i}.1.conv.weight"] *= np.sqrt(0.5)
    sd["predict_disps.0.0.conv.weight"] *= 0.5
    sd["predict_disps.0.0.conv.bias"][:] = -1.0
    with torch.no_grad():
        forward(sd, torch.from_numpy(sample_images(7000 + seed, 2, 64, 192)).double(), calibrate=True)
    return OrderedDict((k, v.float()) for k, v in sd.items())


class DepthNetTwin(torch.nn.Module):
    """the reference depth_model's call convention over `forward` (fp32 or fp64 by the parameters' dtype, on their device)"""

    def __init__(self, params, dtype=torch.float32, device="cpu"):
        super().__init__()
        self.p = OrderedDict((k, v.to(device=device, dtype=dtype)) for k, v in params.items())
        for i, (k, v) in enumerate(self.p.items()):
            self.register_buffer(f"t{i}", v, persistent=False)

    def state_dict(self, *a, **kw):     # the reference names (is_reference_depthnet / DepthNetHIP.load read them)
        return OrderedDict(self.p)

    def forward(self, x=None, skips=None, return_disp=True, epoch=0):
        if x is not None:
            disp, sk = forward(self.p, x.to(next(iter(self.p.values())).dtype), return_skips=True)
            return ([disp], sk) if return_disp else (None, sk)
        return [_decode(self.p, skips)], skips


def _decode(sd, skips):
    x = skips[-1]
    for i in range(5):
        u = F.elu(_conv_refl(F.interpolate(x, scale_factor=2, mode="nearest"), sd[f"depth_upconvs.{i}.1.conv.weight"],
                             sd[f"depth_upconvs.{i}.1.conv.bias"]))
        if i < 4:
            u = u + skips[3 - i]
        x = F.elu(_conv_refl(u, sd[f"iconvs.{i}.0.conv.weight"], sd[f"iconvs.{i}.0.conv.bias"]))
    f = F.elu(_conv_refl(x, sd["feature_convs.0.0.conv.weight"], sd["feature_convs.0.0.conv.bias"]))
    return torch.sigmoid(_conv_refl(f, sd["predict_disps.0.0.conv.weight"], sd["predict_disps.0.0.conv.bias"]))
