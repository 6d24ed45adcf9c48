"""The reference's depth network as a differentiable torch.nn.Module on the HIP library: forward and backward run on the gfx950
kernels of csrc/depthnet_kernel.h and csrc/depthnet_grad_kernel.h (tcsfm_depthnet_*_train / *_backward), so the reference's own
test-time weight tuning (deep-copy, `depth_model.encoder.parameters()` into Adam, `loss.backward()`) runs on them unchanged."""
from __future__ import annotations

import copy
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from .depthnet import SKIP_CHANNELS, DepthNetHIP, named_table

_ENC = "encoder.encoder."
_PLANES = [512, 256, 128, 64, 64, 32]


def _shapes():
    """state_dict names and shapes of the reference depth_model (num_scales = 1), in module order (parameters, then BatchNorm
    running statistics as buffers)"""
    sh = OrderedDict()

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{p}.{k}"] = (c,)
    sh[f"{_ENC}conv1.weight"] = (64, 3, 7, 7)
    bn(f"{_ENC}bn1", 64)
    c = 64
    for li in range(1, 5):
        co = 64 << (li - 1)
        for b in range(2):
            p = f"{_ENC}layer{li}.{b}."
            s = 2 if (b == 0 and li > 1) else 1
            sh[f"{p}conv1.weight"] = (co, c, 3, 3)
            bn(f"{p}bn1", co)
            sh[f"{p}conv2.weight"] = (co, co, 3, 3)
            bn(f"{p}bn2", co)
            if s == 2:
                sh[f"{p}downsample.0.weight"] = (co, c, 1, 1)
                bn(f"{p}downsample.1", co)
            c = co
    for i in range(5):
        sh[f"depth_upconvs.{i}.1.conv.weight"] = (_PLANES[i + 1], _PLANES[i], 3, 3)
        sh[f"depth_upconvs.{i}.1.conv.bias"] = (_PLANES[i + 1],)
    for i in range(5):
        sh[f"iconvs.{i}.0.conv.weight"] = (_PLANES[i + 1], _PLANES[i + 1], 3, 3)
        sh[f"iconvs.{i}.0.conv.bias"] = (_PLANES[i + 1],)
    sh["feature_convs.0.0.conv.weight"] = (8, 32, 3, 3)
    sh["feature_convs.0.0.conv.bias"] = (8,)
    sh["predict_disps.0.0.conv.weight"] = (1, 8, 3, 3)
    sh["predict_disps.0.0.conv.bias"] = (1,)
    return sh


def _is_buffer(name: str) -> bool:
    return name.endswith("running_mean") or name.endswith("running_var")


class _Native:
    """the library state behind one module on one device and image size: a DepthNetHIP (engine + tcsfm_depthnet) fed by
    tcsfm_depthnet_load_device, and the version stamp of the parameters it holds"""

    def __init__(self, H, W, max_images, device):
        from .engine import Engine
        with torch.cuda.device(device):
            self.eng = Engine(H, W, 2, device=device.index)
        self.net = DepthNetHIP(self.eng, max_images)
        self.lib, self.dn = self.eng.lib, self.net._dn
        self.stamp = None
        e, d = C.c_int64(), C.c_int64()
        self.eng._call(self.lib.tcsfm_depthnet_tape_size(self.dn, 1, C.byref(e), C.byref(d)))
        self.tape_per_image = (int(e.value), int(d.value))

    def load(self, named):
        """named: [(name, contiguous float32 device tensor)]"""
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_depthnet_load_device(self.dn, *named_table(named)))

    @staticmethod
    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])

    def grads_call(self, fn, N, pre_args, named_out):
        self.eng._bind()
        self.eng._call(fn(self.dn, N, *pre_args, *named_table(named_out)[:3]))


def _check_stamp(ctx):
    """the backward reads the instance's current weights: refuse if a later forward re-folded different parameters into it"""
    if ctx.nat.stamp != ctx.stamp:
        raise RuntimeError("DepthNetModule: a parameter or buffer changed in place and another forward ran before this graph's "
                           "backward; the backward would use the new weights.  Run backward before updating the parameters.")


def _nhwc(s: torch.Tensor) -> torch.Tensor:
    return DepthNetHIP._to_nhwc(s)


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, *params):
        nat = mod._native_for(x)
        N = x.shape[0]
        imgs = x.float().contiguous()
        tape = torch.empty(N * nat.tape_per_image[0], device=x.device, dtype=torch.float32)
        skips = [torch.empty((N, nat.eng.H >> (k + 1), nat.eng.W >> (k + 1), c), device=x.device, dtype=torch.float32)
                 for k, c in enumerate(SKIP_CHANNELS)]
        nat.eng._bind()
        nat.eng._call(nat.lib.tcsfm_depthnet_encode_train(nat.dn, N, nat.eng._p(imgs), C.cast(nat.ptrs(skips), C.c_void_p),
                                                          nat.eng._p(tape)))
        ctx.mod, ctx.nat, ctx.N, ctx.stamp = mod, nat, N, nat.stamp
        ctx.save_for_backward(tape)
        return tuple(s.permute(0, 3, 1, 2) for s in skips)

    @staticmethod
    def backward(ctx, *dskips):
        (tape,) = ctx.saved_tensors
        _check_stamp(ctx)
        nat, N, mod = ctx.nat, ctx.N, ctx.mod
        names = mod._enc_names
        want = [(k, i) for i, k in enumerate(names) if ctx.needs_input_grad[2 + i]]
        grads = [None] * len(names)
        if want:
            d = [(_nhwc(g) if g is not None else None) for g in dskips]
            out = [(k, torch.empty(mod._param_shape(k), device=tape.device, dtype=torch.float32)) for k, _ in want]
            nat.grads_call(nat.lib.tcsfm_depthnet_encode_backward, N, (nat.eng._p(tape), C.cast(nat.ptrs(d), C.c_void_p)), out)
            for (k, i), (_, t) in zip(want, out):
                grads[i] = t
        return (None, None, *grads)


class _Decode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, *args):
        skips, params = args[:5], args[5:]
        nat = mod._native_for(skips[0], H=skips[0].shape[2] * 2, W=skips[0].shape[3] * 2)
        N = skips[0].shape[0]
        nh = [_nhwc(s) for s in skips]
        for k, (s, c) in enumerate(zip(nh, SKIP_CHANNELS)):
            shp = (N, nat.eng.H >> (k + 1), nat.eng.W >> (k + 1), c)
            if tuple(s.shape) != shp:
                raise ValueError(f"DepthNetModule: skip {k} of shape {tuple(skips[k].shape)}: expected [N,C,h,w] = {shp[0], shp[3], shp[1], shp[2]}")
        tape = torch.empty(N * nat.tape_per_image[1], device=skips[0].device, dtype=torch.float32)
        disp = torch.empty((N, 1, nat.eng.H, nat.eng.W), device=skips[0].device, dtype=torch.float32)
        nat.eng._bind()
        nat.eng._call(nat.lib.tcsfm_depthnet_decode_train(nat.dn, N, C.cast(nat.ptrs(nh), C.c_void_p), nat.eng._p(disp),
                                                          nat.eng._p(tape)))
        ctx.mod, ctx.nat, ctx.N, ctx.stamp = mod, nat, N, nat.stamp
        ctx.save_for_backward(tape)
        return disp

    @staticmethod
    def backward(ctx, ddisp):
        (tape,) = ctx.saved_tensors
        _check_stamp(ctx)
        nat, N, mod = ctx.nat, ctx.N, ctx.mod
        names = mod._dec_names
        want = [(k, i) for i, k in enumerate(names) if ctx.needs_input_grad[6 + i]]
        dev = tape.device
        dsk = [torch.empty((N, nat.eng.H >> (k + 1), nat.eng.W >> (k + 1), c), device=dev, dtype=torch.float32)
               if ctx.needs_input_grad[1 + k] else None for k, c in enumerate(SKIP_CHANNELS)]
        out = [(k, torch.empty(mod._param_shape(k), device=dev, dtype=torch.float32)) for k, _ in want]
        if want or any(d is not None for d in dsk):
            nat.grads_call(nat.lib.tcsfm_depthnet_decode_backward, N,
                           (nat.eng._p(tape), nat.eng._p(ddisp.float().contiguous()), C.cast(nat.ptrs(dsk), C.c_void_p)), out)
        grads = [None] * len(names)
        for (k, i), (_, t) in zip(want, out):
            grads[i] = t
        return (None, *[(d.permute(0, 3, 1, 2) if d is not None else None) for d in dsk], *grads)


class DepthNetModule(torch.nn.Module):
    """The reference depth_model (ResNet18 encoder + U-Net decoder, num_scales = 1) with nn.Parameters under the reference's names
    (`encoder.encoder.layer1.0.conv1.weight`, `depth_upconvs.0.1.conv.weight`, ...; BatchNorm running statistics are buffers), whose
    forward and backward run on the HIP library.  `params`: a reference depth module, its state_dict, or a dict of numpy arrays;
    `fc.*` and `num_batches_tracked` are ignored.  BatchNorm always uses its running statistics: a forward in training mode
    (module.train()) is refused, and the module starts in evaluation mode.  Gradients reach every parameter that requires them and
    every `skips` input that requires them; images get none (an `x` that requires grad is refused)."""

    def __init__(self, params, max_images: int = 6):
        super().__init__()
        sd = params.state_dict() if hasattr(params, "state_dict") else params
        self.max_images = int(max_images)
        shapes = _shapes()
        for k, shp in shapes.items():
            if k not in sd:
                raise KeyError(f"DepthNetModule: {k}: missing")
            v = sd[k]
            t = (v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(torch.float32).clone()
            if tuple(t.shape) != shp:
                raise ValueError(f"DepthNetModule: {k}: shape {tuple(t.shape)}, expected {shp}")
            *path, leaf = k.split(".")
            m = self
            for p in path:
                if p not in m._modules:
                    m.add_module(p, torch.nn.Module())
                m = m._modules[p]
            if _is_buffer(k):
                m.register_buffer(leaf, t)
            else:
                m.register_parameter(leaf, torch.nn.Parameter(t))
        for k in sd:
            if k.startswith("feature_convs.1.") or k.startswith("predict_disps.1."):
                raise ValueError(f"DepthNetModule: {k}: num_scales > 1 is not supported")
        self._names = list(shapes)
        self._pnames = [k for k in self._names if not _is_buffer(k)]
        self._enc_names = [k for k in self._pnames if k.startswith(_ENC)]
        self._dec_names = [k for k in self._pnames if not k.startswith(_ENC)]
        self._native = {}
        self.eval()

    def _param_shape(self, k):
        return self.get_parameter(k).shape

    def __deepcopy__(self, memo):
        """an independent module: parameters and buffers copied, native state created on first use"""
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_native" else copy.deepcopy(v, memo)
        return new

    def _tensors(self):
        return [(k, self.get_buffer(k) if _is_buffer(k) else self.get_parameter(k)) for k in self._names]

    def _native_for(self, t: torch.Tensor, H=None, W=None):
        """the native state for t's device and image size, re-folded when a parameter's or buffer's version moved"""
        H = int(t.shape[2]) if H is None else int(H)
        W = int(t.shape[3]) if W is None else int(W)
        key = (t.device.index, H, W)
        nat = self._native.get(key)
        if nat is None:
            nat = self._native[key] = _Native(H, W, self.max_images, t.device)
        named = self._tensors()
        stamp = tuple((id(v), int(v._version)) for _, v in named)
        if nat.stamp != stamp:
            for k, v in named:
                if v.device != t.device or v.dtype != torch.float32:
                    raise ValueError(f"DepthNetModule: {k} is a {v.dtype} tensor on {v.device}: move the module to {t.device} (float32)")
            nat.load([(k, v.detach().contiguous()) for k, v in named])
            nat.stamp = stamp
        return nat

    def forward(self, x=None, skips=None, return_disp=True, epoch=0):
        """depth_model(x=None, skips=None, return_disp=True, epoch=0) -> ([disp [N,1,H,W]], skips) or (None, skips)"""
        if self.training:
            raise RuntimeError("DepthNetModule: training-mode BatchNorm (batch statistics) is not supported; call .eval() "
                               "(BatchNorm then uses its running statistics, as the reference's test-time optimisation does)")
        if x is not None and x.requires_grad:
            raise RuntimeError("DepthNetModule: gradients with respect to the images are not supported (x.requires_grad)")
        if x is not None and (x.dim() != 4 or x.shape[1] != 3):
            raise ValueError(f"DepthNetModule: x of shape {tuple(x.shape)}: expected images [N,3,H,W]")
        enc_p = [self.get_parameter(k) for k in self._enc_names]
        dec_p = [self.get_parameter(k) for k in self._dec_names]
        grad_on = torch.is_grad_enabled()
        if x is not None:
            if grad_on and any(p.requires_grad for p in enc_p):
                skips = list(_Encode.apply(self, x, *enc_p))
            else:
                nat = self._native_for(x)
                skips = [s.permute(0, 3, 1, 2) for s in nat.net.encode(x.float())]
            if not return_disp:
                return None, skips
        elif skips is None:
            raise ValueError("DepthNetModule: needs x or skips")
        skips = list(skips)
        if grad_on and (any(p.requires_grad for p in dec_p) or any(s.requires_grad for s in skips)):
            disp = _Decode.apply(self, *skips, *dec_p)
        else:
            nat = self._native_for(skips[0], H=skips[0].shape[2] * 2, W=skips[0].shape[3] * 2)
            disp = nat.net.decode([_nhwc(s) for s in skips])
        return [disp], skips
