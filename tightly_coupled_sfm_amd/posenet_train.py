"""The reference's pose network as a differentiable torch.nn.Module on the HIP library: forward, input gradient and parameter
gradients run on the gfx950 kernels of csrc/posenet_kernel.h, csrc/posenet_grad_kernel.h and csrc/posenet_wgrad_kernel.h
(tcsfm_posenet_forward_train / tcsfm_posenet_param_backward), so the reference's optimize_pose_weights_all tuning mode
(optimization_experiments/optimizer.py:187-189: deep-copy, `pose_model.parameters()` into Adam, `loss.backward()` through
solve_pose_iteratively) runs on them unchanged."""
from __future__ import annotations

import copy

import numpy as np
import torch

from .posenet import PARAM_NAMES, PARAM_SHAPES, PoseNetHIP


class _Native:
    """the library state behind one module on one device and image size: an engine and a PoseNetHIP fed by
    tcsfm_posenet_load_device, and the version stamp of the parameters it holds"""

    def __init__(self, H, W, max_images, device):
        from .engine import Engine
        with torch.cuda.device(device):
            self.eng = Engine(H, W, max_images, device=device.index)
        self.net = PoseNetHIP(self.eng, max_images)
        self.max_images = max_images
        self.stamp = None


def _check_stamp(ctx):
    """the backward reads the instance's current weights: refuse if a later forward loaded different parameters into it"""
    if ctx.nat.stamp != ctx.stamp:
        raise RuntimeError("PoseNetModule: a parameter changed in place and another forward ran before this graph's backward; "
                           "the backward would use the new weights.  Run backward before updating the parameters.")


class _Forward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, imgs, *params):
        nat = mod._native_for(imgs)
        x = imgs.detach().contiguous()
        pose, tape = nat.net.forward_train(x)
        ctx.mod, ctx.nat, ctx.stamp = mod, nat, nat.stamp
        ctx.save_for_backward(x, tape)
        ctx.set_materialize_grads(False)
        return pose

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pose):
        n = len(PARAM_NAMES)
        if g_pose is None:
            return (None, None) + (None,) * n
        _check_stamp(ctx)
        x, tape = ctx.saved_tensors
        want = [k for i, k in enumerate(PARAM_NAMES) if ctx.needs_input_grad[2 + i]]
        need_x = bool(ctx.needs_input_grad[1])
        if not want and not need_x:
            return (None, None) + (None,) * n
        d_imgs, grads = ctx.nat.net.param_backward(x, tape, g_pose.contiguous(), want=want, need_d_imgs=need_x)
        return (None, d_imgs) + tuple(grads.get(k) for k in PARAM_NAMES)


class PoseNetModule(torch.nn.Module):
    """The reference pose_model (models/pose_models.py:88-147) with nn.Parameters under the reference's names (`conv1.0.weight`,
    `conv1.0.bias`, `conv1.1.weight`, `conv1.1.bias`, ..., `pose_pred.weight` [6,256,1,1], `pose_pred.bias`), whose forward and
    backward run on the HIP library.  `params`: a reference pose module, its state_dict, or a dict of numpy arrays (absent
    convolution biases / GroupNorm affine parameters start at 0 / 1, 0).  Gradients reach every parameter that requires them and
    the images when they require them.  `return_features=True` is not supported."""

    def __init__(self, params, max_images: int = 8):
        super().__init__()
        sd = params.state_dict() if hasattr(params, "state_dict") else params
        self.max_images = int(max_images)
        for k, shp in PARAM_SHAPES.items():
            if k in sd:
                v = sd[k]
                t = (v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(torch.float32).clone()
                if k == "pose_pred.weight" and tuple(t.shape) == (6, 256):
                    t = t.reshape(shp)
            elif k.endswith(".0.weight") or k.startswith("pose_pred"):
                raise KeyError(f"PoseNetModule: {k}: missing")
            else:
                t = torch.ones(shp) if k.endswith(".1.weight") else torch.zeros(shp)
            if tuple(t.shape) != shp:
                raise ValueError(f"PoseNetModule: {k}: shape {tuple(t.shape)}, expected {shp}")
            *path, leaf = k.split(".")
            m = self
            for p in path:
                if p not in m._modules:
                    m.add_module(p, torch.nn.Module())
                m = m._modules[p]
            m.register_parameter(leaf, torch.nn.Parameter(t))
        self._native = {}

    def __deepcopy__(self, memo):
        """an independent module: parameters copied, native state created on first use"""
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_native" else copy.deepcopy(v, memo)
        return new

    def _tensors(self):
        return [(k, self.get_parameter(k)) for k in PARAM_NAMES]

    def _native_for(self, imgs: torch.Tensor, n_images: int = 0):
        """the native state for the images' device and size (and at least n_images images), reloaded when a parameter's version moved"""
        if imgs.dim() != 4 or not imgs.is_cuda:
            raise ValueError(f"PoseNetModule: images of shape {tuple(imgs.shape)} on {imgs.device}: expected [N,C,H,W] on the GPU")
        H, W, N = int(imgs.shape[2]), int(imgs.shape[3]), max(int(imgs.shape[0]), int(n_images))
        key = (imgs.device.index, H, W)
        nat = self._native.get(key)
        if nat is None or nat.max_images < N:
            nat = self._native[key] = _Native(H, W, max(N, self.max_images), imgs.device)
        named = self._tensors()
        stamp = tuple((id(v), int(v._version)) for _, v in named)
        if nat.stamp != stamp:
            for k, v in named:
                if v.device != imgs.device or v.dtype != torch.float32:
                    raise ValueError(f"PoseNetModule: {k} is a {v.dtype} tensor on {v.device}: move the module to {imgs.device} (float32)")
            nat.net.load_device({k: v.detach().contiguous() for k, v in named})
            nat.stamp = stamp
        return nat

    def forward(self, imgs, return_features=False):
        """pose_model(imgs): imgs [N,6,H,W] -> pose [N,6]"""
        if return_features:
            raise NotImplementedError("PoseNetModule: return_features=True is not supported")
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or imgs.shape[1] != 6:
            raise ValueError(f"PoseNetModule: imgs of shape {tuple(getattr(imgs, 'shape', ()))}: expected images [N,6,H,W]")
        if imgs.dtype != torch.float32:
            raise TypeError(f"PoseNetModule: imgs must be float32 (got {imgs.dtype})")
        params = [p for _, p in self._tensors()]
        if torch.is_grad_enabled() and (imgs.requires_grad or any(p.requires_grad for p in params)):
            return _Forward.apply(self, imgs, *params)
        return self._native_for(imgs).net(imgs.detach())
