"""The reference's depth network (models/depth_w_access.py, num_scales = 1) on the HIP library: the hand-written gfx950 kernels of
csrc/depthnet_kernel.h behind the reference module's call convention, so that DepthOptimizer and helpers.get_disp_for_eigen take a
DepthNetHIP as their depth_model unchanged."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .engine import Engine, _chk

SKIP_CHANNELS = (64, 64, 128, 256, 512)


def read_depth_state_dict(path: str, load_best: bool = True) -> dict:
    """'depth_state_dict' of a reference checkpoint (resolved like posenet.read_pose_state_dict)"""
    import os
    if os.path.isdir(path):
        path = os.path.join(path, "best_model", "best_model.pt") if load_best else os.path.join(path, "checkpoint.pt")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if "depth_state_dict" not in ck:
        raise KeyError(f"{path}: no 'depth_state_dict' entry (keys: {sorted(ck)})")
    return ck["depth_state_dict"]


def is_reference_depthnet(module) -> bool:
    """does `module` carry the parameters of the reference's depth_model (ResNet18 encoder + the U-Net decoder, num_scales = 1)?"""
    try:
        sd = module.state_dict()
    except Exception:
        return False
    need = ["encoder.encoder.conv1.weight", "encoder.encoder.bn1.running_var", "encoder.encoder.layer4.1.conv2.weight",
            "depth_upconvs.0.1.conv.weight", "iconvs.4.0.conv.weight", "feature_convs.0.0.conv.weight", "predict_disps.0.0.conv.weight"]
    return (all(k in sd for k in need) and tuple(sd["encoder.encoder.conv1.weight"].shape) == (64, 3, 7, 7)
            and "feature_convs.1.0.conv.weight" not in sd and tuple(sd["predict_disps.0.0.conv.weight"].shape) == (1, 8, 3, 3))


def named_table(named):
    """the library's by-name tables from [(name, contiguous float32 torch tensor or numpy array)]: (n, names, pointers, shapes [n,4]
    int64, zero-padded), the last three as void pointers that keep their arrays alive"""
    n = len(named)
    names = (C.c_char_p * max(n, 1))(*[k.encode() for k, _ in named])
    ptrs = (C.c_void_p * max(n, 1))(*[a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data for _, a in named])
    shapes = np.zeros((max(n, 1), 4), dtype=np.int64)
    for i, (_, a) in enumerate(named):
        shapes[i, :a.ndim] = a.shape
    return n, C.cast(names, C.c_void_p), C.cast(ptrs, C.c_void_p), shapes.ctypes.data_as(C.c_void_p)


class DepthNetHIP:
    """depth_model.forward on the engine's GPU.  `params`: a reference depth_model (nn.Module) or its state_dict / a dict of numpy
    arrays under the same names.  Calls with more than max_images images run in chunks (an image's result does not depend on the
    other images of a call)."""

    def __init__(self, engine: Engine, max_images: int, params=None):
        self.eng, self.lib = engine, engine.lib
        self.max_images = int(max_images)
        dn = C.c_void_p()
        engine._bind()
        engine._call(self.lib.tcsfm_depthnet_create(engine._h, self.max_images, C.byref(dn)))
        self._dn = dn
        engine._adopt(self, self.lib.tcsfm_depthnet_destroy, dn)
        self.training = False
        if params is not None:
            self.load(params)

    def close(self):
        if getattr(self, "_dn", None):
            self.eng._release(self)         # (a no-op when the engine was closed first: it took the network with it)
            self._dn = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # the nn.Module surface DepthOptimizer uses
    def train(self, mode: bool = True):
        return self

    def eval(self):
        return self

    def load(self, params):
        sd = params.state_dict() if hasattr(params, "state_dict") else params
        named = []
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or k.startswith("fc.") or ".fc." in k:
                continue
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if a.ndim > 4:
                raise ValueError(f"{k}: {a.ndim}-dimensional tensor")
            named.append((k, np.ascontiguousarray(a, dtype=np.float32)))
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_depthnet_load(self._dn, *named_table(named)))
        return self

    def load_checkpoint(self, path: str, load_best: bool = True):
        """the 'depth_state_dict' entry of a reference checkpoint file, or of `<dir>/best_model/best_model.pt` / `<dir>/checkpoint.pt`"""
        return self.load(read_depth_state_dict(path, load_best))

    def split(self, layer: int):
        """tcsfm_debug_depthnet_split: (ks, oh, ow, nb, pb, kw) of convolution `layer` (0 = conv1, evaluation order)"""
        v = [C.c_int() for _ in range(6)]
        self.eng._call(self.lib.tcsfm_debug_depthnet_split(self._dn, int(layer), *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def _skip_shapes(self, N):
        e = self.eng
        return [(N, e.H >> (k + 1), e.W >> (k + 1), c) for k, c in enumerate(SKIP_CHANNELS)]

    def encode(self, imgs: torch.Tensor, flip: bool = False):
        """imgs [N,3,H,W] -> the five skips as NHWC tensors [N,h,w,C]"""
        e = self.eng
        e._bind()
        N = imgs.shape[0]
        imgs = _chk(imgs, (N, 3, e.H, e.W), "imgs")
        skips = [torch.empty(s, device=imgs.device, dtype=torch.float32) for s in self._skip_shapes(N)]
        for i0 in range(0, N, self.max_images):
            i1 = min(N, i0 + self.max_images)
            t = (C.c_void_p * 5)(*[s[i0:i1].data_ptr() for s in skips])
            e._call(self.lib.tcsfm_depthnet_encode(self._dn, i1 - i0, e._p(imgs[i0:i1]), int(bool(flip)), C.cast(t, C.c_void_p)))
        return skips

    def decode(self, skips_nhwc) -> torch.Tensor:
        """five NHWC skips -> disparity [N,1,H,W]"""
        e = self.eng
        e._bind()
        N = skips_nhwc[0].shape[0]
        for s, shp in zip(skips_nhwc, self._skip_shapes(N)):
            if tuple(s.shape) != shp or s.dtype != torch.float32 or not s.is_cuda or not s.is_contiguous():
                raise ValueError(f"skip of shape {tuple(s.shape)}: expected a contiguous float32 CUDA tensor {shp}")
        disp = torch.empty((N, 1, e.H, e.W), device=skips_nhwc[0].device, dtype=torch.float32)
        for i0 in range(0, N, self.max_images):
            i1 = min(N, i0 + self.max_images)
            t = (C.c_void_p * 5)(*[s[i0:i1].data_ptr() for s in skips_nhwc])
            e._call(self.lib.tcsfm_depthnet_decode(self._dn, i1 - i0, C.cast(t, C.c_void_p), e._p(disp[i0:i1])))
        return disp

    def forward(self, imgs: torch.Tensor, flip: bool = False) -> torch.Tensor:
        """encode + decode without exposing the skips: imgs [N,3,H,W] -> disparity [N,1,H,W]"""
        e = self.eng
        e._bind()
        N = imgs.shape[0]
        imgs = _chk(imgs, (N, 3, e.H, e.W), "imgs")
        disp = torch.empty((N, 1, e.H, e.W), device=imgs.device, dtype=torch.float32)
        for i0 in range(0, N, self.max_images):
            i1 = min(N, i0 + self.max_images)
            e._call(self.lib.tcsfm_depthnet_forward(self._dn, i1 - i0, e._p(imgs[i0:i1]), int(bool(flip)), e._p(disp[i0:i1])))
        return disp

    def disp_for_eigen(self, imgs: torch.Tensor, min_depth: Optional[float] = None, max_depth: Optional[float] = None) -> torch.Tensor:
        """tcsfm_depthnet_disp_for_eigen: helpers.get_disp_for_eigen on the device -- the network on the frames and on their mirror
        images, disp_to_depth's scaled_disp of both (min_depth / max_depth: default_opts' when None), the second un-flipped, blended by
        batch_post_process_disparity in float64 with NumPy's bits: imgs [N,3,H,W] float32 CUDA -> float64 [N,H,W]"""
        from .engine import default_opts
        e = self.eng
        e._bind()
        N = int(imgs.shape[0])
        imgs = _chk(imgs, (N, 3, e.H, e.W), "imgs")
        o = default_opts(**{k: float(v) for k, v in (("min_depth", min_depth), ("max_depth", max_depth)) if v is not None})
        out = torch.empty((N, e.H, e.W), device=imgs.device, dtype=torch.float64)
        e._call(self.lib.tcsfm_depthnet_disp_for_eigen(self._dn, C.byref(o), N, e._p(imgs), e._p(out)))
        return out

    @staticmethod
    def _to_nhwc(s: torch.Tensor) -> torch.Tensor:
        """[N,C,h,w] -> the NHWC buffer: the tensor behind a view this class returned, else an NHWC-contiguous copy"""
        t = s.permute(0, 2, 3, 1)
        return t if t.is_contiguous() and t.dtype == torch.float32 else t.float().contiguous()

    def __call__(self, x: Optional[torch.Tensor] = None, skips=None, return_disp: bool = True, epoch: int = 0):
        """depth_model(x=None, skips=None, return_disp=True, epoch=0) -> ([disp [N,1,H,W]], skips) or (None, skips); skips are [N,C,h,w]
        views of NHWC buffers"""
        if x is not None:
            nhwc = self.encode(x.float())
            views = [s.permute(0, 3, 1, 2) for s in nhwc]
            if not return_disp:
                return None, views
        elif skips is not None:
            views = list(skips)
            nhwc = [self._to_nhwc(s) for s in views]
        else:
            raise ValueError("DepthNetHIP: needs x or skips")
        return [self.decode(nhwc)], views


_NETS = {}     # id(module) -> (parameter / buffer version stamp, engine, DepthNetHIP)


def library_depthnet(depth_model, eng: Engine, n_images: int) -> Optional[DepthNetHIP]:
    """a DepthNetHIP holding `depth_model`'s parameters on `eng` (created once per module and engine, reloaded when a parameter's or
    buffer's version counter moves), or None when the module is not the reference architecture or does not live on the GPU"""
    if not isinstance(depth_model, torch.nn.Module) or not is_reference_depthnet(depth_model):
        return None
    tensors = list(depth_model.parameters()) + list(depth_model.buffers())
    if any(t.device.type != "cuda" for t in tensors):
        return None
    stamp = tuple(int(t._version) for t in tensors)
    hit = _NETS.get(id(depth_model))
    if hit is None or hit[1] is not eng or hit[2].max_images < n_images:
        hit = (stamp, eng, DepthNetHIP(eng, max(int(n_images), 6), depth_model))
    elif hit[0] != stamp:
        hit[2].load(depth_model)
        hit = (stamp, eng, hit[2])
    _NETS[id(depth_model)] = hit
    return hit[2]
