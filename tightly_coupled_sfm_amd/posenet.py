"""PoseNet (models/pose_models.py:88-147) on the HIP library: the hand-written gfx950 convolution stack of
csrc/posenet_kernel.h behind the reference module's call convention, and the coupled loop of train_mono.py:41-81 kept inside
the library (tcsfm_solve_pose_iteratively)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .engine import Engine, _chk

_CONV = ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7"]
_CHANS, _KSZ = [6, 16, 32, 64, 128, 256, 256, 256], [7, 5, 3, 3, 3, 3, 3]
PARAM_SHAPES_W = [(_CHANS[l + 1], _CHANS[l], _KSZ[l], _KSZ[l]) for l in range(7)]
# the reference pose_model's parameters in module order: name -> shape
PARAM_SHAPES = {}
for _l, _c in enumerate(_CONV):
    PARAM_SHAPES[f"{_c}.0.weight"] = PARAM_SHAPES_W[_l]
    for _k in ("0.bias", "1.weight", "1.bias"):
        PARAM_SHAPES[f"{_c}.{_k}"] = (_CHANS[_l + 1],)
PARAM_SHAPES["pose_pred.weight"] = (6, 256, 1, 1)
PARAM_SHAPES["pose_pred.bias"] = (6,)
PARAM_NAMES = tuple(PARAM_SHAPES)


def read_pose_state_dict(path: str, load_best: bool = True) -> dict:
    """'pose_state_dict' of a reference checkpoint (utils/learning_helpers.py:29-37 resolves the file the same way)"""
    import os
    if os.path.isdir(path):
        path = os.path.join(path, "best_model", "best_model.pt") if load_best else os.path.join(path, "checkpoint.pt")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if "pose_state_dict" not in ck:
        raise KeyError(f"{path}: no 'pose_state_dict' entry (keys: {sorted(ck)})")
    return ck["pose_state_dict"]


def is_reference_posenet(module) -> bool:
    """does `module` carry the parameters of the reference's pose_model (conv1..conv7 = (conv2d_wn, GroupNorm, ReLU), pose_pred)?"""
    try:
        sd = module.state_dict()
    except Exception:
        return False
    need = [f"{c}.0.weight" for c in _CONV] + [f"{c}.1.weight" for c in _CONV] + ["pose_pred.weight", "pose_pred.bias"]
    return all(k in sd for k in need) and tuple(sd["conv1.0.weight"].shape) == (16, 6, 7, 7) and tuple(sd["pose_pred.weight"].shape[:2]) == (6, 256)


class _PoseNetInputGrad(torch.autograd.Function):
    """PoseNetHIP.__call__ under autograd: tcsfm_posenet_forward_train / tcsfm_posenet_backward.  Differentiable with respect to the
    images only: the weights are the library's frozen copy (the reference's default tuning mode, optimize_depth_encoder)."""

    @staticmethod
    def forward(ctx, net, imgs):
        pose, tape = net.forward_train(imgs)
        ctx.net, ctx.stamp = net, net._stamp
        ctx.save_for_backward(tape)
        ctx.set_materialize_grads(False)
        return pose

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pose):
        if g_pose is None:
            return None, None
        ctx.net._check_stamp(ctx.stamp)
        tape, = ctx.saved_tensors
        return None, ctx.net.backward(tape, g_pose.contiguous())


class PoseNetHIP:
    """pose_model.forward on the engine's GPU.  `params`: a reference pose_model (nn.Module) or its state_dict / a dict of
    numpy arrays under the same names.

    Under autograd (grad enabled and ``imgs.requires_grad``) the pose carries a grad_fn: the gradient with respect to the IMAGES
    (csrc/posenet_grad_kernel.h).  Through __call__ the parameters get no gradient -- they are the library's frozen copy, as in the
    reference's default test-time tuning mode.  Tuning the pose network's weights (the reference's optimize_pose_weights_all) goes
    through `param_backward` (csrc/posenet_wgrad_kernel.h: every parameter's gradient from the same tape) and `load_device` (a
    stream-ordered reload from device tensors); posenet_train.PoseNetModule wraps both as a torch.nn.Module."""

    _stamp = 0               # counts load() calls: a backward refuses a tape made with other weights

    def __init__(self, engine: Engine, max_images: int, params=None):
        self.eng, self.lib = engine, engine.lib
        self.max_images = int(max_images)
        pn = C.c_void_p()
        engine._call(self.lib.tcsfm_posenet_create(engine._h, self.max_images, C.byref(pn)))
        self._pn = pn
        engine._adopt(self, self.lib.tcsfm_posenet_destroy, pn)
        if params is not None:
            self.load(params)

    def close(self):
        if getattr(self, "_pn", None):
            self.eng._release(self)         # (a no-op when the engine was closed first: it took the network with it)
            self._pn = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, params):
        sd = params.state_dict() if hasattr(params, "state_dict") else params
        arr = lambda k: None if k not in sd else np.ascontiguousarray(
            (sd[k].detach().cpu().numpy() if isinstance(sd[k], torch.Tensor) else np.asarray(sd[k])), dtype=np.float32)
        keep = []
        def table(suffix):
            t = (C.c_void_p * 7)()
            for i, c in enumerate(_CONV):
                a = arr(f"{c}.{suffix}")
                keep.append(a)
                t[i] = None if a is None else a.ctypes.data
            return t
        cw, cb, gw, gb = table("0.weight"), table("0.bias"), table("1.weight"), table("1.bias")
        hw, hb = arr("pose_pred.weight").reshape(6, 256).copy(), arr("pose_pred.bias")
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_posenet_load(self._pn, cw, cb, gw, gb, hw.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p)))
        self._stamp += 1
        return self

    def load_device(self, named):
        """tcsfm_posenet_load_device: `named` maps the reference's parameter names to contiguous float32 tensors on the engine's
        device (conv{l}.0.bias and conv{l}.1.weight / .bias may be absent: 0, 1, 0).  Asynchronous, no host copy; same prepared
        weights as load() of the same values."""
        e = self.eng
        keep = []

        def one(k, shape, required):
            if k not in named or named[k] is None:
                if required:
                    raise KeyError(f"PoseNetHIP.load_device: {k}: missing")
                return None
            t = named[k].detach()
            if t.dim() == 4 and len(shape) == 2:
                t = t.reshape(shape)
            t = _chk(t, shape, k)
            keep.append(t)
            return e._p(t).value

        def table(suffix, shapes, required=False):
            return (C.c_void_p * 7)(*[one(f"{c}.{suffix}", shp, required) for c, shp in zip(_CONV, shapes)])
        cw = table("0.weight", PARAM_SHAPES_W, True)
        vec = [(sh[0],) for sh in PARAM_SHAPES_W]
        cb, gw, gb = table("0.bias", vec), table("1.weight", vec), table("1.bias", vec)
        hw, hb = one("pose_pred.weight", (6, 256), True), one("pose_pred.bias", (6,), True)
        e._bind()
        e._call(self.lib.tcsfm_posenet_load_device(self._pn, cw, cb, gw, gb, C.c_void_p(hw), C.c_void_p(hb)))
        self._stamp += 1
        return self

    def param_backward(self, imgs, tape, d_pose, want=None, need_d_imgs=True):
        """tcsfm_posenet_param_backward: the images and the tape of forward_train and the pose's cotangent [N,6] ->
        (d_imgs [N,6,H,W] or None, {name: gradient}) with the current weights.  `want`: the parameter names whose gradient is
        computed (None: all 30; names as in the reference, gradients in the parameters' own shapes, pose_pred.weight [6,256,1,1]).
        The work of everything not asked for is skipped."""
        e = self.eng
        e._bind()
        N = d_pose.shape[0]
        d_pose = _chk(d_pose, (N, 6), "d_pose")
        tape = _chk(tape, (self.tape_size(N),), "tape")
        want = list(PARAM_NAMES) if want is None else list(want)
        bad = [k for k in want if k not in PARAM_SHAPES]
        if bad:
            raise KeyError(f"PoseNetHIP.param_backward: unknown parameter names {bad}")
        if "conv1.0.weight" in want:
            if imgs is None:
                raise ValueError("PoseNetHIP.param_backward: conv1.0.weight's gradient needs the images of the forward")
            imgs = _chk(imgs.detach(), (N, 6, e.H, e.W), "imgs")
        else:
            imgs = None
        dev = d_pose.device
        grads = {k: torch.empty(PARAM_SHAPES[k], device=dev, dtype=torch.float32) for k in want}
        table = lambda suffix: (C.c_void_p * 7)(*[(grads[f"{c}.{suffix}"].data_ptr() if f"{c}.{suffix}" in grads else None) for c in _CONV])
        opt = lambda k: C.c_void_p(grads[k].data_ptr()) if k in grads else None
        d_imgs = torch.empty((N, 6, e.H, e.W), device=dev, dtype=torch.float32) if need_d_imgs else None
        e._call(self.lib.tcsfm_posenet_param_backward(self._pn, N, None if imgs is None else e._p(imgs), e._p(tape), e._p(d_pose),
                                                      None if d_imgs is None else e._p(d_imgs), table("0.weight"), table("0.bias"),
                                                      table("1.weight"), table("1.bias"), opt("pose_pred.weight"), opt("pose_pred.bias")))
        return d_imgs, grads

    def _check_stamp(self, stamp):
        if stamp != self._stamp:
            raise RuntimeError("PoseNetHIP: the weights were loaded again between this forward and its backward: the tape belongs "
                               "to the earlier weights (run the forward again)")

    def load_checkpoint(self, path: str, load_best: bool = True):
        """The reference's checkpoint files (utils/learning_helpers.py:20-48: `torch.save` of a dict whose 'pose_state_dict' entry is
        the PoseNet's state_dict; `<dir>/best_model/best_model.pt` or `<dir>/checkpoint.pt`).  `path` is such a file or the directory."""
        self.load(read_pose_state_dict(path, load_best))

    def __call__(self, imgs: torch.Tensor) -> torch.Tensor:
        """pose_model(imgs): imgs [N,6,H,W] -> [N,6]; with a grad_fn (towards imgs only) when grad is enabled and imgs requires grad"""
        e = self.eng
        e._bind()
        N = imgs.shape[0]
        imgs = _chk(imgs, (N, 6, e.H, e.W), "imgs")
        if torch.is_grad_enabled() and imgs.requires_grad:
            return _PoseNetInputGrad.apply(self, imgs)
        out = torch.empty((N, 6), device=imgs.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_posenet_forward(self._pn, N, e._p(imgs), e._p(out)))
        return out

    def tape_size(self, N: int) -> int:
        n = C.c_int64(0)
        self.eng._call(self.lib.tcsfm_posenet_tape_size(self._pn, int(N), C.byref(n)))
        return int(n.value)

    def forward_train(self, imgs: torch.Tensor):
        """tcsfm_posenet_forward_train: imgs [N,6,H,W] -> (pose [N,6] with the bits of __call__, tape) -- the tape (a flat float32
        tensor, layout in include/tcsfm.h) is what backward needs; the images themselves are not kept"""
        e = self.eng
        e._bind()
        N = imgs.shape[0]
        imgs = _chk(imgs.detach(), (N, 6, e.H, e.W), "imgs")
        pose = torch.empty((N, 6), device=imgs.device, dtype=torch.float32)
        tape = torch.empty((self.tape_size(N),), device=imgs.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_posenet_forward_train(self._pn, N, e._p(imgs), e._p(pose), e._p(tape)))
        return pose, tape

    def backward(self, tape: torch.Tensor, d_pose: torch.Tensor) -> torch.Tensor:
        """tcsfm_posenet_backward: the tape of forward_train and the pose's cotangent [N,6] -> d_imgs [N,6,H,W], with the current weights"""
        e = self.eng
        e._bind()
        N = d_pose.shape[0]
        d_pose = _chk(d_pose, (N, 6), "d_pose")
        tape = _chk(tape, (self.tape_size(N),), "tape")
        d_imgs = torch.empty((N, 6, e.H, e.W), device=d_pose.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_posenet_backward(self._pn, N, e._p(tape), e._p(d_pose), e._p(d_imgs)))
        return d_imgs

    def tape_layer(self, tape: torch.Tensor, layer: int, N: int):
        """tcsfm_debug_posenet_tape_layer: layer 1..7 of a tape -> (raw [N,cout,oh,ow], scsh [N,cout,2], mean_rstd [N,16,2],
        act [N,cout,oh,ow]); act > 0 are the ReLU decisions backward takes"""
        e = self.eng
        e._bind()
        oh, ow = self.split(layer, N)[:2]
        cout = [16, 32, 64, 128, 256, 256, 256][int(layer) - 1]
        tape = _chk(tape, (self.tape_size(N),), "tape")
        raw = torch.empty((int(N), oh, ow, cout), device=tape.device, dtype=torch.float32)
        act = torch.empty_like(raw)
        scsh = torch.empty((int(N), cout, 2), device=tape.device, dtype=torch.float32)
        mr = torch.empty((int(N), 16, 2), device=tape.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_debug_posenet_tape_layer(self._pn, int(N), e._p(tape), int(layer), e._p(raw), e._p(scsh), e._p(mr), e._p(act)))
        return raw.permute(0, 3, 1, 2), scsh, mr, act.permute(0, 3, 1, 2)

    def split(self, layer: int, N: int):
        """tcsfm_debug_posenet_split: (oh, ow, nb, ks, pb) of layer 1..7 in a call over N images"""
        v = [C.c_int(0) for _ in range(5)]
        self.eng._call(self.lib.tcsfm_debug_posenet_split(self._pn, int(layer), int(N), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def layer(self, layer: int, N: int):
        """tcsfm_debug_posenet_layer: layer 1..7 of the most recent evaluation -> (raw convolution output [N,cout,oh,ow],
        GroupNorm (scale, shift) [N,cout,2]); the layer's activation is relu(raw * scale + shift)"""
        e = self.eng
        e._bind()
        oh, ow = self.split(layer, N)[:2]
        cout = [16, 32, 64, 128, 256, 256, 256][int(layer) - 1]
        raw = torch.empty((int(N), oh, ow, cout), device=e.dev, dtype=torch.float32)
        scsh = torch.empty((int(N), cout, 2), device=raw.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_debug_posenet_layer(self._pn, int(layer), int(N), e._p(raw), e._p(scsh)))
        return raw.permute(0, 3, 1, 2), scsh

    def odometry_sequence(self, frames, depths, K, opts=None, sources: int = 1, iterations: int = 4, ring: int = 0, windows_per_call: int = 0,
                          target_pos: int = 0, source_size=None, cam_height=None, disparity=None):
        """tcsfm_odometry_sequence: for every window of a sequence (frames [T,3,H,W] float32, or uint8 [T,3,H,W] / [T,H,W,3] / depths [T,1,H,W] CPU tensors, pinned for
        asynchronous copies; K [3,3]) the coupled PoseNet loop gives the initial poses and the engine refines them, windows
        running on the engine's lanes -> (initial poses, refined poses), each [T-S, 2S, 6] CPU tensors.  depths=None: the depth
        network of Engine.attach_depthnet computes them inside the call (frames in, poses out).  source_size=(h, w): `frames` are
        camera-size bytes, uint8 [T,h,w,3] or [T,3,h,w], resized on the device (Engine.refine_sequence).  cam_height=h: every frame's
        DNet scale from the ring's own depth plane (tcsfm_sequence_scale); fetch them with Engine.sequence_scales().  disparity="plain" /
        "post" (depths=None only): every frame's disparity is kept inside the call (tcsfm_sequence_disparity); fetch them with
        Engine.sequence_disparities()"""
        from .engine import check_cam_height, check_disparity
        cam_height = check_cam_height(cam_height)
        disp_mode = check_disparity(disparity)
        e = self.eng
        T, S = int(frames.shape[0]), int(sources)
        depths = e._seq_depths(depths, T)
        frames, fmt = e._seq_frames(frames, T, source_size)
        e._bind()
        from .engine import default_opts
        o = opts or default_opts()
        Kc = e._cpu(torch.as_tensor(np.asarray(K, dtype=np.float32)), (3, 3), "K")
        init = torch.empty((T - S, 2 * S, 6), dtype=torch.float32); out = torch.empty_like(init)
        hp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with e._frame_format(fmt), e._frame_source(source_size), e._cam_height(cam_height, T), e._disparity(disp_mode, T):
            e._call(self.lib.tcsfm_odometry_sequence(e._h, self._pn, int(iterations), C.byref(o), T, S, hp(frames), hp(depths), hp(Kc), hp(init), hp(out),
                                                     None, int(ring), int(windows_per_call), int(target_pos)))
        return init, out

    def solve_pose_iteratively(self, num_iter: int, tgt, srcs, depth_t, depth_s, K):
        """the coupled loop of train_mono.py:41-81 for a window (layouts of Engine.refine_window) -> (poses [2SB,6], stacked [2SB,num_iter,6])"""
        e = self.eng
        e._bind()
        if isinstance(srcs, (list, tuple)):
            srcs = torch.stack(list(srcs), 0)
        if isinstance(depth_s, (list, tuple)):
            depth_s = torch.stack(list(depth_s), 0)
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        tgt = _chk(tgt, (B, 3, e.H, e.W), "tgt"); srcs = _chk(srcs, (S, B, 3, e.H, e.W), "srcs")
        depth_t = _chk(depth_t, (B, 1, e.H, e.W), "depth_t"); depth_s = _chk(depth_s, (S, B, 1, e.H, e.W), "depth_s")
        K = _chk(K, (B, 3, 3), "K")
        N = 2 * S * B
        poses = torch.empty((N, 6), device=tgt.device, dtype=torch.float32)
        stacked = torch.empty((N, int(num_iter), 6), device=tgt.device, dtype=torch.float32)
        e._call(self.lib.tcsfm_solve_pose_iteratively(e._h, self._pn, int(num_iter), B, S, e._p(tgt), e._p(srcs), e._p(depth_t), e._p(depth_s),
                                                      e._p(K), e._p(poses), e._p(stacked)))
        return poses, stacked
