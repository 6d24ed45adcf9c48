"""Host-side engine: torch tensors (device memory, streams) over the C ABI of libtcsfm_hip.so.

PyTorch is plumbing here -- it owns device buffers and the current stream; every computation happens
in the HIP library.  All array arguments are passed as raw device pointers (``tensor.data_ptr()``).

Naming follows the reference: a *pair* is a directed (target, source) frame pair; poses are the
reference's 6-vectors ``[tx,ty,tz,rx,ry,rz]`` (models/stn.py:143-158).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import Opts, default_opts  # noqa: F401


def check_cam_height(cam_height) -> Optional[float]:
    """the `cam_height` keyword of the sequence methods (tcsfm_sequence_scale): None (the stage stays off) or a positive finite number,
    checked before anything touches the GPU -> float or None"""
    if cam_height is None:
        return None
    if isinstance(cam_height, bool) or not isinstance(cam_height, (int, float, np.integer, np.floating)):
        raise TypeError(f"cam_height must be a number or None (got {type(cam_height).__name__})")
    v = float(cam_height)
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f"cam_height must be positive and finite (got {v})")
    return v


DISPARITY_MODES = {None: _lib.SEQ_DISP_OFF, "plain": _lib.SEQ_DISP_PLAIN, "post": _lib.SEQ_DISP_POST}


def check_disparity(disparity) -> int:
    """the `disparity` keyword of the sequence methods (tcsfm_sequence_disparity): None (the stage stays off), "plain" or "post" -> the
    mode, checked before anything touches the GPU"""
    if disparity is not None and not isinstance(disparity, str):
        raise TypeError(f"disparity must be None, 'plain' or 'post' (got {type(disparity).__name__})")
    if disparity not in DISPARITY_MODES:
        raise ValueError(f"disparity must be None, 'plain' or 'post' (got {disparity!r})")
    return DISPARITY_MODES[disparity]


def _chk(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device})")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if tuple(t.shape) != tuple(shape):
        # same wording as the reference's check_sizes (models/stn.py:24-30)
        raise AssertionError("wrong size for {}, expected {}, got  {}".format(name, "x".join(map(str, shape)), list(t.shape)))
    return t.contiguous()


def frame_format(frames: torch.Tensor, H: int, W: int) -> int:
    """How a sequence call reads the CPU tensor `frames` (tcsfm_sequence_frame_format): _lib.FRAMES_F32_CHW for float32 (its shape is
    checked where it always was), FRAMES_U8_CHW for uint8 [T,3,H,W], FRAMES_U8_HWC for uint8 [T,H,W,3] -- H, W >= 4, so the two cannot
    be confused.  Anything else is a TypeError.  Pure: touches neither the library nor the GPU."""
    if not isinstance(frames, torch.Tensor) or frames.device.type != "cpu":
        raise TypeError("frames must be a CPU tensor (pinned for asynchronous copies): float32 [T,3,H,W], or uint8 [T,3,H,W] / [T,H,W,3]")
    if frames.dtype == torch.float32:
        return _lib.FRAMES_F32_CHW
    if frames.dtype != torch.uint8:
        raise TypeError(f"frames must be float32 or uint8 (got {frames.dtype})")
    shape = tuple(frames.shape)
    if len(shape) == 4 and shape[1:] == (3, H, W):
        return _lib.FRAMES_U8_CHW
    if len(shape) == 4 and shape[1:] == (H, W, 3):
        return _lib.FRAMES_U8_HWC
    raise TypeError(f"uint8 frames must be [T,3,{H},{W}] or [T,{H},{W},3] (got {list(shape)})")


def source_frame_format(frames: torch.Tensor, source_size) -> int:
    """frame_format for camera-size frames (tcsfm_sequence_frame_source): `frames` must be a uint8 CPU tensor [T,h,w,3] (FRAMES_U8_HWC) or
    [T,3,h,w] (FRAMES_U8_CHW) with (h, w) = source_size -- given explicitly, never guessed from the tensor.  (A 3 x 3 source fits both:
    it is read as interleaved.)  Pure."""
    try:
        h, w = (int(v) for v in source_size)
    except (TypeError, ValueError):
        raise TypeError("source_size must be a pair (h, w)") from None
    if h <= 0 or w <= 0:
        raise ValueError(f"source_size must be positive (got {(h, w)})")
    if not isinstance(frames, torch.Tensor) or frames.device.type != "cpu" or frames.dtype != torch.uint8:
        raise TypeError("with source_size, frames must be a uint8 CPU tensor [T,h,w,3] or [T,3,h,w] (float frames are already at the engine's size)")
    shape = tuple(frames.shape)
    if len(shape) == 4 and shape[1:] == (h, w, 3):
        return _lib.FRAMES_U8_HWC
    if len(shape) == 4 and shape[1:] == (3, h, w):
        return _lib.FRAMES_U8_CHW
    raise TypeError(f"uint8 frames of source_size {(h, w)} must be [T,{h},{w},3] or [T,3,{h},{w}] (got {list(shape)})")


def _copy_opts(o: Opts) -> Opts:
    c = Opts()
    C.memmove(C.byref(c), C.byref(o), C.sizeof(Opts))
    return c


class _PhotometricError(torch.autograd.Function):
    """Engine.compute_photometric_error under autograd: the same forward call, tcsfm_photometric_backward behind it
    (Engine.compute_photometric_error_backward).  diff_img, weight_mask and img_rec are differentiable; every mask is not."""

    @staticmethod
    def forward(ctx, engine, opts, t, s, dt, ds, p, K):
        diff, valid, weight, ae, am, rec = engine._photometric(t, s, dt, ds, p, K, opts)
        ctx.engine, ctx.opts = engine, _copy_opts(opts)
        ctx.save_for_backward(t, s, dt, ds, p, K)
        valid_mask = am * valid
        ctx.mark_non_differentiable(valid, ae, am, valid_mask)
        ctx.set_materialize_grads(False)        # a cotangent autograd does not supply stays None: its path launches nothing
        return diff, rec, weight, valid, ae, am, valid_mask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_diff, g_rec, g_weight, *_masks):
        t, s, dt, ds, p, K = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[4:7])
        d_dt, d_ds, d_p = ctx.engine.compute_photometric_error_backward(t, s, dt, ds, p, K, g_diff, g_weight, g_rec, want, ctx.opts)
        return None, None, None, None, d_dt, d_ds, d_p, None


def _cot(g):
    return None if g is None else g.contiguous()


class _DispToDepth(torch.autograd.Function):
    """Engine.disp_to_depth under autograd: the same forward kernel, tcsfm_disp_to_depth_backward behind it."""

    @staticmethod
    def forward(ctx, engine, d, min_depth, max_depth):
        ctx.engine, ctx.range = engine, (min_depth, max_depth)
        ctx.save_for_backward(d)
        ctx.set_materialize_grads(False)        # a cotangent autograd does not supply stays None: its path costs nothing
        return engine._disp_to_depth(d, min_depth, max_depth)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_scaled, g_depth):
        if g_scaled is None and g_depth is None:
            return None, None, None, None
        d, = ctx.saved_tensors
        return None, ctx.engine.disp_to_depth_backward(d, *ctx.range, _cot(g_scaled), _cot(g_depth)), None, None


class _SSIMLoss(torch.autograd.Function):
    """Engine.ssim_loss under autograd: the same forward kernel, tcsfm_ssim_backward behind it."""

    @staticmethod
    def forward(ctx, engine, x, y):
        ctx.engine = engine
        ctx.save_for_backward(x, y)
        ctx.set_materialize_grads(False)
        return engine._ssim(x, y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        if g_out is None:
            return None, None, None
        x, y = ctx.saved_tensors
        g_x, g_y = ctx.engine.ssim_loss_backward(x, y, _cot(g_out), tuple(ctx.needs_input_grad[1:3]))
        return None, g_x, g_y


class _SmoothLoss(torch.autograd.Function):
    """losses.get_smooth_loss under autograd: tcsfm_smooth_loss_device forward (the scalar stays on the device),
    tcsfm_smooth_loss_backward behind it.  img takes no gradient."""

    @staticmethod
    def forward(ctx, engine, disp, img):
        loss, stats = engine.smooth_loss_device(disp, img)
        ctx.engine = engine
        ctx.save_for_backward(disp, img, stats)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        if g_loss is None:
            return None, None, None
        disp, img, stats = ctx.saved_tensors
        return None, ctx.engine.smooth_loss_backward(disp, img, stats, _cot(g_loss)), None


class _WindowLoss(torch.autograd.Function):
    """The window loss of optimizer.py:47-86 under autograd: tcsfm_window_loss forward (the scalar stays on the device),
    tcsfm_window_loss_backward behind it.  diff_img and weight_mask of both sides are differentiable; the masks and auto_mask_error are
    not."""

    @staticmethod
    def forward(ctx, engine, sw, f_diff, f_weight, i_diff, i_weight, f_valid, f_ame, i_valid, i_am):
        loss, stats = engine.window_loss(f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, **sw)
        ctx.engine, ctx.sw = engine, dict(sw)
        ctx.save_for_backward(f_diff, f_weight, i_diff, i_weight, f_valid, f_ame, i_valid, i_am, stats)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        want = tuple(ctx.needs_input_grad[2:6])
        if g_loss is None or not any(want):
            return (None,) * 10
        f_diff, f_weight, i_diff, i_weight, f_valid, f_ame, i_valid, i_am, stats = ctx.saved_tensors
        g = ctx.engine.window_loss_backward(f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, stats, _cot(g_loss),
                                            want=want, **ctx.sw)
        return (None, None, *g, None, None, None, None)


class _PoseNetInput(torch.autograd.Function):
    """Engine.posenet_input under autograd: the same forward kernel; the cotangent of the reconstruction (channels 3..5) goes through
    tcsfm_warp_backward (Engine.inverse_warp2_backward).  Channels 0..2 are tgt * valid: the validity mask is not differentiable
    and the images take no gradient, so they carry none."""

    @staticmethod
    def forward(ctx, engine, t, s, dt, ds, p, K):
        out = engine.posenet_input(t, s, dt, ds, p, K)
        ctx.engine = engine
        ctx.save_for_backward(s.contiguous(), dt.contiguous(), ds.contiguous(), p.contiguous(), K.contiguous())
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None, None
        s, dt, ds, p, K = ctx.saved_tensors
        # the warp is inverse_warp2(src, d_t, d_s, -pose, K) (train_mono.py:80): the gradient of -pose, negated, is the pose's
        d_dt, d_ds, d_neg = ctx.engine.inverse_warp2_backward(s, dt, ds, -p, K, g_rec=g[:, 3:6].contiguous(), want=tuple(ctx.needs_input_grad[3:6]))
        return None, None, None, d_dt, d_ds, (None if d_neg is None else -d_neg), None


class Engine:
    """One handle = one GPU + one HIP stream (include/tcsfm.h).  ``max_pairs`` directed pairs of HxW."""

    def __init__(self, H: int, W: int, max_pairs: int, device: Optional[int] = None, lanes: int = 1):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("tightly_coupled_sfm_amd.Engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.H, self.W, self.max_pairs = int(H), int(W), int(max_pairs)
        h = C.c_void_p()
        rc = self.lib.tcsfm_create(C.byref(h), self.device, self.H, self.W, self.max_pairs)
        if rc != 0:
            raise RuntimeError(f"tcsfm_create failed ({rc}): {self.lib.tcsfm_last_error(None).decode()}")
        self._h = h
        self._nets = {}         # the native networks living on this handle: id -> (destroy function, pointer), see _adopt
        self._seq_depthnet = None   # attach_depthnet: the DepthNetHIP behind depths=None of the sequence calls
        self.lanes = 1
        self.lanes_serial = False
        self.use_torch_stream()
        _lib.hint_env(lanes)
        if lanes > 1:
            self.set_lanes(lanes)

    # -- lifetime ----------------------------------------------------------------------------
    def _adopt(self, owner, destroy, ptr):
        """A native network (tcsfm_depthnet / tcsfm_posenet) refers to this handle and must go before it.  Its Python owner destroys it
        through _release; if the handle is closed first -- the garbage collector finalises the objects of an unreachable group in no
        particular order -- close() destroys the network itself and the owner's _release finds nothing left to do."""
        self._nets[id(owner)] = (destroy, ptr)

    def _release(self, owner):
        net = getattr(self, "_nets", {}).pop(id(owner), None)
        if net is not None:
            net[0](net[1])

    def close(self):
        if getattr(self, "_h", None):
            for destroy, ptr in list(getattr(self, "_nets", {}).values()):
                destroy(ptr)
            self._nets = {}
            self.lib.tcsfm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, rc: int):
        if rc != 0:
            raise RuntimeError(f"tcsfm error {rc}: {self.lib.tcsfm_last_error(self._h).decode()}")

    def use_torch_stream(self):
        """Run on torch's current stream of this device, so tensor producers/consumers stay ordered.  Every tensor-level
        method re-binds on entry (a `with torch.cuda.stream(s):` block is honoured); `refine_into` does not."""
        self._follow_torch = True
        self._bound = None
        self._bind()

    def _bind(self):
        if not self._follow_torch:
            return
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound:
            self._call(self.lib.tcsfm_set_stream(self._h, C.c_void_p(s)))
            self._bound = s

    def use_own_stream(self):
        """Run on the handle's private non-blocking stream; the caller orders it against torch work (synchronize())."""
        self._follow_torch = False
        self._call(self.lib.tcsfm_use_own_stream(self._h))

    def set_stream(self, hip_stream: int):
        """Run on the given HIP stream (a raw hipStream_t, e.g. ``torch.cuda.Stream().cuda_stream``) from now on; the engine stops
        following torch's current stream.  Captured call graphs of the old stream are dropped (tcsfm_set_stream)."""
        self._follow_torch = False
        self._call(self.lib.tcsfm_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def last_error(self) -> str:
        return self.lib.tcsfm_last_error(self._h).decode()

    def synchronize(self):
        self._call(self.lib.tcsfm_synchronize(self._h))

    def profile_begin(self):
        """bracket every kernel launch with HIP events on the handle's stream (bench.py roofline leg)"""
        self._call(self.lib.tcsfm_profile_begin(self._h))

    def profile_end(self):
        """-> {'linearize'|'solve'|'pack': (summed ms, launches) from HIP event pairs,
               'linearize_kernel': (summed ms, launches) from the in-kernel s_memrealtime bracket of the linearisation launches,
               'linearize_busy': (ms during which at least one of them ran, launches)}"""
        ms = (C.c_double * 3)(); cnt = (C.c_int64 * 3)()
        self._call(self.lib.tcsfm_profile_end(self._h, ms, cnt))
        out = {k: (ms[i], cnt[i]) for i, k in enumerate(("linearize", "solve", "pack"))}
        kms = C.c_double(); kn = C.c_int64()
        self._call(self.lib.tcsfm_profile_kernel_time(self._h, C.byref(kms), C.byref(kn)))
        out["linearize_kernel"] = (kms.value, kn.value)
        bms = C.c_double(); bn = C.c_int64()
        self._call(self.lib.tcsfm_profile_kernel_busy(self._h, C.byref(bms), C.byref(bn)))
        out["linearize_busy"] = (bms.value, bn.value)      # union of the launches' intervals: (ms with >= 1 launch running, launches)
        return out

    def trace_begin(self, n_lin: int, n_pairs: int):
        """parity-test hook (tcsfm_debug_trace): record the discrete decisions of the following refine* calls (and of linearize /
        linearize_window: trace_begin(1, N), their one linearisation is bits[0]) -- per linearisation and pair one uint16 per pixel (mask, warp validity, bilinear cell parity, L1 / depth-consistency sign codes:
        include/tcsfm.h) and the LM accept / keep decision"""
        self._trace = (torch.zeros((n_lin, n_pairs, self.H, self.W), dtype=torch.int16, device=self.dev),
                       torch.ones((n_lin, n_pairs), dtype=torch.int32, device=self.dev))
        b, d = self._trace
        self._call(self.lib.tcsfm_debug_trace(self._h, self._p(b), b.numel(), self._p(d), d.numel()))

    def trace_end(self):
        """-> (bits [n_lin,N,H,W] uint16, decide [n_lin,N] int32) as numpy arrays; switches the trace off"""
        torch.cuda.synchronize(self.device)
        self._call(self.lib.tcsfm_debug_trace(self._h, None, 0, None, 0))
        b, d = self._trace
        self._trace = None
        return b.cpu().numpy().view(np.uint16), d.cpu().numpy()

    def debug_solve(self, opts, args) -> int:
        """test hook (tcsfm_debug_solve): ONE launch of a production pose solve kernel on the host records and state of `args`
        (_lib.DebugSolveArgs; numpy arrays behind its pointers, outputs filled in place).  -> the return code: 0, or TCSFM_E_ARG for a
        refused launch (last_error() says why; nothing ran)"""
        self._bind()
        return int(self.lib.tcsfm_debug_solve(self._h, C.byref(opts), C.byref(args)))

    def debug_solve_joint(self, opts, args) -> int:
        """test hook (tcsfm_debug_solve_joint): ONE launch of a production joint solve kernel on the host records and state of `args`
        (_lib.DebugSolveJointArgs; numpy arrays behind its pointers, outputs filled in place).  -> the return code, as debug_solve"""
        self._bind()
        return int(self.lib.tcsfm_debug_solve_joint(self._h, C.byref(opts), C.byref(args)))

    @property
    def dev(self) -> torch.device:
        return torch.device("cuda", self.device)

    def _p(self, t: Optional[torch.Tensor]):
        if t is None:
            return None
        if t.device.index != self.device:   # a pointer from another GPU would fault inside the kernel: refuse it here
            raise ValueError(f"tensor lives on {t.device}, this Engine was created for cuda:{self.device}")
        return C.c_void_p(t.data_ptr())

    # -- reference-function drop-ins -----------------------------------------------------------
    def _disp_to_depth(self, d, min_depth, max_depth):
        s, z = torch.empty_like(d), torch.empty_like(d)
        o = default_opts(min_depth=min_depth, max_depth=max_depth)
        self._call(self.lib.tcsfm_disp_to_depth(self._h, C.byref(o), d.numel(), self._p(d), self._p(s), self._p(z)))
        return s, z

    def disp_to_depth(self, disp: torch.Tensor, min_depth: float, max_depth: float):
        """utils/learning_helpers.py:77-86 -> (scaled_disp, depth).  When grad is enabled and disp requires grad both carry a grad_fn
        (tcsfm_disp_to_depth_backward); the values are the plain call's bits."""
        self._bind()
        d = disp.contiguous()
        if d.dtype != torch.float32 or not d.is_cuda:
            raise TypeError("disp must be a float32 GPU tensor")
        if torch.is_grad_enabled() and d.requires_grad:
            return _DispToDepth.apply(self, d, float(min_depth), float(max_depth))
        return self._disp_to_depth(d, min_depth, max_depth)

    def disp_to_depth_backward(self, disp: torch.Tensor, min_depth: float, max_depth: float, g_scaled=None, g_depth=None) -> torch.Tensor:
        """backward of disp_to_depth (tcsfm_disp_to_depth_backward): the cotangents of scaled_disp and depth (None = absent; at least
        one) -> g_disp, shaped as disp"""
        self._bind()
        d = disp.contiguous()
        if d.dtype != torch.float32 or not d.is_cuda:
            raise TypeError("disp must be a float32 GPU tensor")
        g_scaled = None if g_scaled is None else _chk(g_scaled, d.shape, "g_scaled")
        g_depth = None if g_depth is None else _chk(g_depth, d.shape, "g_depth")
        out = torch.empty_like(d)
        o = default_opts(min_depth=min_depth, max_depth=max_depth)
        self._call(self.lib.tcsfm_disp_to_depth_backward(self._h, C.byref(o), d.numel(), self._p(d), self._p(g_scaled), self._p(g_depth),
                                                         self._p(out)))
        return out

    def _ssim(self, x, y):
        out = torch.empty_like(x)
        o = default_opts()
        self._call(self.lib.tcsfm_ssim(self._h, C.byref(o), x.shape[0] * x.shape[1], self._p(x), self._p(y), self._p(out)))
        return out

    def ssim_loss(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """SSIM_Loss.forward (losses.py:27-41) for [N,C,H,W] tensors.  When grad is enabled and x or y requires grad the result carries a
        grad_fn (tcsfm_ssim_backward); the values are the plain call's bits."""
        self._bind()
        N, Cc = x.shape[0], x.shape[1]
        x = _chk(x, (N, Cc, self.H, self.W), "x"); y = _chk(y, (N, Cc, self.H, self.W), "y")
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            return _SSIMLoss.apply(self, x, y)
        return self._ssim(x, y)

    def ssim_loss_backward(self, x: torch.Tensor, y: torch.Tensor, g_out: torch.Tensor, want=(True, True)):
        """backward of ssim_loss (tcsfm_ssim_backward): x, y and the cotangent of the output -> (g_x, g_y), None where ``want`` is False"""
        self._bind()
        N, Cc = x.shape[0], x.shape[1]
        shape = (N, Cc, self.H, self.W)
        x = _chk(x, shape, "x"); y = _chk(y, shape, "y"); g_out = _chk(g_out, shape, "g_out")
        g_x = torch.empty_like(x) if want[0] else None
        g_y = torch.empty_like(y) if want[1] else None
        self._call(self.lib.tcsfm_ssim_backward(self._h, C.byref(default_opts()), N * Cc, self._p(x), self._p(y), self._p(g_out),
                                                self._p(g_x), self._p(g_y)))
        return g_x, g_y

    def smooth_loss(self, disp: torch.Tensor, img: torch.Tensor) -> float:
        """get_smooth_loss (losses.py:43-61): disp [N,1,H,W], img [N,3,H,W] -> python float"""
        self._bind()
        N = disp.shape[0]
        disp = _chk(disp, (N, 1, self.H, self.W), "disp"); img = _chk(img, (N, 3, self.H, self.W), "img")
        out = C.c_double()
        self._call(self.lib.tcsfm_smooth_loss(self._h, C.byref(default_opts()), N, self._p(disp), self._p(img), C.byref(out)))
        return out.value

    def smooth_loss_device(self, disp: torch.Tensor, img: torch.Tensor):
        """get_smooth_loss without the host round trip (tcsfm_smooth_loss_device) -> (loss: 0-dim float32 tensor, stats [N,3] float64:
        per image the mean disparity and the sums of the x and y terms, the input of smooth_loss_backward)"""
        self._bind()
        N = disp.shape[0]
        disp = _chk(disp, (N, 1, self.H, self.W), "disp"); img = _chk(img, (N, 3, self.H, self.W), "img")
        loss = torch.empty((), dtype=torch.float32, device=disp.device)
        stats = torch.empty((N, 3), dtype=torch.float64, device=disp.device)
        self._call(self.lib.tcsfm_smooth_loss_device(self._h, C.byref(default_opts()), N, self._p(disp), self._p(img), self._p(loss), self._p(stats)))
        return loss, stats

    def smooth_loss_backward(self, disp: torch.Tensor, img: torch.Tensor, stats: torch.Tensor, g_loss: torch.Tensor) -> torch.Tensor:
        """backward of get_smooth_loss with respect to disp (tcsfm_smooth_loss_backward): ``stats`` from smooth_loss_device on the same
        inputs, ``g_loss`` a float32 GPU tensor with one element -> g_disp [N,1,H,W]"""
        self._bind()
        N = disp.shape[0]
        disp = _chk(disp, (N, 1, self.H, self.W), "disp"); img = _chk(img, (N, 3, self.H, self.W), "img")
        if stats.dtype != torch.float64 or not stats.is_cuda or tuple(stats.shape) != (N, 3):
            raise TypeError(f"stats must be a float64 GPU tensor of shape [{N}, 3]")
        g_loss = _chk(g_loss.reshape(()), (), "g_loss")
        out = torch.empty_like(disp)
        self._call(self.lib.tcsfm_smooth_loss_backward(self._h, C.byref(default_opts()), N, self._p(disp), self._p(img),
                                                       self._p(stats.contiguous()), self._p(g_loss), self._p(out)))
        return out

    def _window_maps(self, f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, argmin, automasking, inverse):
        """shape / dtype checks of the eight maps of the window loss -> (B S, the maps with None where the library does not read one)"""
        if f_diff.dim() != 4:
            raise AssertionError("wrong size for fwd diff_img, expected [S*B,1,H,W], got  {}".format(list(f_diff.shape)))
        shape = (f_diff.shape[0], 1, self.H, self.W)
        need = [True, True, True, bool(argmin and automasking), bool(inverse), bool(inverse), bool(inverse), bool(inverse and automasking)]
        names = ("fwd diff_img", "fwd valid_mask", "fwd weight_mask", "fwd auto_mask_error", "inv diff_img", "inv valid_mask", "inv weight_mask",
                 "inv auto_mask")
        maps = []
        for t, n, name in zip((f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am), need, names):
            if not n:
                maps.append(None)
                continue
            if t is None:
                raise ValueError(f"{name} is needed with these switches")
            maps.append(_chk(t, shape, name))
        return shape, maps

    def window_loss(self, f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, S: int, argmin: bool = True,
                    automasking: bool = True, inverse: bool = True, w_dc: float = 0.0):
        """The window loss of optimizer.py:47-86 (tcsfm_window_loss): the forward term (per-pixel min over the S sources with ``argmin``),
        0.25 x the inverse term with ``inverse``, and the depth-consistency terms with weight ``w_dc`` (0 = off).  The maps are
        [S*B,1,H,W] float32, source-major, as solve_pose_iteratively emits them: forward diff_img, valid_mask (warp validity), weight_mask,
        auto_mask_error, then inverse diff_img, valid_mask, weight_mask, auto_mask (None where the switches do not read one)
        -> (loss: 0-dim float32 tensor, stats: 7 float64 = N1, D1, N2, D2, W1, W2, n, the input of window_loss_backward).  No host round
        trip, no synchronisation."""
        self._bind()
        S = int(S)
        shape, maps = self._window_maps(f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, argmin, automasking, inverse)
        if S < 1 or shape[0] % S:
            raise ValueError(f"{shape[0]} maps are not S = {S} sources of B targets")
        loss = torch.empty((), dtype=torch.float32, device=f_diff.device)
        stats = torch.empty((7,), dtype=torch.float64, device=f_diff.device)
        o = default_opts(automask=1 if automasking else 0, w_dc=float(w_dc))
        self._call(self.lib.tcsfm_window_loss(self._h, C.byref(o), shape[0] // S, S, int(bool(argmin)), int(bool(inverse)),
                                              *[self._p(m) for m in maps], self._p(loss), self._p(stats)))
        return loss, stats

    def window_loss_backward(self, f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, stats, g_loss, S: int,
                             argmin: bool = True, automasking: bool = True, inverse: bool = True, w_dc: float = 0.0,
                             want=(True, True, True, True)):
        """backward of window_loss (tcsfm_window_loss_backward): the same maps and switches, ``stats`` of window_loss on them and ``g_loss``, a
        float32 GPU tensor with one element -> (g_fwd_diff, g_fwd_weight, g_inv_diff, g_inv_weight), None where ``want`` is False"""
        self._bind()
        S = int(S)
        shape, maps = self._window_maps(f_diff, f_valid, f_weight, f_ame, i_diff, i_valid, i_weight, i_am, argmin, automasking, inverse)
        if S < 1 or shape[0] % S:
            raise ValueError(f"{shape[0]} maps are not S = {S} sources of B targets")
        if stats.dtype != torch.float64 or not stats.is_cuda or tuple(stats.shape) != (7,):
            raise TypeError("stats must be a float64 GPU tensor of shape [7]")
        g_loss = _chk(g_loss.reshape(()), (), "g_loss")
        outs = [torch.empty(shape, dtype=torch.float32, device=f_diff.device) if w else None for w in want]
        o = default_opts(automask=1 if automasking else 0, w_dc=float(w_dc))
        self._call(self.lib.tcsfm_window_loss_backward(self._h, C.byref(o), shape[0] // S, S, int(bool(argmin)), int(bool(inverse)),
                                                       *[self._p(m) for m in maps], self._p(stats.contiguous()), self._p(g_loss),
                                                       *[self._p(t) for t in outs]))
        return tuple(outs)

    def inverse_warp2(self, img, depth, ref_depth, pose, intrinsics):
        """models/stn.py:234-273 with the reference's argument order; ``pose`` here is what the reference
        passes, i.e. callers that wrote ``inverse_warp2(src, d_t, d_s, -poses, K)`` keep passing ``-poses``."""
        self._bind()
        N = img.shape[0]
        H, W = self.H, self.W
        img = _chk(img, (N, 3, H, W), "img"); depth = _chk(depth, (N, 1, H, W), "depth")
        ref_depth = _chk(ref_depth, (N, 1, H, W), "ref_depth"); intrinsics = _chk(intrinsics, (N, 3, 3), "intrinsics")
        pose6 = _chk(pose[:, 0:6].contiguous(), (N, 6), "pose")
        neg = (-pose6).contiguous()  # the ABI applies pose_vec2mat(-pose) like the reference call sites
        rec = torch.empty_like(img); valid = torch.empty_like(depth); pd = torch.empty_like(depth); cd = torch.empty_like(depth)
        o = default_opts()
        self._call(self.lib.tcsfm_warp(self._h, C.byref(o), N, self._p(img), self._p(depth), self._p(ref_depth), self._p(neg),
                                       self._p(intrinsics), self._p(rec), self._p(valid), self._p(pd), self._p(cd)))
        return rec, valid, pd, cd

    def inverse_warp2_backward(self, img, depth, ref_depth, pose, intrinsics, g_rec=None, g_pd=None, g_cd=None, want=(True, True, True)):
        """backward of inverse_warp2 (tcsfm_warp_backward): the forward's arguments, the cotangents of the reconstruction, the
        projected and the computed depth (None = zero) -> (d_depth, d_ref_depth, d_pose), None where ``want`` is False.  ``pose``
        and d_pose are in the reference's convention, as in inverse_warp2.  No gradient exists for img and intrinsics."""
        self._bind()
        N = img.shape[0]
        H, W = self.H, self.W
        img = _chk(img, (N, 3, H, W), "img"); depth = _chk(depth, (N, 1, H, W), "depth")
        ref_depth = _chk(ref_depth, (N, 1, H, W), "ref_depth"); intrinsics = _chk(intrinsics, (N, 3, 3), "intrinsics")
        pose6 = _chk(pose[:, 0:6].contiguous(), (N, 6), "pose")
        neg = (-pose6).contiguous()
        g_rec = None if g_rec is None else _chk(g_rec, (N, 3, H, W), "g_rec")
        g_pd = None if g_pd is None else _chk(g_pd, (N, 1, H, W), "g_pd")
        g_cd = None if g_cd is None else _chk(g_cd, (N, 1, H, W), "g_cd")
        d_depth = torch.empty_like(depth) if want[0] else None
        d_ref = torch.empty_like(ref_depth) if want[1] else None
        d_neg = torch.empty_like(neg) if want[2] else None
        o = default_opts()
        self._call(self.lib.tcsfm_warp_backward(self._h, C.byref(o), N, self._p(img), self._p(depth), self._p(ref_depth), self._p(neg),
                                                self._p(intrinsics), self._p(g_rec), self._p(g_pd), self._p(g_cd),
                                                self._p(d_depth), self._p(d_ref), self._p(d_neg)))
        return d_depth, d_ref, (None if d_neg is None else -d_neg)     # the ABI's pose is -pose: so is its gradient

    def posenet_input(self, target_img, source_img, target_depth, source_depth, pose, intrinsics):
        """(tgt * valid | img_rec) [N,6,H,W] for the next PoseNet call of the coupled iteration (train_mono.py:73-77);
        `pose` is the estimate so far in the reference convention (the warp uses -pose like train_mono.py:80).  Never carries a
        grad_fn: posenet_input_autograd is the differentiable form."""
        self._bind()
        N = target_img.shape[0]
        H, W = self.H, self.W
        t = _chk(target_img, (N, 3, H, W), "target_img"); s = _chk(source_img, (N, 3, H, W), "source_img")
        dt = _chk(target_depth, (N, 1, H, W), "target_depth"); ds = _chk(source_depth, (N, 1, H, W), "source_depth")
        p = _chk(pose, (N, 6), "pose"); K = _chk(intrinsics, (N, 3, 3), "intrinsics")
        out = torch.empty((N, 6, H, W), device=t.device, dtype=torch.float32)
        o = default_opts()
        self._call(self.lib.tcsfm_warp_posenet_input(self._h, C.byref(o), N, self._p(t), self._p(s), self._p(dt), self._p(ds), self._p(p),
                                                     self._p(K), self._p(out), None))
        return out

    def posenet_input_autograd(self, target_img, source_img, target_depth, source_depth, pose, intrinsics):
        """posenet_input with a grad_fn towards the depths and the pose: the same forward kernel (the same bits); channels 3..5 (the
        reconstruction) go back through the warp's HIP backward (tcsfm_warp_backward), channels 0..2 (tgt * valid) carry no gradient
        because the validity mask is not differentiable.  Images or intrinsics that require grad raise NotImplementedError."""
        if target_img.requires_grad or source_img.requires_grad or intrinsics.requires_grad:
            raise NotImplementedError("posenet_input has no gradient with respect to the images or the intrinsics "
                                      "(DESIGN.md section 7: gradients with respect to the images stay out of scope)")
        return _PoseNetInput.apply(self, target_img, source_img, target_depth, source_depth, pose, intrinsics)

    def _photometric(self, t, s, dt, ds, p, K, o):
        N = t.shape[0]
        diff, valid, weight, ae, am = (torch.empty_like(dt) for _ in range(5))
        rec = torch.empty_like(t)
        self._call(self.lib.tcsfm_photometric(self._h, C.byref(o), N, self._p(t), self._p(s), self._p(dt), self._p(ds), self._p(p),
                                              self._p(K), self._p(diff), self._p(valid), self._p(weight), self._p(ae), self._p(am),
                                              self._p(rec)))
        return diff, valid, weight, ae, am, rec

    def compute_photometric_error(self, target_img, source_img, target_depth, source_depth, pose, intrinsics,
                                  opts: Optional[Opts] = None):
        """optimization_experiments/helpers.py:8-23 -> dict with the reference's keys (+ the raw maps).  When grad is enabled and
        target_depth, source_depth or pose requires grad, diff_img, weight_mask and img_rec carry a grad_fn (HIP backward kernels,
        tcsfm_photometric_backward); the masks never do."""
        self._bind()
        N = target_img.shape[0]
        H, W = self.H, self.W
        t = _chk(target_img, (N, 3, H, W), "target_img"); s = _chk(source_img, (N, 3, H, W), "source_img")
        dt = _chk(target_depth, (N, 1, H, W), "target_depth"); ds = _chk(source_depth, (N, 1, H, W), "source_depth")
        p = _chk(pose, (N, 6), "pose"); K = _chk(intrinsics, (N, 3, 3), "intrinsics")
        o = opts or default_opts()
        if torch.is_grad_enabled() and any(x.requires_grad for x in (t, s, dt, ds, p, K)):
            if t.requires_grad or s.requires_grad or K.requires_grad:
                raise NotImplementedError("compute_photometric_error has no gradient with respect to the images or the intrinsics "
                                          "(DESIGN.md section 7: gradients with respect to the images stay out of scope)")
            if o.depth_is_disp:
                raise NotImplementedError("compute_photometric_error is differentiable on depth maps only (apply disp_to_depth first)")
            diff, rec, weight, valid, ae, am, valid_mask = _PhotometricError.apply(self, o, t, s, dt, ds, p, K)
        else:
            diff, valid, weight, ae, am, rec = self._photometric(t, s, dt, ds, p, K, o)
            valid_mask = am * valid
        return {"diff_img": diff, "img_rec": rec, "valid_mask": valid_mask, "weight_mask": weight, "poses": pose,
                "warp_valid": valid, "auto_mask_error": ae, "auto_mask": am}

    def photometric_maps_backward(self, target_img, img_rec, proj_depth, comp_depth, g_diff=None, g_weight=None, want=(True, True, True),
                                  opts: Optional[Opts] = None):
        """backward of the residual assembly alone (tcsfm_photometric_maps_backward): diff_img and weight_mask as functions of
        (img_rec, projected depth, computed depth); the cotangents of the two maps (None = zero) -> (g_rec, g_proj_depth, g_comp_depth),
        None where ``want`` is False."""
        self._bind()
        N = target_img.shape[0]
        H, W = self.H, self.W
        t = _chk(target_img, (N, 3, H, W), "target_img"); r = _chk(img_rec, (N, 3, H, W), "img_rec")
        pd = _chk(proj_depth, (N, 1, H, W), "proj_depth"); cd = _chk(comp_depth, (N, 1, H, W), "comp_depth")
        g_diff = None if g_diff is None else _chk(g_diff, (N, 1, H, W), "g_diff")
        g_weight = None if g_weight is None else _chk(g_weight, (N, 1, H, W), "g_weight")
        g_rec = torch.empty_like(r) if want[0] else None
        g_pd = torch.empty_like(pd) if want[1] else None
        g_cd = torch.empty_like(cd) if want[2] else None
        o = opts or default_opts()
        self._call(self.lib.tcsfm_photometric_maps_backward(self._h, C.byref(o), N, self._p(t), self._p(r), self._p(pd), self._p(cd),
                                                            self._p(g_diff), self._p(g_weight), self._p(g_rec), self._p(g_pd), self._p(g_cd)))
        return g_rec, g_pd, g_cd

    def compute_photometric_error_backward(self, target_img, source_img, target_depth, source_depth, pose, intrinsics, g_diff=None,
                                           g_weight=None, g_img_rec=None, want=(True, True, True), opts: Optional[Opts] = None):
        """backward of compute_photometric_error (tcsfm_photometric_backward): the forward's arguments and the cotangents of diff_img,
        weight_mask and img_rec (None = zero) -> (d_target_depth, d_source_depth, d_pose), None where ``want`` is False.  ``pose`` and
        d_pose are in the reference's convention, as in compute_photometric_error."""
        self._bind()
        N = target_img.shape[0]
        H, W = self.H, self.W
        t = _chk(target_img, (N, 3, H, W), "target_img"); s = _chk(source_img, (N, 3, H, W), "source_img")
        dt = _chk(target_depth, (N, 1, H, W), "target_depth"); ds = _chk(source_depth, (N, 1, H, W), "source_depth")
        p = _chk(pose, (N, 6), "pose"); K = _chk(intrinsics, (N, 3, 3), "intrinsics")
        g_diff = None if g_diff is None else _chk(g_diff, (N, 1, H, W), "g_diff")
        g_weight = None if g_weight is None else _chk(g_weight, (N, 1, H, W), "g_weight")
        g_img_rec = None if g_img_rec is None else _chk(g_img_rec, (N, 3, H, W), "g_img_rec")
        d_dt = torch.empty_like(dt) if want[0] else None
        d_ds = torch.empty_like(ds) if want[1] else None
        d_p = torch.empty_like(p) if want[2] else None
        o = opts or default_opts()
        self._call(self.lib.tcsfm_photometric_backward(self._h, C.byref(o), N, self._p(t), self._p(s), self._p(dt), self._p(ds), self._p(p),
                                                       self._p(K), self._p(g_diff), self._p(g_weight), self._p(g_img_rec),
                                                       self._p(d_dt), self._p(d_ds), self._p(d_p)))
        return d_dt, d_ds, d_p

    def loss_surface(self, target_img, source_img, target_depth, source_depth, intrinsics, poses, opts: Optional[Opts] = None):
        """costs of ONE pair under P candidate poses (plot_loss_surface.py:31-33,45-47) -> np.ndarray [P] float64"""
        self._bind()
        H, W = self.H, self.W
        t = _chk(target_img, (1, 3, H, W), "target_img"); s = _chk(source_img, (1, 3, H, W), "source_img")
        dt = _chk(target_depth, (1, 1, H, W), "target_depth"); ds = _chk(source_depth, (1, 1, H, W), "source_depth")
        K = _chk(intrinsics, (1, 3, 3), "intrinsics")
        P = poses.shape[0]
        p = _chk(poses, (P, 6), "poses")
        o = opts or default_opts()
        out = np.zeros(P, dtype=np.float64)
        self._call(self.lib.tcsfm_loss_surface(self._h, C.byref(o), self._p(t), self._p(s), self._p(dt), self._p(ds), self._p(K),
                                               P, self._p(p), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- Gauss-Newton engine -----------------------------------------------------------------------
    def _pairs(self, tgt, src, depth_t, depth_s, K, pose):
        N = tgt.shape[0]
        H, W = self.H, self.W
        return (N, _chk(tgt, (N, 3, H, W), "tgt"), _chk(src, (N, 3, H, W), "src"), _chk(depth_t, (N, 1, H, W), "depth_t"),
                _chk(depth_s, (N, 1, H, W), "depth_s"), _chk(K, (N, 3, 3), "K"), _chk(pose, (N, 6), "pose"))

    def linearize(self, tgt, src, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, log_scale=None):
        """normal equations at ``pose`` -> dict(H [N,np,np], g [N,np], cost, cost_photo, cost_dc, n_mask [N]) (numpy f64)"""
        self._bind()
        o = opts or default_opts()
        N, tgt, src, depth_t, depth_s, K, pose = self._pairs(tgt, src, depth_t, depth_s, K, pose)
        n_p = 7 if o.refine == _lib.REFINE_POSE_SCALE else 6
        ls = None if log_scale is None else _chk(log_scale, (N,), "log_scale")
        Hm = np.zeros((N, n_p, n_p)); g = np.zeros((N, n_p)); st = np.zeros((N, 4))
        self._call(self.lib.tcsfm_linearize(self._h, C.byref(o), N, self._p(tgt), self._p(src), self._p(depth_t), self._p(depth_s),
                                            self._p(pose), self._p(ls), self._p(K), Hm.ctypes.data_as(C.c_void_p),
                                            g.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)))
        return dict(H=Hm, g=g, cost=st[:, 0], cost_photo=st[:, 1], cost_dc=st[:, 2], n_mask=st[:, 3])

    def refine(self, tgt, src, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, log_scale=None, stats: bool = False):
        """Refine N directed pairs in place-free style: returns (pose [N,6], log_scale [N] or None, stats or None).
        Asynchronous on the handle's stream; outputs are GPU tensors."""
        self._bind()
        o = opts or default_opts()
        N, tgt, src, depth_t, depth_s, K, pose = self._pairs(tgt, src, depth_t, depth_s, K, pose)
        pose_out = torch.empty_like(pose)
        ls_in = ls_out = None
        if o.refine == _lib.REFINE_POSE_SCALE:
            ls_in = torch.zeros(N, device=pose.device, dtype=torch.float32) if log_scale is None else _chk(log_scale, (N,), "log_scale")
            ls_out = torch.empty_like(ls_in)
        st = torch.empty((N, o.n_iters + 1, _lib.NSTAT), device=pose.device, dtype=torch.float32) if stats else None
        self._call(self.lib.tcsfm_refine(self._h, C.byref(o), N, self._p(tgt), self._p(src), self._p(depth_t), self._p(depth_s),
                                         self._p(K), self._p(pose), self._p(ls_in), self._p(pose_out), self._p(ls_out), self._p(st)))
        return pose_out, ls_out, st

    def linearize_window(self, tgt, srcs, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, log_scale=None, argmin: Optional[bool] = None):
        """ONE linearisation of a window's 2*S*B directed pairs (layouts of refine_window) at ``pose`` under opts.argmin /
        opts.window_rule -> dict(H [2SB,np,np], g [2SB,np], cost, cost_photo, cost_dc, n_mask [2SB]) (numpy f64).  With
        window_rule = WINDOW_REFERENCE the costs add up to the reference's compute_optimization_loss (optimizer.py:47-86)."""
        self._bind()
        o = opts or default_opts()
        if argmin is not None:
            o = _copy_opts(o); o.argmin = 1 if argmin else 0
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        N = 2 * S * B
        tgt = _chk(tgt, (B, 3, self.H, self.W), "tgt"); srcs = _chk(srcs, (S, B, 3, self.H, self.W), "srcs")
        depth_t = _chk(depth_t, (B, 1, self.H, self.W), "depth_t"); depth_s = _chk(depth_s, (S, B, 1, self.H, self.W), "depth_s")
        K = _chk(K, (B, 3, 3), "K"); pose = _chk(pose, (N, 6), "pose")
        n_p = 7 if o.refine == _lib.REFINE_POSE_SCALE else 6
        ls = None if log_scale is None else _chk(log_scale, (N,), "log_scale")
        Hm = np.zeros((N, n_p, n_p)); g = np.zeros((N, n_p)); st = np.zeros((N, 4))
        self._call(self.lib.tcsfm_linearize_window(self._h, C.byref(o), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                   self._p(K), self._p(pose), self._p(ls), Hm.ctypes.data_as(C.c_void_p),
                                                   g.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)))
        return dict(H=Hm, g=g, cost=st[:, 0], cost_photo=st[:, 1], cost_dc=st[:, 2], n_mask=st[:, 3])

    def refine_window(self, tgt, srcs, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, log_scale=None, stats: bool = False,
                      argmin: Optional[bool] = None):
        """Window form (the call surface of solve_pose_iteratively, train_mono.py:41-62): tgt [B,3,H,W], srcs [S,B,3,H,W] (or a
        list of S tensors), depth_t [B,1,H,W], depth_s [S,B,1,H,W] (or list), K [B,3,3], pose [2*S*B,6] in the stacked order
        (forward pairs source-major, then inverse pairs).  The 2*S*B directed pairs are formed inside the library; with
        argmin (default: opts.argmin) and S > 1 the forward pairs use the per-pixel min over the sources (optimizer.py:47-69).
        -> (pose [2SB,6], log_scale [2SB] or None, stats or None)"""
        self._bind()
        o = opts or default_opts()
        if argmin is not None:
            o = _copy_opts(o); o.argmin = 1 if argmin else 0
        if isinstance(srcs, (list, tuple)):
            srcs = torch.stack(list(srcs), 0)
        if isinstance(depth_s, (list, tuple)):
            depth_s = torch.stack(list(depth_s), 0)
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        N = 2 * S * B
        tgt = _chk(tgt, (B, 3, self.H, self.W), "tgt"); srcs = _chk(srcs, (S, B, 3, self.H, self.W), "srcs")
        depth_t = _chk(depth_t, (B, 1, self.H, self.W), "depth_t"); depth_s = _chk(depth_s, (S, B, 1, self.H, self.W), "depth_s")
        K = _chk(K, (B, 3, 3), "K"); pose = _chk(pose, (N, 6), "pose")
        pose_out = torch.empty_like(pose)
        ls_in = ls_out = None
        if o.refine == _lib.REFINE_POSE_SCALE:
            ls_in = torch.zeros(N, device=pose.device, dtype=torch.float32) if log_scale is None else _chk(log_scale, (N,), "log_scale")
            ls_out = torch.empty_like(ls_in)
        st = torch.empty((N, o.n_iters + 1, _lib.NSTAT), device=pose.device, dtype=torch.float32) if stats else None
        self._call(self.lib.tcsfm_refine_window(self._h, C.byref(o), B, S, self._p(tgt), self._p(srcs), self._p(depth_t),
                                                self._p(depth_s), self._p(K), self._p(pose), self._p(ls_in), self._p(pose_out),
                                                self._p(ls_out), self._p(st)))
        return pose_out, ls_out, st

    def refine_dense(self, tgt, src, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, stats: bool = False):
        """Dense mode: refine pose AND per-pixel inverse depth of the target (per-pixel Schur complement).
        -> (pose [N,6], depth [N,1,H,W], stats or None); opts.lambda_depth / opts.prior_depth / min_depth / max_depth apply."""
        self._bind()
        o = opts or default_opts()
        N, tgt, src, depth_t, depth_s, K, pose = self._pairs(tgt, src, depth_t, depth_s, K, pose)
        pose_out, depth_out = torch.empty_like(pose), torch.empty_like(depth_t)
        st = torch.empty((N, o.n_iters + 1, _lib.NSTAT), device=pose.device, dtype=torch.float32) if stats else None
        self._call(self.lib.tcsfm_refine_dense(self._h, C.byref(o), N, self._p(tgt), self._p(src), self._p(depth_t), self._p(depth_s),
                                               self._p(K), self._p(pose), self._p(pose_out), self._p(depth_out), self._p(st)))
        return pose_out, depth_out, st

    def refine_dense_window(self, tgt, srcs, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, stats: bool = False,
                            argmin: Optional[bool] = None):
        """Dense mode in window form (see refine_window for the layout): every directed pair refines its pose and its own copy
        of its target's depth -> (pose [2SB,6], depth [2SB,1,H,W] in the stacked pair order, stats or None)"""
        self._bind()
        o = opts or default_opts()
        if argmin is not None:
            o = _copy_opts(o); o.argmin = 1 if argmin else 0
        if isinstance(srcs, (list, tuple)):
            srcs = torch.stack(list(srcs), 0)
        if isinstance(depth_s, (list, tuple)):
            depth_s = torch.stack(list(depth_s), 0)
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        N = 2 * S * B
        tgt = _chk(tgt, (B, 3, self.H, self.W), "tgt"); srcs = _chk(srcs, (S, B, 3, self.H, self.W), "srcs")
        depth_t = _chk(depth_t, (B, 1, self.H, self.W), "depth_t"); depth_s = _chk(depth_s, (S, B, 1, self.H, self.W), "depth_s")
        K = _chk(K, (B, 3, 3), "K"); pose = _chk(pose, (N, 6), "pose")
        pose_out = torch.empty_like(pose)
        depth_out = torch.empty((N, 1, self.H, self.W), device=pose.device, dtype=torch.float32)
        st = torch.empty((N, o.n_iters + 1, _lib.NSTAT), device=pose.device, dtype=torch.float32) if stats else None
        self._call(self.lib.tcsfm_refine_dense_window(self._h, C.byref(o), B, S, self._p(tgt), self._p(srcs), self._p(depth_t),
                                                      self._p(depth_s), self._p(K), self._p(pose), self._p(pose_out), self._p(depth_out),
                                                      self._p(st)))
        return pose_out, depth_out, st

    def linearize_dense_window(self, tgt, srcs, depth_t, depth_s, K, pose, opts: Optional[Opts] = None, argmin: Optional[bool] = None, depth0=None,
                               sources: bool = False):
        """tcsfm_linearize_dense_window: ONE linearisation of the dense window mode on the reference's own loss (window_rule REFERENCE;
        optimizer.py:47-90) -> dict(loss, fwd, inv_photo, inv_dc, K_f, K_i, a_f, g_pose [2SB,6] float64 (w.r.t. the left SE(3)
        perturbation of every pair's warp), g_rho [B,1,H,W] GPU tensor = d loss / d inverse depth of every target);
        depth0 [B,1,H,W]: the centre of the l_depth_init prior (default: depth_t).  sources=True (tcsfm_linearize_dense_window_sources):
        also g_rho_src [S,B,1,H,W] = d loss / d inverse depth of every SOURCE map (held fixed by the refinement)"""
        self._bind()
        o = _copy_opts(opts or default_opts())
        if argmin is not None:
            o.argmin = 1 if argmin else 0
        o.window_rule = _lib.WINDOW_REFERENCE
        if isinstance(srcs, (list, tuple)):
            srcs = torch.stack(list(srcs), 0)
        if isinstance(depth_s, (list, tuple)):
            depth_s = torch.stack(list(depth_s), 0)
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        N = 2 * S * B
        tgt = _chk(tgt, (B, 3, self.H, self.W), "tgt"); srcs = _chk(srcs, (S, B, 3, self.H, self.W), "srcs")
        depth_t = _chk(depth_t, (B, 1, self.H, self.W), "depth_t"); depth_s = _chk(depth_s, (S, B, 1, self.H, self.W), "depth_s")
        K = _chk(K, (B, 3, 3), "K"); pose = _chk(pose, (N, 6), "pose")
        d0 = None if depth0 is None else _chk(depth0, (B, 1, self.H, self.W), "depth0")
        scal = np.zeros(8); gp = np.zeros((N, 6))
        g_rho = torch.empty((B, 1, self.H, self.W), device=pose.device, dtype=torch.float32)
        g_src = torch.empty((S, B, 1, self.H, self.W), device=pose.device, dtype=torch.float32) if sources else None
        if sources:
            self._call(self.lib.tcsfm_linearize_dense_window_sources(self._h, C.byref(o), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                                     self._p(K), self._p(pose), self._p(d0), scal.ctypes.data_as(C.c_void_p),
                                                                     gp.ctypes.data_as(C.c_void_p), self._p(g_rho), self._p(g_src)))
        else:
            self._call(self.lib.tcsfm_linearize_dense_window(self._h, C.byref(o), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                             self._p(K), self._p(pose), self._p(d0), scal.ctypes.data_as(C.c_void_p),
                                                             gp.ctypes.data_as(C.c_void_p), self._p(g_rho)))
        torch.cuda.synchronize(self.device)
        out = dict(loss=scal[0], fwd=scal[1], inv_photo=scal[2], inv_dc=scal[3], K_f=scal[4], K_i=scal[5], a_f=scal[6], pose_consist=scal[7], g_pose=gp, g_rho=g_rho)
        if sources:
            out["g_rho_src"] = g_src
        return out

    def scale_recovery(self, depth, intrinsics, real_cam_height: float, pad_to_batch: int = 0, maps: bool = False):
        """ScaleRecovery.forward (dnet_layers.py:306-327): depth [N,1,H,W], K [N,3,3] -> scale [1] (GPU tensor)
        (+ median [1], height [N,1,H,W], mask [N,1,H,W] with maps=True)"""
        self._bind()
        N = depth.shape[0]
        depth = _chk(depth, (N, 1, self.H, self.W), "depth"); K = _chk(intrinsics, (N, 3, 3), "intrinsics")
        scale = torch.empty(1, device=depth.device, dtype=torch.float32); med = torch.empty_like(scale)
        hm = torch.empty_like(depth) if maps else None
        mm = torch.empty_like(depth) if maps else None
        o = default_opts()
        self._call(self.lib.tcsfm_scale_recovery(self._h, C.byref(o), N, self._p(depth), self._p(K), float(real_cam_height),
                                                 int(pad_to_batch), self._p(scale), self._p(med), self._p(hm), self._p(mm)))
        return (scale, med, hm, mm) if maps else scale

    def scale_recovery_frames(self, depth, intrinsics, real_cam_height: float):
        """tcsfm_scale_recovery_frames: depth [N,1,H,W], K [N,3,3] or [3,3] (one camera for all) -> (scale [N], median [N], count [N]
        int32) as CUDA tensors: item n's scale and median are the bits of scale_recovery(depth[n:n+1], K[n:n+1], h), count its ground
        pixels; two launches whatever N, on the engine's stream"""
        self._bind()
        N = depth.shape[0]
        depth = _chk(depth, (N, 1, self.H, self.W), "depth")
        if isinstance(intrinsics, torch.Tensor) and tuple(intrinsics.shape) == (3, 3):
            intrinsics = intrinsics[None].expand(N, 3, 3).contiguous()
        K = _chk(intrinsics, (N, 3, 3), "intrinsics")
        scale = torch.empty(N, device=depth.device, dtype=torch.float32); med = torch.empty_like(scale)
        count = torch.empty(N, device=depth.device, dtype=torch.int32)
        o = default_opts()
        self._call(self.lib.tcsfm_scale_recovery_frames(self._h, C.byref(o), N, self._p(depth), self._p(K), float(real_cam_height),
                                                        self._p(scale), self._p(med), self._p(count)))
        return scale, med, count

    # -- lanes: several refinements in flight (include/tcsfm.h "lanes") -----------------------------------------
    def set_lanes(self, n: int):
        _lib.warn_if_queues_late(int(n))
        self._call(self.lib.tcsfm_set_lanes(self._h, int(n)))
        self.lanes = int(n)
        self.lanes_serial = self.lane_probe()["serial"]

    def lane_probe(self):
        """tcsfm_lane_probe: what tcsfm_set_lanes measured -- {'serial': the streams of this process do not run side by side and lane calls
        fall back to the handle's own stream, 'one_stream_us', 'two_streams_us': the probe's 16 stand-in launches}"""
        s_, a, b = C.c_int(0), C.c_float(0), C.c_float(0)
        self._call(self.lib.tcsfm_lane_probe(self._h, C.byref(s_), C.byref(a), C.byref(b)))
        return {"serial": bool(s_.value), "one_stream_us": round(a.value * 1e3, 1), "two_streams_us": round(b.value * 1e3, 1)}

    def set_graph_replay(self, max_graphs: int = 4):
        """tcsfm_set_graph_replay: repeated device-pointer refine calls (same tensors, same options) are captured once and
        replayed as one HIP graph per call -- one host launch instead of nine; bit-identical results.  0 switches it off."""
        self._call(self.lib.tcsfm_set_graph_replay(self._h, int(max_graphs)))

    def graph_replay_counts(self):
        """(captures, replays) so far, handle + lanes"""
        c, r = C.c_int(0), C.c_int(0)
        self._call(self.lib.tcsfm_graph_replay_counts(self._h, C.byref(c), C.byref(r)))
        return c.value, r.value

    # -- coalesced calls: queued calls of one shape as ONE launch sequence (include/tcsfm.h "coalesced calls") -------------------
    def set_coalesce(self, max_calls: int):
        """tcsfm_set_coalesce: up to `max_calls` queued refine_window_queued calls of one shape run as one launch sequence"""
        self._call(self.lib.tcsfm_set_coalesce(self._h, int(max_calls)))

    def set_coalesce_lanes(self, n_streams: int):
        """tcsfm_set_coalesce_lanes: merged sequences alternate over `n_streams` of the handle's streams (needs that many lanes);
        `flush()` / `synchronize()` order the handle's stream behind them"""
        self._call(self.lib.tcsfm_set_coalesce_lanes(self._h, int(n_streams)))

    def refine_window_queued(self, tgt, srcs, depth_t, depth_s, K, pose, pose_out, opts: Opts):
        """tcsfm_refine_window_queued: note a window call (validated contiguous float32 CUDA tensors in the window layout, see
        refine_window); it runs -- merged with the other waiting calls of its shape -- when the queue is full, at flush() or at
        synchronize().  Per window the result is bit-identical to refine_window on its own."""
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        self._call(self.lib.tcsfm_refine_window_queued(self._h, C.byref(opts), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                       self._p(K), self._p(pose), self._p(pose_out)))

    def refine_window_scale_queued(self, tgt, srcs, depth_t, depth_s, K, pose, log_scale, pose_out, log_scale_out, opts: Opts):
        """tcsfm_refine_window_scale_queued: refine_window_queued with the depth-scale unknown (opts.refine = REFINE_POSE_SCALE)"""
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        self._call(self.lib.tcsfm_refine_window_scale_queued(self._h, C.byref(opts), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                             self._p(K), self._p(pose), self._p(log_scale), self._p(pose_out), self._p(log_scale_out)))

    def refine_dense_window_queued(self, tgt, srcs, depth_t, depth_s, K, pose, pose_out, depth_out, opts: Opts):
        """tcsfm_refine_dense_window_queued: the dense counterpart of refine_window_queued (window layout of refine_dense_window; depth_out
        [2*S*B,1,H,W]); per-pair Gauss-Newton calls with one source per target are merged, anything else runs at once"""
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        self._call(self.lib.tcsfm_refine_dense_window_queued(self._h, C.byref(opts), B, S, self._p(tgt), self._p(srcs), self._p(depth_t), self._p(depth_s),
                                                             self._p(K), self._p(pose), self._p(pose_out), self._p(depth_out)))

    def flush(self):
        self._call(self.lib.tcsfm_flush(self._h))

    def coalesce_counts(self):
        """(launch sequences issued, calls they carried)"""
        b, c = C.c_int(0), C.c_int(0)
        self._call(self.lib.tcsfm_coalesce_counts(self._h, C.byref(b), C.byref(c)))
        return b.value, c.value

    def refine_window_async(self, lane: int, tgt, srcs, depth_t, depth_s, K, pose, pose_out, opts: Opts, log_scale=None, log_scale_out=None):
        """tcsfm_refine_window on `lane`, zero-allocation and asynchronous: tensors must be validated / contiguous float32 CUDA
        tensors in the window layout (see refine_window); the lane waits for the work queued on this engine's stream so far.
        Outputs are valid for consumers on this engine's stream after lane_wait(lane), for the host after lane_synchronize(lane)."""
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        self._call(self.lib.tcsfm_refine_window_async(self._h, int(lane), C.byref(opts), B, S, self._p(tgt), self._p(srcs), self._p(depth_t),
                                                      self._p(depth_s), self._p(K), self._p(pose), self._p(log_scale), self._p(pose_out),
                                                      self._p(log_scale_out), None))

    def refine_dense_window_async(self, lane: int, tgt, srcs, depth_t, depth_s, K, pose, pose_out, depth_out, opts: Opts):
        """tcsfm_refine_dense_window on `lane` (see refine_window_async: validated contiguous float32 CUDA tensors, no allocation;
        pose_out [2SB,6], depth_out [2SB,1,H,W])"""
        S, B = int(srcs.shape[0]), int(srcs.shape[1])
        self._call(self.lib.tcsfm_refine_dense_window_async(self._h, int(lane), C.byref(opts), B, S, self._p(tgt), self._p(srcs), self._p(depth_t),
                                                            self._p(depth_s), self._p(K), self._p(pose), self._p(pose_out), self._p(depth_out), None))

    def attach_depthnet(self, net):
        """tcsfm_sequence_depthnet: `net` (a loaded DepthNetHIP of this engine; None detaches) computes the depths of refine_sequence,
        refine_dense_sequence and PoseNetHIP.odometry_sequence calls that pass depths=None -- on the device, frame by frame as the
        frames land, the bits of Engine.disp_to_depth(net.forward(frames), opts.min_depth, opts.max_depth)[1].  The engine keeps a
        reference to `net` while it is attached."""
        if net is not None and (getattr(net, "eng", None) is not self or not getattr(net, "_dn", None)):
            raise ValueError("attach_depthnet: needs a DepthNetHIP of this engine (or None)")
        self._call(self.lib.tcsfm_sequence_depthnet(self._h, None if net is None else net._dn))
        self._seq_depthnet = net

    def _seq_depths(self, depths, T):
        """the `depths` argument of a sequence call: a checked CPU tensor, or None where an attached depth network stands in"""
        if depths is None:
            net = getattr(self, "_seq_depthnet", None)
            if net is None or not getattr(net, "_dn", None):
                raise ValueError("depths=None needs a depth network: call Engine.attach_depthnet(DepthNetHIP) first")
            return None
        return self._cpu(depths, (T, 1, self.H, self.W), "depths")

    def _seq_frames(self, frames, T, source_size=None):
        """the `frames` argument of a sequence call, checked before anything touches the GPU -> (contiguous CPU tensor, frame format).
        source_size=(h, w): camera-size bytes, [T,h,w,3] or [T,3,h,w] (tcsfm_sequence_frame_source)"""
        frames = torch.as_tensor(frames)
        if source_size is not None:
            return frames.contiguous(), source_frame_format(frames, source_size)
        fmt = frame_format(frames, self.H, self.W)
        if fmt == _lib.FRAMES_F32_CHW:
            return self._cpu(frames, (T, 3, self.H, self.W), "frames"), fmt
        return frames.contiguous(), fmt

    @contextlib.contextmanager
    def _frame_format(self, fmt):
        """the handle reads `frames` as `fmt` for the one call inside the block, and as float32 again afterwards, whatever happens"""
        if fmt == _lib.FRAMES_F32_CHW:
            yield
            return
        self._call(self.lib.tcsfm_sequence_frame_format(self._h, int(fmt)))
        try:
            yield
        finally:
            self.lib.tcsfm_sequence_frame_format(self._h, _lib.FRAMES_F32_CHW)

    @contextlib.contextmanager
    def _frame_source(self, source_size):
        """the handle reads `frames` at the camera's size for the one call inside the block, and at H x W again afterwards"""
        if source_size is None:
            yield
            return
        h, w = (int(v) for v in source_size)
        self._call(self.lib.tcsfm_sequence_frame_source(self._h, h, w))
        try:
            yield
        finally:
            self.lib.tcsfm_sequence_frame_source(self._h, 0, 0)

    @contextlib.contextmanager
    def _cam_height(self, cam_height, T):
        """the scale stage (tcsfm_sequence_scale) is on, at this camera height, for the one call inside the block, and off again afterwards"""
        self._seq_scale_T = 0
        if cam_height is None:
            yield
            return
        self._call(self.lib.tcsfm_sequence_scale(self._h, float(cam_height)))
        try:
            yield
            self._seq_scale_T = int(T)
        finally:
            self.lib.tcsfm_sequence_scale(self._h, 0.0)

    @contextlib.contextmanager
    def _disparity(self, mode, T):
        """the disparity stage (tcsfm_sequence_disparity) is on, in this mode, for the one call inside the block, and off again afterwards"""
        self._seq_disp = None
        if mode == _lib.SEQ_DISP_OFF:
            yield
            return
        self._call(self.lib.tcsfm_sequence_disparity(self._h, int(mode)))
        try:
            yield
            self._seq_disp = (int(T), int(mode))
        finally:
            self.lib.tcsfm_sequence_disparity(self._h, _lib.SEQ_DISP_OFF)

    def sequence_disparities(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """tcsfm_sequence_disparities: frames first .. first + count - 1 (count=None: to the last) of the disparities the last sequence
        call kept with disparity= -> NumPy [count,H,W]: float32 for "plain" (disp_to_depth's scaled_disp of the network's output),
        float64 for "post" (helpers.get_disp_for_eigen of every frame: np.concatenate of the driver's pred_disps).  Raises when that call
        kept nothing."""
        T, mode = getattr(self, "_seq_disp", None) or (0, _lib.SEQ_DISP_POST)
        first = int(first)
        count = max(T - first, 1) if count is None else int(count)
        out = np.empty((max(count, 1), self.H, self.W), dtype=np.float64 if mode == _lib.SEQ_DISP_POST else np.float32)
        got = C.c_int(0)
        self._call(self.lib.tcsfm_sequence_disparities(self._h, T, first, count, out.ctypes.data_as(C.c_void_p), C.byref(got)))
        assert got.value == mode
        return out

    def depth_eval(self, disp: torch.Tensor, gt: torch.Tensor, protocol="eigen", median_scaling: bool = True, min_depth: float = 1e-3,
                   max_depth: float = 80.0, depth_unit: float = 30.0, lds_pairs: int = -1) -> torch.Tensor:
        """tcsfm_depth_eval: the per-frame evaluation of paper_plots_and_data/evaluate_depth_eigen.py on the device.  disp [N,H,W] (or
        [N,1,H,W]) float32 or float64 CUDA: disparity planes at the engine's size; gt [N,gt_h,gt_w] float32 CUDA -> float64 [N,10]:
        abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, n_valid, n_median per frame (include/tcsfm.h); on the engine's stream"""
        if not isinstance(disp, torch.Tensor) or not disp.is_cuda or disp.dtype not in (torch.float32, torch.float64):
            raise TypeError("disp must be a float32 or float64 CUDA tensor")
        N = int(disp.shape[0])
        d = disp.reshape(N, self.H, self.W).contiguous()
        if gt.dim() != 3:
            raise AssertionError("wrong size for gt, expected {}xgt_hxgt_w, got  {}".format(N, list(gt.shape)))
        g = _chk(gt, (N, int(gt.shape[1]), int(gt.shape[2])), "gt")
        self._bind()
        out = torch.empty((N, _lib.NEVAL), dtype=torch.float64, device=d.device)
        o, e = default_opts(), _lib.depth_eval_opts(protocol, median_scaling, min_depth, max_depth, depth_unit, lds_pairs)
        self._call(self.lib.tcsfm_depth_eval(self._h, C.byref(o), C.byref(e), N, int(d.dtype == torch.float64), self._p(d), int(g.shape[1]),
                                             int(g.shape[2]), self._p(g), self._p(out)))
        return out

    def sequence_depth_eval(self, gt: np.ndarray, first: int = 0, protocol="eigen", median_scaling: bool = True, min_depth: float = 1e-3,
                            max_depth: float = 80.0, depth_unit: float = 30.0, lds_pairs: int = -1) -> np.ndarray:
        """tcsfm_sequence_depth_eval: frames first .. first + len(gt) - 1 of the disparities the last sequence call kept with disparity=
        ("plain" or "post"), evaluated on the device against gt, NumPy float32 [count,gt_h,gt_w] of ONE size -> NumPy float64 [count,10]
        as depth_eval's.  The planes do not leave the device.  Raises when that call kept nothing."""
        gt = np.ascontiguousarray(gt, dtype=np.float32)
        if gt.ndim != 3 or gt.shape[0] < 1:
            raise ValueError(f"gt must be [count,gt_h,gt_w] with count >= 1 (got {list(gt.shape)})")
        T = (getattr(self, "_seq_disp", None) or (0, 0))[0]
        out = np.empty((gt.shape[0], _lib.NEVAL), dtype=np.float64)
        e = _lib.depth_eval_opts(protocol, median_scaling, min_depth, max_depth, depth_unit, lds_pairs)
        self._call(self.lib.tcsfm_sequence_depth_eval(self._h, C.byref(e), T, int(first), int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2]),
                                                      gt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def flip_ramp(self, W: Optional[int] = None) -> np.ndarray:
        """tcsfm_flip_ramp: l_mask of batch_post_process_disparity for width W (default: the engine's), float64 [W] with the bits of
        1.0 - np.clip(20 * (np.linspace(0, 1, W) - 0.05), 0, 1).  Host only."""
        W = int(self.W if W is None else W)
        out = np.empty(max(W, 1), dtype=np.float64)
        if _lib.load().tcsfm_flip_ramp(W, out.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError(f"flip_ramp: W must be at least 2 (got {W})")
        return out

    def disp_post_process(self, l_disp: torch.Tensor, r_disp_mirrored: torch.Tensor) -> torch.Tensor:
        """tcsfm_disp_post_process: batch_post_process_disparity on the device.  l_disp [N,H,W] (or [N,1,H,W]) float32 CUDA: the frames'
        scaled disparity; r_disp_mirrored: the mirrored frames', STILL mirrored (the kernel un-flips it) -> float64 [N,H,W], NumPy's bits
        of the reference's expression; on the engine's stream"""
        N = int(l_disp.shape[0])
        l = _chk(l_disp.reshape(N, self.H, self.W), (N, self.H, self.W), "l_disp")
        r = _chk(r_disp_mirrored.reshape(N, self.H, self.W), (N, self.H, self.W), "r_disp_mirrored")
        self._bind()
        out = torch.empty((N, self.H, self.W), dtype=torch.float64, device=l.device)
        o = default_opts()
        self._call(self.lib.tcsfm_disp_post_process(self._h, C.byref(o), N, self._p(l), self._p(r), self._p(out)))
        return out

    def sequence_scales(self, T: Optional[int] = None):
        """tcsfm_sequence_scales: the per-frame scales of the last sequence call that ran with cam_height= -> dict(scale [T] float32,
        median [T] float32, count [T] int32) of CPU tensors, by frame index; a frame without ground pixels has NaN scale and median.
        Window w's metric factor is depth_unit * scale[w + tp] (streaming.metric_poses).  Raises when that call kept nothing."""
        T = int(getattr(self, "_seq_scale_T", 0) if T is None else T)
        scale = torch.empty(max(T, 1), dtype=torch.float32); med = torch.empty_like(scale); count = torch.empty(max(T, 1), dtype=torch.int32)
        hp = lambda t: C.c_void_p(t.data_ptr())
        self._call(self.lib.tcsfm_sequence_scales(self._h, T, hp(scale), hp(med), hp(count)))
        return dict(scale=scale[:T], median=med[:T], count=count[:T])

    def resize_u8(self, frames_u8: torch.Tensor, source_layout: str = "hwc", out: str = "f32") -> torch.Tensor:
        """tcsfm_resize_u8: uint8 CUDA frames at the camera's size, [N,h,w,3] (source_layout "hwc") or [N,3,h,w] ("chw"), -> the engine's
        H x W with the bytes of Pillow's Image.resize((W, H), Image.LANCZOS): out="u8" in the source's layout, out="f32" as float32
        [N,3,H,W] = bytes / 255 (what the window entries read); on the engine's stream"""
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise TypeError("resize_u8 takes a uint8 CUDA tensor [N,h,w,3] or [N,3,h,w]")
        if source_layout not in ("hwc", "chw") or out not in ("f32", "u8"):
            raise ValueError("source_layout must be 'hwc' or 'chw', out 'f32' or 'u8'")
        shape = tuple(frames_u8.shape)
        hwc = source_layout == "hwc"
        if shape[3 if hwc else 1] != 3:
            raise TypeError(f"{source_layout} frames must be {'[N,h,w,3]' if hwc else '[N,3,h,w]'} (got {list(shape)})")
        n, (h, w) = shape[0], (shape[1:3] if hwc else shape[2:4])
        fmt = _lib.FRAMES_U8_HWC if hwc else _lib.FRAMES_U8_CHW
        self._bind()
        src = frames_u8.contiguous()
        if out == "f32":
            dst, dfmt = torch.empty((n, 3, self.H, self.W), dtype=torch.float32, device=src.device), _lib.FRAMES_F32_CHW
        else:
            dst, dfmt = torch.empty((n, self.H, self.W, 3) if hwc else (n, 3, self.H, self.W), dtype=torch.uint8, device=src.device), fmt
        o = default_opts()
        self._call(self.lib.tcsfm_resize_u8(self._h, C.byref(o), fmt, int(n), int(h), int(w), self._p(src), dfmt, self._p(dst)))
        return dst

    def scale_intrinsics(self, K, source_size) -> np.ndarray:
        """tcsfm_scale_intrinsics: the camera's K [3,3] at source_size=(h, w) -> float32 K of the engine's H x W frames, as the reference's
        loaders scale it (K[0] *= W / w; K[1] *= H / h in double).  Host only."""
        h, w = (int(v) for v in source_size)
        Ks = np.ascontiguousarray(np.asarray(K, dtype=np.float32).reshape(3, 3))
        out = np.empty((3, 3), dtype=np.float32)
        rc = _lib.load().tcsfm_scale_intrinsics(h, w, int(self.H), int(self.W), Ks.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"scale_intrinsics: source_size {(h, w)} must be positive")
        return out

    def frames_from_u8(self, u8: torch.Tensor) -> torch.Tensor:
        """tcsfm_frames_from_u8: uint8 CUDA frames [N,3,H,W] or [N,H,W,3] (interleaved RGB) -> float32 [N,3,H,W], the correctly rounded
        u8 / 255 of the reference's ArrayToTensor, for callers of the window entries; on the engine's stream"""
        if not isinstance(u8, torch.Tensor) or not u8.is_cuda or u8.dtype != torch.uint8:
            raise TypeError("frames_from_u8 takes a uint8 CUDA tensor")
        shape = tuple(u8.shape)
        if len(shape) == 4 and shape[1:] == (3, self.H, self.W):
            fmt = _lib.FRAMES_U8_CHW
        elif len(shape) == 4 and shape[1:] == (self.H, self.W, 3):
            fmt = _lib.FRAMES_U8_HWC
        else:
            raise TypeError(f"uint8 frames must be [N,3,{self.H},{self.W}] or [N,{self.H},{self.W},3] (got {list(shape)})")
        self._bind()
        u8 = u8.contiguous()
        out = torch.empty((shape[0], 3, self.H, self.W), dtype=torch.float32, device=u8.device)
        o = default_opts()
        self._call(self.lib.tcsfm_frames_from_u8(self._h, C.byref(o), fmt, int(shape[0]), self._p(u8), self._p(out)))
        return out

    def refine_sequence(self, frames: torch.Tensor, depths: Optional[torch.Tensor], K, init_poses, opts: Optional[Opts] = None, sources: int = 1,
                        ring: int = 0, log_scale: bool = False, windows_per_call: int = 0, target_pos: int = 0, source_size=None, cam_height=None,
                        disparity=None):
        """tcsfm_refine_sequence: the whole window loop of a sequence inside the library (frames [T,3,H,W] float32 -- or the camera's
        bytes, uint8 [T,3,H,W] / [T,H,W,3], converted to u8 / 255 on the device -- / depths [T,1,H,W] CPU
        tensors -- pinned for asynchronous copies --, K [3,3], init_poses [T-S, 2S, 6]) -> refined poses [T-S, 2S, 6] (CPU tensor;
        with log_scale=True also the log depth scales [T-S, 2S]); calls of `windows_per_call` windows (0 = default 8, capped by max_pairs / 2S) run on
        the engine's lanes.  Window w = frames w .. w+S; its target is frame w + target_pos (0: the first; -1: the middle one, (S+1)//2, as
        the reference's loaders choose it), its sources the others in order.  depths=None: the depth network of attach_depthnet
        computes them inside the call.  source_size=(h, w): `frames` are the camera's bytes at ITS size, uint8 [T,h,w,3] or [T,3,h,w]; the
        library resizes them to H x W on the device with Pillow's Lanczos bytes (tcsfm_sequence_frame_source); K is the H x W frames'
        (Engine.scale_intrinsics).  cam_height=h (metres / depth unit; None: off): every frame's DNet ground-plane scale is computed from
        the ring's own depth plane inside the call (tcsfm_sequence_scale); fetch them with Engine.sequence_scales().  disparity="plain" /
        "post" (depths=None only): every frame's scaled disparity / flip-post-processed disparity (helpers.get_disp_for_eigen) is kept on
        the device inside the call (tcsfm_sequence_disparity); fetch them with Engine.sequence_disparities().  The return values are unchanged."""
        cam_height = check_cam_height(cam_height)
        disp_mode = check_disparity(disparity)
        T, S = int(frames.shape[0]), int(sources)
        depths = self._seq_depths(depths, T)
        frames, fmt = self._seq_frames(frames, T, source_size)
        self._bind()
        o = opts or default_opts()
        cpu = lambda a, shape, name: self._cpu(a, shape, name)
        Kc = cpu(torch.as_tensor(np.asarray(K, dtype=np.float32)), (3, 3), "K")
        p0 = cpu(torch.as_tensor(np.asarray(init_poses, dtype=np.float32)), (T - S, 2 * S, 6), "init_poses")
        out = torch.empty_like(p0)
        ls = torch.zeros((T - S, 2 * S), dtype=torch.float32) if log_scale else None
        hp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with self._frame_format(fmt), self._frame_source(source_size), self._cam_height(cam_height, T), self._disparity(disp_mode, T):
            self._call(self.lib.tcsfm_refine_sequence(self._h, C.byref(o), T, S, hp(frames), hp(depths), hp(Kc), hp(p0), hp(out), hp(ls), int(ring),
                                                      int(windows_per_call), int(target_pos)))
        return (out, ls) if log_scale else out

    def refine_dense_sequence(self, frames: torch.Tensor, depths: Optional[torch.Tensor], K, init_poses, opts: Optional[Opts] = None, sources: int = 1,
                              ring: int = 0, windows_per_call: int = 0, target_pos: int = 0, out_depths: Optional[torch.Tensor] = None,
                              source_size=None, cam_height=None, disparity=None):
        """tcsfm_refine_dense_sequence: the dense mode (pose + per-pixel inverse depth) over a sequence, arguments as refine_sequence
        -> (poses [T-S, 2S, 6], refined depth maps [T-S, 2S, 1, H, W]) as CPU tensors.
        out_depths: a caller-owned (pinned) CPU tensor of that shape to receive the depth maps; a caller that runs sequence after
        sequence should pass one -- pinning a fresh 70 MB result buffer costs ten times the refinement of a 120-frame sequence.
        source_size=(h, w): camera-size bytes, as for refine_sequence.  cam_height: per-frame scales, as for refine_sequence.
        disparity: the frames' disparities, as for refine_sequence."""
        cam_height = check_cam_height(cam_height)
        disp_mode = check_disparity(disparity)
        T, S = int(frames.shape[0]), int(sources)
        depths = self._seq_depths(depths, T)
        frames, fmt = self._seq_frames(frames, T, source_size)
        self._bind()
        o = opts or default_opts()
        Kc = self._cpu(torch.as_tensor(np.asarray(K, dtype=np.float32)), (3, 3), "K")
        p0 = self._cpu(torch.as_tensor(np.asarray(init_poses, dtype=np.float32)), (T - S, 2 * S, 6), "init_poses")
        out = torch.empty_like(p0)
        if out_depths is None:      # pinned: the copies back run beside the kernels
            dout = torch.empty((T - S, 2 * S, 1, self.H, self.W), dtype=torch.float32, pin_memory=True)
        else:
            dout = out_depths
            if dout.is_cuda or dout.dtype != torch.float32 or not dout.is_contiguous() or tuple(dout.shape) != (T - S, 2 * S, 1, self.H, self.W):
                raise TypeError("out_depths must be a contiguous float32 CPU tensor [T-S, 2S, 1, H, W]")
        hp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with self._frame_format(fmt), self._frame_source(source_size), self._cam_height(cam_height, T), self._disparity(disp_mode, T):
            self._call(self.lib.tcsfm_refine_dense_sequence(self._h, C.byref(o), T, S, hp(frames), hp(depths), hp(Kc), hp(p0), hp(out), hp(dout), int(ring),
                                                            int(windows_per_call), int(target_pos)))
        return out, dout

    @staticmethod
    def _cpu(t, shape, name):
        t = torch.as_tensor(t)
        if t.is_cuda or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 CPU tensor (pinned for asynchronous copies)")
        if tuple(t.shape) != tuple(shape):
            raise AssertionError("wrong size for {}, expected {}, got  {}".format(name, "x".join(map(str, shape)), list(t.shape)))
        return t.contiguous()

    def lane_wait(self, lane: int):
        self._call(self.lib.tcsfm_lane_wait(self._h, int(lane)))

    def lane_event(self, lane: int):
        """mark the current end of the lane's work -> opaque event handle for stream_wait_event"""
        ev = C.c_void_p()
        self._call(self.lib.tcsfm_lane_event(self._h, int(lane), C.byref(ev)))
        return ev

    def stream_wait_event(self, stream: "torch.cuda.Stream", event):
        """make a torch stream wait (on the device) for a lane_event mark"""
        self._call(self.lib.tcsfm_stream_wait_event(self._h, C.c_void_p(stream.cuda_stream), event))

    def lane_synchronize(self, lane: int):
        self._call(self.lib.tcsfm_lane_synchronize(self._h, int(lane)))

    def refine_into(self, tgt, src, depth_t, depth_s, K, pose_in, pose_out, opts: Opts, log_scale_in=None, log_scale_out=None,
                    stats_out=None):
        """Zero-allocation variant used by bench.py: tensors must already be validated/contiguous; pose_out may alias pose_in."""
        self._call(self.lib.tcsfm_refine(self._h, C.byref(opts), tgt.shape[0], self._p(tgt), self._p(src), self._p(depth_t),
                                         self._p(depth_s), self._p(K), self._p(pose_in), self._p(log_scale_in), self._p(pose_out),
                                         self._p(log_scale_out), self._p(stats_out)))


# -- SE(3) host utilities (liegroups stand-ins; double precision, no GPU needed) ---------------------
def _vec(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(n)
    return a, a.ctypes.data_as(C.c_void_p)


def pose_to_matrix(pose) -> np.ndarray:
    a, pa = _vec(pose, 6); T = np.zeros(12); _lib.load().tcsfm_pose_to_matrix(pa, T.ctypes.data_as(C.c_void_p)); return T.reshape(3, 4)


def matrix_to_pose(T) -> np.ndarray:
    a, pa = _vec(T, 12); p = np.zeros(6); _lib.load().tcsfm_matrix_to_pose(pa, p.ctypes.data_as(C.c_void_p)); return p


def se3_exp(xi) -> np.ndarray:
    a, pa = _vec(xi, 6); T = np.zeros(12); _lib.load().tcsfm_se3_exp(pa, T.ctypes.data_as(C.c_void_p)); return T.reshape(3, 4)


def se3_log(T) -> np.ndarray:
    a, pa = _vec(T, 12); x = np.zeros(6); _lib.load().tcsfm_se3_log(pa, x.ctypes.data_as(C.c_void_p)); return x


def se3_mul(A, B) -> np.ndarray:
    a, pa = _vec(A, 12); b, pb = _vec(B, 12); c = np.zeros(12)
    _lib.load().tcsfm_se3_mul(pa, pb, c.ctypes.data_as(C.c_void_p)); return c.reshape(3, 4)


def se3_inv(A) -> np.ndarray:
    a, pa = _vec(A, 12); b = np.zeros(12); _lib.load().tcsfm_se3_inv(pa, b.ctypes.data_as(C.c_void_p)); return b.reshape(3, 4)
