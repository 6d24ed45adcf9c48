"""The optimiser of the reference's weight-tuning loop on the HIP library: torch.optim.Adam / SGD as the reference builds them
(optimization_experiments/optimizer.py:211-214: `torch.optim.Adam(params)` / `torch.optim.SGD(params)` over parameter groups with their
own `lr`; :266-268: one `step()` per epoch) as ONE kernel launch over all tensors (csrc/optim_kernel.h, tcsfm_optim_*), and the
per-window reset of the tuned network -- the reference deep-copies it for every window (:176-191) -- as snapshot() / restore().

    opt = LibraryOptimizer([{"params": model.encoder.parameters(), "lr": 2e-4}], kind="adam")
    opt.snapshot()                       # once
    for window in windows:
        opt.restore()                    # parameters back to the snapshot's bits, moments and step counts zero
        for epoch in range(epochs):
            opt.zero_grad(); loss(model, window).backward(); opt.step()

step() and restore() write the parameters in place on the device and bump their version counters, so a DepthNetModule / PoseNetModule
re-folds them into its native network at its next forward, exactly as after a torch optimiser's step."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_KINDS = {"adam": _lib.OPTIM_ADAM, "sgd": _lib.OPTIM_SGD}
_engines = {}


def _default_engine(device_index):
    """a small handle per device: the optimiser needs a handle's stream and device, none of its image-sized scratch"""
    from .engine import Engine
    e = _engines.get(device_index)
    if e is None:
        with torch.cuda.device(device_index):
            e = _engines[device_index] = Engine(32, 32, 1, device=device_index)
    return e


class LibraryOptimizer:
    """`params_or_groups`: an iterable of tensors, or of dicts with `params` (a tensor or an iterable of tensors) and optionally `lr`, as
    torch.optim takes them.  kind 'adam' is torch.optim.Adam with weight_decay = 0 and amsgrad = False, 'sgd' is torch.optim.SGD
    without momentum or weight decay.  Parameters must be contiguous float32 tensors on the engine's device; `engine=None` uses a small
    engine of this module on the parameters' device.  `param_groups[k]['lr']` is read at every step (schedules work)."""

    def __init__(self, params_or_groups, kind="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, engine=None):
        if kind not in _KINDS:
            raise ValueError(f"LibraryOptimizer: kind {kind!r}: expected 'adam' or 'sgd'")
        if isinstance(params_or_groups, torch.Tensor):
            params_or_groups = [params_or_groups]
        groups = list(params_or_groups)
        if not groups:
            raise ValueError("LibraryOptimizer: got an empty parameter list")
        if not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.kind, self.betas, self.eps = kind, (float(betas[0]), float(betas[1])), float(eps)
        self.param_groups = []
        for g in groups:
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            self.param_groups.append(dict(g, params=ps, lr=float(g.get("lr", lr))))
        self._params = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise ValueError("LibraryOptimizer: got an empty parameter list")
        if len({id(p) for p in self._params}) != len(self._params):
            raise ValueError("LibraryOptimizer: a parameter appears in more than one group")
        dev = self._params[0].device
        if dev.type != "cuda":
            raise ValueError(f"LibraryOptimizer: parameters on {dev}: the step runs on the GPU")
        self.eng = engine if engine is not None else _default_engine(dev.index)
        for p in self._params:
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or dev.index != self.eng.device:
                raise ValueError("LibraryOptimizer: parameters must be contiguous float32 tensors on the engine's device "
                                 f"(cuda:{self.eng.device}); got {tuple(p.shape)} {p.dtype} on {p.device}")
        self._index = {id(p): i for i, p in enumerate(self._params)}
        n = len(self._params)
        self._numel = [int(p.numel()) for p in self._params]
        # an empty tensor has no data pointer and nothing of it is ever read: a present gradient is signalled by this address
        self._nonnull = torch.zeros(4, dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * n)(*[(p.data_ptr() or None) for p in self._params])
        self._ptrs = [p.data_ptr() for p in self._params]
        numel = (C.c_int64 * n)(*self._numel)
        self.lib = self.eng.lib
        o = C.c_void_p()
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_optim_create(self.eng._h, _KINDS[kind], n, ptrs, numel, C.byref(o)))
        self._o = o
        self.eng._adopt(self, self.lib.tcsfm_optim_destroy, o)
        self.has_snapshot = False

    def __del__(self):
        try:
            self.eng._release(self)
        except Exception:
            pass

    def _check_storage(self):
        for p, ptr in zip(self._params, self._ptrs):
            if p.data_ptr() != ptr:
                raise RuntimeError("LibraryOptimizer: a parameter's storage moved since the optimiser was created (`.data = ...`, `.to(...)`); "
                                   "build a new optimiser")

    def _bump(self):
        for p in self._params:
            torch.autograd.graph.increment_version(p)

    def zero_grad(self, set_to_none=True):
        for p in self._params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        """one optimiser step over every parameter that has a gradient (p.grad is None: skipped, its step count stays), asynchronous
        on torch's current stream"""
        self._check_storage()
        n = len(self._params)
        keep, gp, wrote = [], [], []
        for p, numel in zip(self._params, self._numel):
            g = p.grad
            if g is None:
                gp.append(None)
                continue
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.layout != torch.strided:
                g = (g.to_dense() if g.layout != torch.strided else g).to(device=p.device, dtype=torch.float32).contiguous()
            if g.numel() != numel:
                raise ValueError(f"LibraryOptimizer: gradient of shape {tuple(g.shape)} for a parameter of shape {tuple(p.shape)}")
            keep.append(g)
            gp.append(g.data_ptr() if numel else self._nonnull.data_ptr())
            wrote.append(p)
        grads = (C.c_void_p * n)(*gp)
        lr = (C.c_double * n)(*[float(g["lr"]) for g in self.param_groups for _ in g["params"]])
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_optim_step(self._o, grads, lr, self.betas[0], self.betas[1], self.eps))
        for p in wrote:
            torch.autograd.graph.increment_version(p)

    def snapshot(self):
        """keep a copy of every parameter's current values (on the device, owned by the library)"""
        self._check_storage()
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_optim_snapshot(self._o))
        self.has_snapshot = True

    def restore(self):
        """parameters back to the snapshot's bits, moments zero, step counts zero"""
        self._check_storage()
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_optim_restore(self._o))
        self._bump()

    def state(self, p):
        """{'step': int, 'exp_avg': tensor, 'exp_avg_sq': tensor} of parameter p, as copies (SGD keeps no moments: None)"""
        i = self._index[id(p)]
        step = C.c_int64(0)
        m = v = None
        if self.kind == "adam":
            m, v = torch.empty_like(p), torch.empty_like(p)
        self.eng._bind()
        self.eng._call(self.lib.tcsfm_optim_get_state(self._o, i, self.eng._p(m) if m is not None and m.numel() else None,
                                                      self.eng._p(v) if v is not None and v.numel() else None, C.byref(step)))
        return {"step": int(step.value), "exp_avg": m, "exp_avg_sq": v}
