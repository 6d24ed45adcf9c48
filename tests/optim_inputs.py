"""Inputs and judge of the device optimiser's tests (csrc/optim_kernel.h, tcsfm_optim_*), shared by tests/test_optim_inputs_cpu.py and
tests/test_gpu_optim.py.

INPUTS (build(seed)).  One float32 arena with the tensors laid end to end behind a one-float lead, so pointers are only 4-byte aligned
and the 16-byte phase changes from tensor to tensor.  Sizes: numel in {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 70001}
(below / at / above the group of four, the wave, the block's 256 threads, half a chunk, two chunks, 35 chunks), then 300 tensors of
random size 1..97: more tensors than any per-launch table would hold, a work item each.  Parameters are randn * 10^U(-6,0).  Gradients
for K = 6 steps are +-10^U(-10,0) (g * g >= 1e-20: no fp32 subnormal arises), 5 % of them exact zeros, and the first 100 elements of the
big tensor have gradient zero at every step.  The gradient arenas of the even steps (2, 4, 6) have a two-float lead: there a gradient's
16-byte phase differs from its parameter's.  Tensor NONE_TENSOR (numel 4099) has grad = None at steps 2 and 4.  Two parameter groups:
lr 2e-4 (the reference's value, run_sequential_optimization.py) and 1e-2 (every third tensor).

JUDGE (judge(...)).  torch.optim.Adam / SGD (foreach=False) on float64 CPU copies, K steps.  With p0 the starting value and p64, m64, v64
the float64 results, per element:
    |p - p64| <= K (ulp32(max(|p0|, |p64|) + K lr) + 16 2^-24 lr)     one rounding of p per step, whose magnitude never exceeds
                                                                     max(|p0|, |p64|) + K lr (an Adam step moves p by at most ~lr,
                                                                     an SGD step by lr |g| <= lr), plus the update's rounding chain:
                                                                     a dozen fp32 roundings of a quantity of size <= lr
    |m - m64| <= 4 2^-24 max_t |g_t|                                 m stays below max |g|; g - m, the product, the sum and the
                                                                     once-rounded 1 - beta1 each contribute at most 2^-24 of that
    |v - v64| <= 2^-24 max_t g_t^2                                   v stays below K (1 - beta2) max g^2 = 0.006 max g^2
step counts equal, and where every gradient a tensor's element saw was zero, p keeps its bits.  The bounds come from the formats, not from
any implementation; test_optim_inputs_cpu.py checks that torch's own fp32 Adam / SGD pass them (the inputs are fair) and that a step with
a wrong bias correction or a lost tail element does not (they bite)."""
import numpy as np
import torch

K = 6
HEAD_SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 70001]
N_SMALL = 300
BIG_TENSOR = HEAD_SIZES.index(70001)
NONE_TENSOR = HEAD_SIZES.index(4099)
NONE_STEPS = (2, 4)                      # 1-based
LRS = (2e-4, 1e-2)
BETAS, EPS = (0.9, 0.999), 1e-8


def _layout(sizes, lead):
    offs, at = [], lead
    for n in sizes:
        offs.append(at)
        at += n
    return offs, at


def build(seed=0):
    """-> dict: sizes, offsets, p_arena [float32], g_arenas [K float32 arenas], g_offsets [K], present [K][n] bool, lr [n]"""
    gen = torch.Generator().manual_seed(1000 + seed)
    sizes = HEAD_SIZES + [int(x) for x in torch.randint(1, 98, (N_SMALL,), generator=gen)]
    n = len(sizes)
    offs, total = _layout(sizes, 1)
    p = torch.zeros(total + 3, dtype=torch.float32)
    body = torch.randn(total - 1, generator=gen, dtype=torch.float64) * 10.0 ** (-6.0 * torch.rand(total - 1, generator=gen, dtype=torch.float64))
    p[1:total] = body.float()
    g_arenas, g_offsets, present = [], [], []
    for k in range(K):
        lead = 1 if k % 2 == 0 else 2        # steps 2, 4, 6 (k = 1, 3, 5): another 16-byte phase than the parameters'
        go, gt = _layout(sizes, lead)
        mag = 10.0 ** (-10.0 * torch.rand(gt - lead, generator=gen, dtype=torch.float64))
        sign = torch.where(torch.rand(gt - lead, generator=gen) < 0.5, -1.0, 1.0).double()
        g = (mag * sign).float()
        g[torch.rand(gt - lead, generator=gen) < 0.05] = 0.0
        b = go[BIG_TENSOR] - lead
        g[b:b + 100] = 0.0
        arena = torch.zeros(gt + 3, dtype=torch.float32)
        arena[lead:gt] = g
        g_arenas.append(arena)
        g_offsets.append(go)
        present.append([not (i == NONE_TENSOR and (k + 1) in NONE_STEPS) for i in range(n)])
    lr = [LRS[1] if i % 3 == 1 else LRS[0] for i in range(n)]
    return dict(sizes=sizes, offsets=offs, p_arena=p, g_arenas=g_arenas, g_offsets=g_offsets, present=present, lr=lr)


def params_of(inp, arena=None):
    a = inp["p_arena"] if arena is None else arena
    return [a[o:o + n] for o, n in zip(inp["offsets"], inp["sizes"])]


def grads_of(inp, k, arena=None):
    """gradients of step k (0-based): views into the step's arena, None where the tensor has no gradient"""
    a = inp["g_arenas"][k] if arena is None else arena
    return [(a[o:o + n] if ok else None) for o, n, ok in zip(inp["g_offsets"][k], inp["sizes"], inp["present"][k])]


def torch_run(inp, kind, dtype, steps=K):
    """torch.optim.Adam / SGD (foreach=False) on CPU copies of `dtype` -> (params, exp_avg, exp_avg_sq, step counts)"""
    ps = [torch.nn.Parameter(p.detach().clone().to(dtype)) for p in params_of(inp)]
    groups = [{"params": [q for q, l in zip(ps, inp["lr"]) if l == lr], "lr": lr} for lr in LRS]
    opt = (torch.optim.Adam(groups, betas=BETAS, eps=EPS, foreach=False) if kind == "adam" else torch.optim.SGD(groups, foreach=False))
    counts = [0] * len(ps)
    for k in range(steps):
        for i, (q, g) in enumerate(zip(ps, grads_of(inp, k))):
            q.grad = None if g is None else g.detach().clone().to(dtype)
            counts[i] += g is not None
        opt.step()
    m = [opt.state[q].get("exp_avg", torch.zeros_like(q)) if kind == "adam" else None for q in ps]
    v = [opt.state[q].get("exp_avg_sq", torch.zeros_like(q)) if kind == "adam" else None for q in ps]
    if kind == "adam":
        counts = [int(opt.state[q]["step"]) if "step" in opt.state[q] else 0 for q in ps]
    return [q.detach() for q in ps], m, v, counts


def plain_run(inp, kind, wrong=None, steps=K):
    """the kernel's arithmetic, element-wise in fp32 torch on the CPU (scalars computed in double, rounded once); `wrong`: None, 'no_bc2'
    (the second bias correction left out) or 'tail' (the last element of every tensor is never updated) -> as torch_run"""
    f = lambda x: torch.tensor(x, dtype=torch.float64).float()
    ps = [p.detach().clone() for p in params_of(inp)]
    m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    counts = [0] * len(ps)
    b1, b2 = BETAS
    for k in range(steps):
        for i, g in enumerate(grads_of(inp, k)):
            if g is None:
                continue
            counts[i] += 1
            t = counts[i]
            sl = slice(0, max(ps[i].numel() - 1, 0)) if wrong == "tail" else slice(None)
            p_, g_, m_, v_ = ps[i][sl], g[sl], m[i][sl], v[i][sl]
            if kind == "adam":
                a, b = f(inp["lr"][i] / (1.0 - b1 ** t)), f(1.0 if wrong == "no_bc2" else (1.0 - b2 ** t) ** 0.5)
                m_.copy_(m_ + f(1.0 - b1) * (g_ - m_))
                v_.copy_(f(b2) * v_ + (f(1.0 - b2) * g_) * g_)
                p_.copy_(p_ - a * (m_ / (v_.sqrt() / b + f(EPS))))
            else:
                p_.copy_(p_ - f(inp["lr"][i]) * g_)
    return ps, (m if kind == "adam" else [None] * len(ps)), (v if kind == "adam" else [None] * len(ps)), counts


def _ulp32(x64):
    x = x64.float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))).double() - x.double())


_REF = {}


def reference(inp_seed, inp, kind, steps=K):
    """the float64 result, computed once per (seed, kind, steps) and shared"""
    key = (inp_seed, kind, steps)
    if key not in _REF:
        _REF[key] = torch_run(inp, kind, torch.float64, steps)
    return _REF[key]


def judge(inp, kind, ref, params, exp_avg, exp_avg_sq, counts, steps=K):
    """params / exp_avg / exp_avg_sq: lists of CPU float32 tensors (moments None for SGD), counts: list of int; ref = reference(...)
    -> dict(ok, failures [str], p / m / v: the largest |error| / bound seen)"""
    p64, m64, v64, c64 = ref
    p0 = params_of(inp)
    worst, fails = {"p": 0.0, "m": 0.0, "v": 0.0}, []
    for i, n in enumerate(inp["sizes"]):
        if counts[i] != c64[i]:
            fails.append(f"tensor {i}: step count {counts[i]}, expected {c64[i]}")
        if n == 0:
            continue
        gs = [g for g in (grads_of(inp, k)[i] for k in range(steps)) if g is not None]
        gmax = torch.stack([g.double().abs() for g in gs]).max(0).values if gs else torch.zeros(n, dtype=torch.float64)
        lr = inp["lr"][i]
        p = params[i].detach().cpu().reshape(-1)
        bound = steps * (_ulp32(torch.maximum(p0[i].double().abs(), p64[i].abs()) + steps * lr) + 16 * 2.0 ** -24 * lr)
        err = (p.double() - p64[i]).abs()
        worst["p"] = max(worst["p"], float((err / bound).max()))
        if bool((err > bound).any()) or not bool(torch.isfinite(p).all()):
            j = int((err / bound).argmax())
            fails.append(f"tensor {i} (numel {n}) element {j}: p {float(p[j]):.9e} float64 {float(p64[i][j]):.9e} bound {float(bound[j]):.3e}")
        still = gmax == 0
        if bool(still.any()) and not torch.equal(p[still].view(torch.int32), p0[i][still].view(torch.int32)):
            fails.append(f"tensor {i}: an element whose gradients were all zero changed")
        if kind != "adam":
            continue
        for name, got, want, bnd in (("m", exp_avg[i], m64[i], 4 * 2.0 ** -24 * gmax), ("v", exp_avg_sq[i], v64[i], 2.0 ** -24 * gmax * gmax)):
            e = (got.detach().cpu().reshape(-1).double() - want).abs()
            ratio = torch.where(bnd > 0, e / bnd.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
            worst[name] = max(worst[name], float(ratio.max()))
            if bool((e > bnd).any()):
                j = int(ratio.argmax())
                fails.append(f"tensor {i} (numel {n}) element {j}: {name} {float(got.reshape(-1)[j]):.9e} float64 {float(want[j]):.9e} bound {float(bnd[j]):.3e}")
    return dict(ok=not fails, failures=fails, **worst)
