"""Inputs, float64 reference and judging rules of the backward passes of disp_to_depth, SSIM_Loss and get_smooth_loss
(tcsfm_disp_to_depth_backward, tcsfm_ssim_backward, tcsfm_smooth_loss_device / _backward and the three drop-ins under autograd), shared
by tests/test_loss_grad_inputs_cpu.py and tests/test_gpu_loss_grad.py.  No GPU here.

REFERENCE.  Autograd in torch.float64 through the reference's own expressions: 1 / (a + b disp) (utils/learning_helpers.py:77-86),
oracle.torch_twin.ssim, and the torch body of tightly_coupled_sfm_amd.losses.get_smooth_loss (CPU tensors take it).  The yardstick is
the same code in torch.float32.

CASES.  (H, W, N) = (2, 2, 1) -- reflect padding of 1 is legal there --, (4, 4, 1), (5, 9, 3), (17, 33, 3), (37, 53, 3) and
(192, 640, 2).  A handle cannot be created below 4 x 4 (tcsfm_create refuses, and tests/test_abi_cpu.py pins that), so 2 x 2 is
checked at the level of the closed forms only (tests/test_loss_grad_inputs_cpu.py) and 4 x 4 is the smallest frame on the GPU.
Disparities are sigmoid-range, differ per item and sit on a grid of 1 / 4096: two neighbours are equal or differ by far more than
TIE in both precisions.  Each map holds a constant patch, whose edge differences are exactly zero: sgn(0) = 0 is pinned.  For SSIM x
is the disparity and a second textured plane (C = 2), y is x plus a perturbation; item 0 has a small region with y = x, where the
value sits at the clamp's lower edge.

COTANGENTS.  Seeded normal maps, one scale per item and per map as photo_grad_inputs.cotangents.  SSIM: zero where the float64 value
(1 - SSIM) / 2 is within TIE of 0 or 1 without being exactly there, or where the float32 twin gates otherwise than float64.  The smooth
loss has ONE scalar cotangent, nothing can be masked: smooth_input_report counts the edges on which float32 and float64 disagree in
sign and the non-zero |delta n| below TIE, and the CPU test asserts both are zero.

JUDGING.  photo_grad_inputs.judge: per item and tensor the relative L2 error and the max error over RMS each at most MARGIN = 4 times
the float32 twin's figure, exact zeros where float64 is exactly zero, relative L2 below REL_L2_MAX = 1e-4.
"""
import functools

import numpy as np
import torch

import photo_grad_inputs as PG
from oracle import torch_twin as tw
from tightly_coupled_sfm_amd import losses

WG = PG.WG
MARGIN, REL_L2_MAX, TIE = PG.MARGIN, PG.REL_L2_MAX, PG.TIE
errors, judge, mask_cap = WG.errors, PG.judge, PG.mask_cap
CASES = [(2, 2, 1), (4, 4, 1), (5, 9, 3), (17, 33, 3), (37, 53, 3), (192, 640, 2)]
IDS = [f"{H}x{W}-N{N}" for (H, W, N) in CASES]
F64_CASES, LARGE = CASES[:-1], CASES[-1]           # every cotangent subset | all cotangents once
GPU_CASES = [c for c in CASES if min(c[:2]) >= 4]  # tcsfm_create refuses frames below 4 x 4 (tests/test_abi_cpu.py pins that)
MIN_DEPTH, MAX_DEPTH = 0.06, 2.67
SSIM_C = 2
D2D_COTS, SSIM_OUTS = ("g_scaled", "g_depth"), ("g_x", "g_y")
D2D_SUBSETS = [D2D_COTS, ("g_scaled",), ("g_depth",)]
SSIM_WANTS = [SSIM_OUTS, ("g_x",), ("g_y",)]
SMOOTH_G = 1.7                                      # the scalar cotangent of the smooth loss


def _T(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


def _dt(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def _scale(n, m):
    return 10.0 ** ((((3 * n + 2 * m) % 7) - 3) / 2)


def patch(H, W):
    """the constant patch of every disparity map -> (r0, r1, c0, c1); at H = 2 one row of two pixels, else at least 2 x 2"""
    r0, c0 = H // 3, W // 3
    return r0, r0 + (1 if H == 2 else max(2, H // 3)), c0, c0 + max(2, W // 3)


@functools.lru_cache(maxsize=None)
def make_disp(case):
    """-> disp [N,1,H,W] float32 in (0.03, 0.97), multiples of 1 / 4096: a ramp and noise, another mix per item, a constant patch"""
    H, W, N = case
    rng = np.random.default_rng(4200 + 11 * H + W + N)
    v, u = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.empty((N, 1, H, W))
    r0, r1, c0, c1 = patch(H, W)
    for n in range(N):
        d = 0.15 + (0.25 + 0.1 * n) * (0.6 * v + 0.4 * u) + (0.3 - 0.08 * n) * rng.uniform(0, 1, (H, W))
        d[r0:r1, c0:c1] = 0.4 + 0.05 * n
        out[n, 0] = np.round(d * 4096) / 4096
    assert out.min() > 0.03 and out.max() < 0.97
    return np.ascontiguousarray(out, np.float32)


@functools.lru_cache(maxsize=None)
def make_img(case):
    H, W, N = case
    return np.ascontiguousarray(np.random.default_rng(4300 + 5 * H + W + N).uniform(0, 1, (N, 3, H, W)), np.float32)


def same_region(H, W):
    """the region of item 0 where y = x -> (r0, r1, c0, c1): off the border, so that (r1 - r0 - 2) (c1 - c0 - 2) windows lie inside it
    -- at most mask_cap(H W); one pixel in a frame too small for that"""
    if H < 5 or W < 5:
        return 0, 1, 0, 1
    rh = min(4, H - 2)
    return 1, 1 + rh, 1, 1 + min(W - 2, 2 + mask_cap(H * W) // (rh - 2))


@functools.lru_cache(maxsize=None)
def make_ssim(case):
    """-> x, y [N,2,H,W] float32: x = (the disparity, a textured plane), y = x + a perturbation of +-(0.03 .. 0.12) per pixel"""
    H, W, N = case
    rng = np.random.default_rng(4400 + 3 * H + W + N)
    x = np.concatenate([make_disp(case).astype(np.float64), rng.uniform(0.1, 0.9, (N, 1, H, W))], 1)
    y = x + rng.choice([-1.0, 1.0], x.shape) * rng.uniform(0.03, 0.12, x.shape)
    r0, r1, c0, c1 = same_region(H, W)
    y[0, :, r0:r1, c0:c1] = x[0, :, r0:r1, c0:c1]
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# disp_to_depth
@functools.lru_cache(maxsize=None)
def d2d_cotangents(case):
    H, W, N = case
    rng = np.random.default_rng(9200 + 7 * H + W + N)
    out = {}
    for m, k in enumerate(D2D_COTS):
        g = rng.standard_normal((N, 1, H, W))
        for n in range(N):
            g[n] *= _scale(n, m)
        out[k] = np.ascontiguousarray(g, np.float32)
    return out


def d2d_gradient(disp, cot, dtype="f64", power=2):
    """autograd through scaled = a + b disp, depth = 1 / scaled (`power` = 1: the planted fault g_depth / s) -> dict g_disp"""
    dt = _dt(dtype)
    d = _T(disp, dt).requires_grad_()
    lo, hi = 1 / MAX_DEPTH, 1 / MIN_DEPTH
    s = lo + (hi - lo) * d
    depth = 1 / s if power == 2 else -torch.log(s)
    outs = dict(g_scaled=s, g_depth=depth)
    sum((outs[k] * _T(cot[k], dt)).sum() for k in cot).backward()
    return dict(g_disp=d.grad.double().numpy())


@functools.lru_cache(maxsize=None)
def twin_d2d(case, subset=D2D_COTS, dtype="f64"):
    """computed once per (case, subset, dtype) and shared: treat as read-only"""
    cot = d2d_cotangents(case)
    return d2d_gradient(make_disp(case), {k: cot[k] for k in subset}, dtype)


def d2d_closed_form(disp, cot):
    d = np.asarray(disp, np.float64)
    lo, hi = 1 / MAX_DEPTH, 1 / MIN_DEPTH
    s = lo + (hi - lo) * d
    return (hi - lo) * (np.asarray(cot.get("g_scaled", 0.0), np.float64) - np.asarray(cot.get("g_depth", 0.0), np.float64) / s ** 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# SSIM
@functools.lru_cache(maxsize=None)
def ssim_mask(case):
    """-> (ties, flips) [N,C,H,W] bool: float64 value within TIE of 0 or 1 but not exactly there | the float32 twin gates otherwise"""
    x, y = make_ssim(case)
    v64 = PG.ssim_raw(_T(x, torch.float64), _T(y, torch.float64)).numpy()
    v32 = PG.ssim_raw(_T(x, torch.float32), _T(y, torch.float32)).double().numpy()
    ties = ((np.abs(v64) < TIE) & (v64 != 0)) | ((np.abs(v64 - 1) < TIE) & (v64 != 1))
    gate = lambda v: (v >= 0) & (v <= 1)
    return ties, (gate(v64) != gate(v32)) & ~ties


@functools.lru_cache(maxsize=None)
def ssim_cotangent(case):
    """-> g_out [N,C,H,W] float32, zero on the mask; item n of plane c is scaled by 10^((((3 n + 2 c) % 7) - 3) / 2)"""
    H, W, N = case
    ties, flips = ssim_mask(case)
    g = np.random.default_rng(9300 + 7 * H + W + N).standard_normal((N, SSIM_C, H, W))
    for n in range(N):
        for c in range(SSIM_C):
            g[n, c] *= _scale(n, c)
    return np.ascontiguousarray(np.where(ties | flips, 0.0, g), np.float32)


def ssim_gradient(x, y, g_out, want=SSIM_OUTS, dtype="f64"):
    """autograd through torch_twin.ssim -> dict g_x, g_y (only those in `want`)"""
    dt = _dt(dtype)
    xs, ys = _T(x, dt).requires_grad_("g_x" in want), _T(y, dt).requires_grad_("g_y" in want)
    (tw.ssim(xs, ys) * _T(g_out, dt)).sum().backward()
    return {k: t.grad.double().numpy() for k, t in (("g_x", xs), ("g_y", ys)) if k in want}


@functools.lru_cache(maxsize=None)
def twin_ssim(case, dtype="f64"):
    """computed once per (case, dtype) and shared: treat as read-only"""
    return ssim_gradient(*make_ssim(case), ssim_cotangent(case), SSIM_OUTS, dtype)


def _refl(i, n):
    i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return np.clip(i, 0, n - 1)


def ssim_closed_form(x, y, g_out, side="g_y", multiplicity=True, closed=True):
    """the kernel's formula at numpy level (float64): sum over the windows q and their nine reflected taps of g_out[q] dv_q / d(tap)
    as a scatter (the multiplicity arises by itself; False: only unreflected taps count, m = 1).  `closed` False: the planted fault
    of a clamp that passes on the OPEN interval only."""
    x, y, g = (np.asarray(a, np.float64) for a in (x, y, g_out))
    if side == "g_x":
        x, y = y, x
    N, C, H, W = x.shape
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    taps = [(_refl(vv + dv, H), _refl(uu + du, W), dv, du) for dv in (-1, 0, 1) for du in (-1, 0, 1)]
    xs, ys = np.stack([x[:, :, a, b] for a, b, _, _ in taps]), np.stack([y[:, :, a, b] for a, b, _, _ in taps])
    mx, my = xs.mean(0), ys.mean(0)
    sx, sy, sxy = (xs * xs).mean(0) - mx * mx, (ys * ys).mean(0) - my * my, (xs * ys).mean(0) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + 1e-4, 2 * sxy + 9e-4, mx * mx + my * my + 1e-4, sx + sy + 9e-4
    s = A1 * A2 / (B1 * B2)
    v = (1 - s) / 2
    k = np.where(((v >= 0) & (v <= 1)) if closed else ((v > 0) & (v < 1)), g * -0.5, 0.0)
    out = np.zeros_like(y)
    nn, cc = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    for i, (a, b, dv, du) in enumerate(taps):
        ds = ((2 * mx * A2 + 2 * (xs[i] - mx) * A1) / (B1 * B2) - s * (2 * my / B1 + 2 * (ys[i] - my) / B2)) / 9
        ok = True if multiplicity else ((vv + dv >= 0) & (vv + dv < H) & (uu + du >= 0) & (uu + du < W))
        np.add.at(out, (nn[:, :, None, None], cc[:, :, None, None], a[None, None], b[None, None]), np.where(ok, k * ds, 0.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# smooth loss
def smooth_gradient(disp, img, g=SMOOTH_G, dtype="f64"):
    """autograd through losses.get_smooth_loss's torch body (CPU tensors) -> (dict g_disp, the loss as a float)"""
    dt = _dt(dtype)
    d = _T(disp, dt).requires_grad_()
    L = losses.get_smooth_loss(d, _T(img, dt))
    (L * g).backward()
    return dict(g_disp=d.grad.double().numpy()), float(L.detach())


@functools.lru_cache(maxsize=None)
def twin_smooth(case, dtype="f64"):
    """computed once per (case, dtype) and shared: treat as read-only"""
    return smooth_gradient(make_disp(case), make_img(case), SMOOTH_G, dtype)[0]


def smooth_input_report(disp):
    """-> (edges on which the float32 and the float64 sign of delta n disagree, edges with 0 < |delta n| < TIE in either precision)"""
    bad_sign = near = 0
    deltas = []
    for dt in (torch.float64, torch.float32):
        d = _T(disp, dt)
        n = d / (d.mean(2, True).mean(3, True) + 1e-7)
        deltas.append([(n[:, :, :, :-1] - n[:, :, :, 1:]).double().numpy(), (n[:, :, :-1, :] - n[:, :, 1:, :]).double().numpy()])
    for a, b in zip(*deltas):
        bad_sign += int((np.sign(a) != np.sign(b)).sum())
        near += int((((np.abs(a) > 0) & (np.abs(a) < TIE)) | ((np.abs(b) > 0) & (np.abs(b) < TIE))).sum())
    return bad_sign, near


def smooth_closed_form(disp, img, g=SMOOTH_G, mean_term=True, sgn0=0.0):
    """the kernel's formula at numpy level (float64) -> (g_disp [N,1,H,W], l_n [N], sum_j g_n[j] n_j [N]).  `mean_term` False and
    `sgn0` = 1 are the planted faults (the coupling through the mean dropped; sgn(0) taken as 1)."""
    d, im = np.asarray(disp, np.float64), np.asarray(img, np.float64)
    N, _, H, W = d.shape
    m = d.mean((2, 3), keepdims=True) + 1e-7
    n = d / m
    wx = np.exp(-np.abs(im[:, :, :, :-1] - im[:, :, :, 1:]).mean(1, keepdims=True))
    wy = np.exp(-np.abs(im[:, :, :-1, :] - im[:, :, 1:, :]).mean(1, keepdims=True))
    dx, dy = n[:, :, :, :-1] - n[:, :, :, 1:], n[:, :, :-1, :] - n[:, :, 1:, :]
    sgn = lambda a: np.where(a == 0, sgn0, np.sign(a))
    Nx, Ny = N * H * (W - 1), N * (H - 1) * W
    gn = np.zeros_like(d)
    gn[:, :, :, :-1] += sgn(dx) * wx / Nx; gn[:, :, :, 1:] -= sgn(dx) * wx / Nx
    gn[:, :, :-1, :] += sgn(dy) * wy / Ny; gn[:, :, 1:, :] -= sgn(dy) * wy / Ny
    ln = (np.abs(dx) * wx).sum((1, 2, 3)) / Nx + (np.abs(dy) * wy).sum((1, 2, 3)) / Ny
    coupling = (gn * n).sum((1, 2, 3))
    out = g * (gn - (ln.reshape(N, 1, 1, 1) / (H * W) if mean_term else 0.0)) / m
    return out, ln, coupling


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: 17 x 33, B = 1, S = 2 (tests/test_gpu_loss_grad.py::test_end_to_end_optimization_loss)
E2E_CASE = (17, 33, 2, 1.0)
E2E_DEPTH_RANGE = (0.1, 100.0)
E2E_OPTIONS = dict(num_source_imgs=2, diff_img_argmin=False, automasking=False, l_inverse_reconstruction=True, l_depth_consist=True,
                   l_depth_consist_weight=0.15, l_depth_init=True, l_depth_init_weight=0.1, l_smooth=True, l_smooth_weight=0.05,
                   l_pose_consist=False)
E2E_TENSORS = ("d_disp_t", "d_disp_s")


@functools.lru_cache(maxsize=None)
def e2e_inputs():
    """one target (item 0's) and the two sources of PG.make_case(17, 33, 2, 1.0) -> dict of float32 arrays: tgt [1,3,H,W], src [2,3,H,W],
    disp_t [1,1,H,W], disp_s [2,1,H,W] (the case's depths as sigmoid disparities of E2E_DEPTH_RANGE), disp_init [1,1,H,W] (the target
    disparity times 1 +- 5..15 %), pose [2,6], K [2,3,3]"""
    c = PG.make_case(*E2E_CASE)
    lo, hi = 1 / E2E_DEPTH_RANGE[1], 1 / E2E_DEPTH_RANGE[0]
    to_disp = lambda depth: (1 / depth.astype(np.float64) - lo) / (hi - lo)
    disp_t, disp_s = to_disp(c["depth_t"][:1]), to_disp(c["depth_s"])
    assert 0 < min(disp_t.min(), disp_s.min()) and max(disp_t.max(), disp_s.max()) < 1
    rng = np.random.default_rng(4500)
    init = disp_t * (1 + rng.choice([-1.0, 1.0], disp_t.shape) * rng.uniform(0.05, 0.15, disp_t.shape))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(tgt=f(c["tgt"][:1]), src=f(c["src"]), disp_t=f(disp_t), disp_s=f(disp_s), disp_init=f(init), pose=f(c["pose"]),
                K=f(np.repeat(c["K"][:1], 2, 0)))


def e2e_twin(masks, dtype="f64", inputs=None, options=None, depth_range=None, hooks=None):
    """the chain of the GPU test in torch on the CPU: disparity leaves -> 1 / (a + b disp) -> torch_twin.photometric for the forward
    and the inverse pairs -> losses.compute_optimization_loss (its CPU path) with E2E_OPTIONS and torch_twin.ssim; `masks`: the
    library's valid_mask (validity x auto-mask, as helpers.compute_photometric_error returns it) of both directions, detached (dict
    fwd_valid, inv_valid, numpy [2,1,H,W]).  `inputs` (default e2e_inputs()), `options` (default E2E_OPTIONS) and `depth_range`
    (default E2E_DEPTH_RANGE) let other chains reuse it (tests/tuning_chain_inputs.py).  `hooks`: {name: callable(tensor) -> tensor}
    applied to "repeat" (the repeated target depth) and "inv_ref_depth" (the same tensor as the inverse pairs take it): where planted
    faults cut or alter a path
    -> (dict d_disp_t, d_disp_s; the loss as a float)"""
    dt = _dt(dtype)
    i = e2e_inputs() if inputs is None else inputs
    options = E2E_OPTIONS if options is None else options
    hook = lambda name, t: (hooks or {}).get(name, lambda a: a)(t)
    disp_t, disp_s = _T(i["disp_t"], dt).requires_grad_(), _T(i["disp_s"], dt).requires_grad_()
    lo, hi = (1 / d for d in reversed(E2E_DEPTH_RANGE if depth_range is None else depth_range))
    depth = lambda d: 1 / (lo + (hi - lo) * d)
    tgt2, src, pose, K = _T(i["tgt"], dt).repeat(2, 1, 1, 1), _T(i["src"], dt), _T(i["pose"], dt), _T(i["K"], dt)
    dt2, ds = hook("repeat", depth(disp_t).repeat(2, 1, 1, 1)), depth(disp_s)
    fwd, inv = tw.photometric(tgt2, src, dt2, ds, pose, K), tw.photometric(src, tgt2, ds, hook("inv_ref_depth", dt2), -pose, K)
    pack = lambda r, valid, p: dict(diff_img=r["diff"], valid_mask=_T(valid, dt), weight_mask=r["weight"], poses=p)
    L = losses.compute_optimization_loss(options, tgt2[:1], disp_t, _T(i["disp_init"], dt), pack(fwd, masks["fwd_valid"], pose),
                                         pack(inv, masks["inv_valid"], -pose), tw.ssim)
    L.backward()
    return dict(d_disp_t=disp_t.grad.double().numpy(), d_disp_s=disp_s.grad.double().numpy()), float(L.detach())


def e2e_twin_masks(dtype="f64", inputs=None, depth_range=None):
    """the masks as the twin itself takes them (the CPU test: they are not empty) -> dict as `masks` of e2e_twin"""
    dt = _dt(dtype)
    i = e2e_inputs() if inputs is None else inputs
    lo, hi = (1 / d for d in reversed(E2E_DEPTH_RANGE if depth_range is None else depth_range))
    depth = lambda d: 1 / (lo + (hi - lo) * _T(d, dt))
    tgt2, src, pose, K = _T(i["tgt"], dt).repeat(2, 1, 1, 1), _T(i["src"], dt), _T(i["pose"], dt), _T(i["K"], dt)
    dt2, ds = depth(i["disp_t"]).repeat(2, 1, 1, 1), depth(i["disp_s"])
    fwd, inv = tw.photometric(tgt2, src, dt2, ds, pose, K), tw.photometric(src, tgt2, ds, dt2, -pose, K)
    return dict(fwd_valid=fwd["mask"].numpy(), inv_valid=inv["mask"].numpy())
