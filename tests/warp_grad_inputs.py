"""Inputs, float64 reference and judging rules of the warp's backward pass (tcsfm_warp_backward, stn.inverse_warp2 under autograd),
shared by tests/test_warp_grad_inputs_cpu.py and tests/test_gpu_warp_grad.py.  No GPU here.

REFERENCE.  Autograd through oracle.torch_twin.warp in torch.float64, called with -pose as the call sites do; the fp32 yardstick is
the same function in torch.float32 (tests/test_warp_grad_golden_cpu.py ties the twin's gradients to the reference's own).

CASES.  operator_inputs.make_case (every item of a batch differs): less than one 256-thread block, two ragged sizes with odd
widths, 100x333, the production size, and 19 items on an Engine made for 24; each at the ground-truth poses and at 30 times those,
where most samples leave the frame and many pixels sit in the Z clamp.

COTANGENTS.  Seeded normal maps with a different scale per item and per map (a scatter that used item 0's or a fixed fixed-point
scale is caught), zero on the TIE MASK: the gradient of a bilinear sample is discontinuous at cell borders, so fp32 and float64 may
legitimately disagree there.  Masked are the pixels whose float64 sample position lies within TIE_PX of a cell border in x or y,
whose projected position lies within TIE_PX of the frame edges 0, W-1, H-1, or whose p2 is within TIE_Z of the clamp 1e-3.
1e-3 px covers an fp32 evaluation of the pixel coordinate at these widths (ulp at ~600 is 6e-5, times a handful of operations).
The masked share of an item's frame is capped (mask_cap) and the float32 twin must take the float64 cell at every unmasked valid
pixel: tests/test_warp_grad_inputs_cpu.py asserts both for every case, so an input that breaks them is reported as a bad input.

JUDGING.  Per item and per tensor (d_depth_t, d_depth_s, d_pose): relative L2 error and max error over RMS against float64.  Pass
when each is at most MARGIN = 4 times the float32 twin's figure on the same inputs and cotangents (the project's margin: two bits
for contraction and ordering) AND the relative L2 is below REL_L2_MAX = 1e-4 (what the suite asserts for continuous arithmetic
elsewhere); where the reference is exactly zero the result must be exactly zero.
"""
import functools

import numpy as np
import torch

import operator_inputs as OI
from oracle import torch_twin as tw

MARGIN = OI.MARGIN
REL_L2_MAX = 1e-4
TIE_PX, TIE_Z = 1e-3, 1e-6
SHAPES = [(5, 9, 3), (17, 33, 3), (37, 53, 3), (100, 333, 2), (192, 640, 2)]
MANY, MANY_MAX_PAIRS = OI.MANY, OI.MANY_MAX_PAIRS
POSE_SCALES = (1.0, 30.0)
CASES = [(H, W, N, s) for (H, W, N) in SHAPES + [MANY] for s in POSE_SCALES]
IDS = [f"{H}x{W}-N{N}-pose_x{s:g}" for (H, W, N, s) in CASES]
TENSORS = ("d_depth_t", "d_depth_s", "d_pose")
COTS = ("g_rec", "g_pd", "g_cd")
SUBSETS = [COTS, ("g_rec",), ("g_pd",), ("g_cd",)]

make_case = OI.make_case


def mask_cap(hw):
    return max(2, int(0.015 * hw))


def _T(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


def geometry(c, dt=torch.float64):
    """the twin's sample geometry (oracle.torch_twin.warp, pose = -c['pose']) -> numpy [N, H*W]: ix, iy (grid_sample's pixel
    coordinates), xp, yp (projected position), p2 (depth before the clamp)"""
    N, _, H, W = c["src"].shape
    K, pose, d_t = _T(c["K"], dt), _T(c["pose"], dt), _T(c["depth_t"], dt)
    v, u = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    pix = torch.stack([u, v, torch.ones_like(u)], 0).view(1, 3, -1)
    cam = (torch.inverse(K) @ pix) * d_t.view(N, 1, -1)
    P = K @ tw.pose_matrix(-pose)
    pc = P[:, :, :3] @ cam + P[:, :, 3:]
    Z = pc[:, 2].clamp(min=1e-3)
    xp, yp = pc[:, 0] / Z, pc[:, 1] / Z
    xn, yn = 2 * xp / (W - 1) - 1, 2 * yp / (H - 1) - 1
    ix, iy = ((xn + 1) * W - 1) / 2, ((yn + 1) * H - 1) / 2
    f = lambda t: t.double().numpy()
    return dict(ix=f(ix), iy=f(iy), xp=f(xp), yp=f(yp), p2=f(pc[:, 2]), valid=f(((xn.abs() <= 1) & (yn.abs() <= 1)).to(dt)) > 0.5)


@functools.lru_cache(maxsize=None)
def tie_mask(case):
    """-> (mask [N, H*W] bool, float64 geometry)"""
    H, W, N, s = case
    g = geometry(make_case(*case))
    frac = lambda a: np.minimum(a - np.floor(a), np.ceil(a) - a)
    near = (frac(g["ix"]) < TIE_PX) | (frac(g["iy"]) < TIE_PX)
    near |= (np.abs(g["xp"]) < TIE_PX) | (np.abs(g["xp"] - (W - 1)) < TIE_PX) | (np.abs(g["yp"]) < TIE_PX) | (np.abs(g["yp"] - (H - 1)) < TIE_PX)
    near |= np.abs(g["p2"] - 1e-3) < TIE_Z
    return near, g


def cell_flips32(case):
    """unmasked, valid pixels at which the float32 twin takes another bilinear cell than float64 -> count"""
    near, g = tie_mask(case)
    g32 = geometry(make_case(*case), torch.float32)
    flip = (np.floor(g32["ix"]) != np.floor(g["ix"])) | (np.floor(g32["iy"]) != np.floor(g["iy"]))
    return int((flip & g["valid"] & ~near).sum())


@functools.lru_cache(maxsize=None)
def cotangents(case):
    """-> dict g_rec [N,3,H,W], g_pd, g_cd [N,1,H,W] float32, zero on the tie mask; item n of map m is scaled by 10^((((3 n + 2 m) % 7) - 3) / 2)"""
    H, W, N, s = case
    rng = np.random.default_rng(9000 + 7 * H + W + N + int(s))
    near = tie_mask(case)[0].reshape(N, 1, H, W)
    out = {}
    for m, (k, ch) in enumerate((("g_rec", 3), ("g_pd", 1), ("g_cd", 1))):
        g = rng.standard_normal((N, ch, H, W))
        for n in range(N):
            g[n] *= 10.0 ** ((((3 * n + 2 * m) % 7) - 3) / 2)
        out[k] = np.ascontiguousarray(np.where(near, 0.0, g), np.float32)
    return out


@functools.lru_cache(maxsize=None)
def twin(case, subset=COTS, dtype="f64"):
    """autograd through oracle.torch_twin.warp with the cotangents of `subset` (the others absent) -> dict of float64 numpy arrays:
    d_depth_t, d_depth_s [N,1,H,W], d_pose [N,6] (gradient with respect to c['pose']; the warp is called with -pose), and the forward's
    rec, valid, proj_depth, comp_depth.  Computed once per (case, subset, dtype) and shared: treat as read-only."""
    dt = torch.float64 if dtype == "f64" else torch.float32
    c, cot = make_case(*case), cotangents(case)
    src, K = _T(c["src"], dt), _T(c["K"], dt)
    d_t, d_s, pose = (_T(c[k], dt).requires_grad_() for k in ("depth_t", "depth_s", "pose"))
    rec, valid, pd, cd = tw.warp(src, d_t, d_s, -pose, K)
    outs = dict(g_rec=rec, g_pd=pd, g_cd=cd)
    L = sum((outs[k] * _T(cot[k], dt)).sum() for k in subset)
    L.backward()
    z = lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy()
    f = lambda t: t.detach().double().numpy()
    return dict(d_depth_t=z(d_t), d_depth_s=z(d_s), d_pose=z(pose), rec=f(rec), valid=f(valid), proj_depth=f(pd), comp_depth=f(cd))


def errors(got, ref):
    """one item's tensor against float64 -> (relative L2 error, max error over the reference's RMS); (0, 0) for an all-zero reference
    that is matched exactly, (inf, inf) for one that is not"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    d = got - ref
    nrm = float(np.linalg.norm(ref))
    if nrm == 0.0:
        return (0.0, 0.0) if not d.any() else (float("inf"), float("inf"))
    return float(np.linalg.norm(d)) / nrm, float(np.abs(d).max()) / (nrm / np.sqrt(ref.size))


def judge(got, ref, t32, tag, report=None):
    """got / ref / t32: dicts with TENSORS ([N, ...] arrays): the result under test, the float64 twin and the float32 twin
    -> (failures, figures).  failures: list of (tag, tensor, item, criterion, value, bound); figures: {tensor: worst ratio to the float32
    twin's error over the items, both measures}.  `report`: called with one line per tensor and item, before anything is judged."""
    fails, worst = [], {}
    for k in TENSORS:
        N = ref[k].shape[0]
        for n in range(N):
            g, r = np.asarray(got[k][n], np.float64), ref[k][n]
            zero_bad = int(((r == 0) & (g != 0)).sum())
            (l2, mx), (l2_32, mx_32) = errors(g, r), errors(t32[k][n], r)
            ratio = max(l2 / l2_32 if l2_32 > 0 else (0.0 if l2 == 0 else float("inf")), mx / mx_32 if mx_32 > 0 else (0.0 if mx == 0 else float("inf")))
            if report:
                report(f"{tag}\t{k}[{n}]\trel_l2={l2:.3e}\tf32={l2_32:.3e}\tmax/rms={mx:.3e}\tf32={mx_32:.3e}\tratio={ratio:.3f}\tnonzero_at_exact_zero={zero_bad}")
            worst[k] = max(worst.get(k, 0.0), ratio)
            if zero_bad:
                fails.append((tag, k, n, "exact zero", zero_bad, 0))
            if not l2 <= MARGIN * l2_32:
                fails.append((tag, k, n, "rel_l2 vs 4 x f32", l2, MARGIN * l2_32))
            if not mx <= MARGIN * mx_32:
                fails.append((tag, k, n, "max/rms vs 4 x f32", mx, MARGIN * mx_32))
            if not l2 < REL_L2_MAX:
                fails.append((tag, k, n, "rel_l2 < 1e-4", l2, REL_L2_MAX))
    return fails, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# planted faults, made at numpy level from the true float64 gradient (tests/test_warp_grad_inputs_cpu.py: the judge rejects each)
def x_path_gradient(case, subset=COTS):
    """the part of the float64 gradient that flows through the sample's x coordinate -> dict d_depth_t, d_pose (what a dropped
    W / (W - 1) scales): the twin's warp with the y coordinate of the grid detached"""
    dt = torch.float64
    c, cot = make_case(*case), cotangents(case)
    N, _, H, W = c["src"].shape
    src, ref_depth, K = _T(c["src"], dt), _T(c["depth_s"], dt), _T(c["K"], dt)
    d_t, pose = (_T(c[k], dt).requires_grad_() for k in ("depth_t", "pose"))
    v, u = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    pix = torch.stack([u, v, torch.ones_like(u)], 0).view(1, 3, -1)
    cam = (torch.inverse(K) @ pix) * d_t.view(N, 1, -1)
    P = K @ tw.pose_matrix(-pose)
    pc = P[:, :, :3] @ cam + P[:, :, 3:]
    Z = pc[:, 2].clamp(min=1e-3)
    xn, yn = 2 * (pc[:, 0] / Z) / (W - 1) - 1, (2 * (pc[:, 1] / Z) / (H - 1) - 1).detach()
    xn = torch.where(xn.detach().abs() > 1, torch.full_like(xn, 2.0), xn)
    yn = torch.where(yn.abs() > 1, torch.full_like(yn, 2.0), yn)
    grid = torch.stack([xn, yn], 2).view(N, H, W, 2)
    F = torch.nn.functional
    L = 0
    if "g_rec" in subset:
        L = L + (F.grid_sample(src, grid, padding_mode="zeros", align_corners=False) * _T(cot["g_rec"], dt)).sum()
    if "g_pd" in subset:
        L = L + (F.grid_sample(ref_depth, grid, padding_mode="zeros", align_corners=False) * _T(cot["g_pd"], dt)).sum()
    L.backward()
    return dict(d_depth_t=d_t.grad.numpy(), d_pose=pose.grad.numpy())


def planted_faults(case):
    """-> {name: (faulty gradient dict, tensors the fault must be caught on)} from the float64 gradient with all three cotangents"""
    H, W, N, s = case
    ref, cot = twin(case), cotangents(case)
    near, g = tie_mask(case)
    true = {k: ref[k].copy() for k in TENSORS}
    out = {}
    # 1. d ix / d (X/Z) taken as 1 instead of W / (W - 1)
    xg = x_path_gradient(case)
    f = {k: v.copy() for k, v in true.items()}
    for k in ("d_depth_t", "d_pose"):
        f[k] = true[k] - xg[k] / W            # x part scaled by (W - 1) / W
    out["w_factor_dropped"] = (f, ("d_depth_t", "d_pose"))
    # 2. one tap weight of the scatter swapped (w00 <-> w01) at every unmasked valid pixel
    f = {k: v.copy() for k, v in true.items()}
    gp = cot["g_pd"].reshape(N, -1).astype(np.float64)
    for n in range(N):
        sel = g["valid"][n] & ~near[n]
        ix, iy = g["ix"][n][sel], g["iy"][n][sel]
        x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
        wx, wy = ix - x0, iy - y0
        delta = gp[n][sel] * ((1 - wx) * (1 - wy) - wx * (1 - wy))        # w00 - w01: what tap 01 gains and tap 00 loses
        flat = f["d_depth_s"][n].reshape(-1)
        in00, in01 = (x0 >= 0) & (y0 >= 0) & (y0 < H), (x0 + 1 < W) & (y0 >= 0) & (y0 < H)
        np.add.at(flat, (y0 * W + x0)[in00], -delta[in00])
        np.add.at(flat, (y0 * W + x0 + 1)[in01], delta[in01])
    out["tap_weight_swapped"] = (f, ("d_depth_s",))
    # 3. the g_comp_depth path dropped on out-of-frame pixels (all that flows there)
    f = {k: v.copy() for k, v in true.items()}
    f["d_depth_t"] = np.where(ref["valid"] == 0, 0.0, true["d_depth_t"])
    out["g_cd_dropped_out_of_frame"] = (f, ("d_depth_t",))
    # 4. the sign of d_pose flipped
    f = {k: v.copy() for k, v in true.items()}
    f["d_pose"] = -true["d_pose"]
    out["d_pose_sign"] = (f, ("d_pose",))
    # 5. item 0's gradient returned for every item
    f = {k: np.repeat(v[:1], N, 0) for k, v in true.items()}
    out["item0_for_all"] = (f, TENSORS)
    # 6. the clamp ignored: g_comp_depth passes through Z at clamped pixels
    f = {k: v.copy() for k, v in true.items()}
    clamped = (g["p2"] < 1e-3).reshape(N, 1, H, W)
    f["d_depth_t"] = np.where(clamped, true["d_depth_t"] + cot["g_cd"].astype(np.float64), true["d_depth_t"])
    out["clamp_ignored"] = (f, ("d_depth_t",))
    return out
