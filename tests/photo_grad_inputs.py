"""Inputs, float64 reference and judging rules of the photometric assembly's backward pass (tcsfm_photometric_maps_backward,
tcsfm_photometric_backward, compute_photometric_error under autograd), shared by tests/test_photo_grad_inputs_cpu.py and
tests/test_gpu_photo_grad.py.  No GPU here.

REFERENCE.  MAPS: autograd through `assembly` (the two lines of oracle.torch_twin.photometric that turn (rec, proj_depth, comp_depth)
into diff and weight; the CPU test ties it to torch_twin.photometric bit for bit) in torch.float64.  Its leaves are the float64 twin's
warp outputs rounded to float32: the same numbers for the kernel, the float64 and the float32 twin.  CHAIN: autograd through
oracle.torch_twin.photometric in float64 with respect to depth_t, depth_s and pose.  The fp32 yardstick is the same code in float32.

CASES.  warp_grad_inputs.CASES as they are.

PHOTO TIE MASK (float64, TIE = 1e-6).  A pixel is masked when 0 < |rec - tgt| < TIE in a channel, or | |rec - tgt| - 1 | < TIE but not
0, or the SSIM value (1 - s) / 2 of a channel is within TIE of 0 or 1, or 0 < |r| < TIE, or | |r| - 1 | < TIE but not 0, with
r = (cd - pd) / (cd + pd).  Exact 0 and exact 1 are not ties: both precisions take them identically and torch's conventions (sgn(0) =
0, a clamp passes on the closed interval) decide them.  Pixels where the float32 twin decides otherwise than float64 -- sgn(rec - tgt),
sgn(r), which pixels sit at exact 1, the SSIM clamp and, in the chain, the bilinear cell -- join the mask.

COTANGENTS.  Seeded normal maps, a different scale per item and per map, zero on the mask; for the chain also zero on the warp's tie
mask (g_diff, g_weight and g_img_rec alike).  Zeroing the cotangent AT the tied pixel is enough for the assembly's decisions, each of
which is multiplied by its own pixel's cotangent.  The bilinear cell of pixel p is multiplied by g_rec[p], which g_diff feeds through
the 3 x 3 windows around p: where the float32 twin takes another cell than float64, g_diff is zero on the 3 x 3 neighbourhood.

JUDGING.  Per item and tensor as warp_grad_inputs.judge: relative L2 and max error over RMS each at most MARGIN = 4 times the float32
twin's figure, exact zeros where float64 is exactly zero, and (maps only) relative L2 below 1e-4.
"""
import functools

import numpy as np
import torch

import warp_grad_inputs as WG
from oracle import torch_twin as tw

CASES, IDS = WG.CASES, WG.IDS
MARGIN, REL_L2_MAX = WG.MARGIN, WG.REL_L2_MAX
TIE = 1e-6
W_L1, W_SSIM = 0.15, 0.85
MAP_TENSORS, MAP_COTS = ("g_rec", "g_pd", "g_cd"), ("g_diff", "g_weight")
CHAIN_TENSORS, CHAIN_COTS = WG.TENSORS, ("g_diff", "g_weight", "g_img_rec")
MAP_SUBSETS = [MAP_COTS, ("g_diff",), ("g_weight",)]
CHAIN_SUBSETS = [CHAIN_COTS, ("g_diff",), ("g_weight",), ("g_img_rec",)]
make_case, mask_cap = WG.make_case, WG.mask_cap


def _T(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


def _dt(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def assembly(tgt, rec, pd, cd, w_l1=W_L1, w_ssim=W_SSIM):
    """torch_twin.photometric's residual assembly on given warp outputs -> (diff, weight)"""
    diff = (w_l1 * (rec - tgt).abs().clamp(0, 1) + w_ssim * tw.ssim(tgt, rec)).mean(1, True)
    weight = 1 - ((cd - pd).abs() / (cd + pd)).clamp(0, 1)
    return diff, weight


def ssim_raw(x, y):
    """(1 - SSIM) / 2 before its clamp: torch_twin.ssim's expression"""
    F = torch.nn.functional
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mx, my = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x * x, 3, 1) - mx * mx
    sy = F.avg_pool2d(y * y, 3, 1) - my * my
    sxy = F.avg_pool2d(x * y, 3, 1) - mx * my
    n = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4)
    d = (mx * mx + my * my + 1e-4) * (sx + sy + 9e-4)
    return (1 - n / d) / 2


@functools.lru_cache(maxsize=None)
def leaves(case):
    """the float64 twin's warp outputs rounded to float32 -> dict tgt, rec [N,3,H,W], pd, cd [N,1,H,W] (float32 numpy)"""
    ref = WG.twin(case)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(tgt=make_case(*case)["tgt"], rec=f(ref["rec"]), pd=f(ref["proj_depth"]), cd=f(ref["comp_depth"]))


@functools.lru_cache(maxsize=None)
def _forward(case, mode, dtype):
    """the quantities the decisions are taken on -> dict of float64 numpy: d = rec - tgt [N,3,HW], v = raw SSIM value [N,3,HW],
    num = cd - pd, den = cd + pd [N,HW]"""
    dt = _dt(dtype)
    H, W, N, _ = case
    c = make_case(*case)
    if mode == "maps":
        l = leaves(case)
        tgt, rec, pd, cd = (_T(l[k], dt) for k in ("tgt", "rec", "pd", "cd"))
    else:
        tgt = _T(c["tgt"], dt)
        rec, _, pd, cd = tw.warp(_T(c["src"], dt), _T(c["depth_t"], dt), _T(c["depth_s"], dt), -_T(c["pose"], dt), _T(c["K"], dt))
    f = lambda t, ch: t.double().numpy().reshape(N, ch, H * W)
    return dict(d=f(rec - tgt, 3), v=f(ssim_raw(tgt, rec), 3), num=f(cd - pd, 1)[:, 0], den=f(cd + pd, 1)[:, 0])


def _decisions(q):
    """the discrete decisions of the assembly's backward, as integer codes per pixel"""
    r_abs = np.abs(q["num"]) / q["den"]
    return dict(sgn_d=np.sign(q["d"]), one_d=(np.abs(q["d"]) == 1), in_d=(np.abs(q["d"]) <= 1), gate=(q["v"] >= 0) & (q["v"] <= 1),
                sgn_r=np.sign(q["num"]), one_r=(r_abs == 1), in_r=(r_abs <= 1))


@functools.lru_cache(maxsize=None)
def photo_tie_mask(case, mode):
    """-> (ties [N,HW] bool: the float64 conditions; flips [N,HW] bool: pixels off the ties (and, in the chain, off the warp's tie
    mask) where the float32 twin decides otherwise; cell [N,HW] bool: chain only, valid pixels where float32 takes another cell)"""
    H, W, N, _ = case
    q = _forward(case, mode, "f64")
    ad = np.abs(q["d"])
    r = np.abs(q["num"]) / q["den"]
    ties = ((ad > 0) & (ad < TIE)).any(1) | ((np.abs(ad - 1) < TIE) & (ad != 1)).any(1)
    ties |= ((np.abs(q["v"]) < TIE) | (np.abs(q["v"] - 1) < TIE)).any(1)
    ties |= ((r > 0) & (r < TIE)) | ((np.abs(r - 1) < TIE) & (r != 1))
    a, b = _decisions(q), _decisions(_forward(case, mode, "f32"))
    flips = np.zeros((N, H * W), bool)
    for k in a:
        dif = a[k] != b[k]
        flips |= dif.any(1) if dif.ndim == 3 else dif
    cell = np.zeros((N, H * W), bool)
    known = ties.copy()
    if mode == "chain":
        near, g = WG.tie_mask(case)
        g32 = WG.geometry(make_case(*case), torch.float32)
        cell = ((np.floor(g32["ix"]) != np.floor(g["ix"])) | (np.floor(g32["iy"]) != np.floor(g["iy"]))) & g["valid"]
        known |= near
    return ties, flips & ~known, cell


@functools.lru_cache(maxsize=None)
def mask(case, mode):
    """-> dict of [N,HW] bool masks per cotangent: where it is zero"""
    H, W, N, _ = case
    ties, flips, cell = photo_tie_mask(case, mode)
    m = ties | flips
    if mode == "maps":
        return dict(g_diff=m, g_weight=m)
    m = m | WG.tie_mask(case)[0] | cell
    wide = np.stack([WG.OI.dilate3(cell[n].reshape(H, W)).reshape(-1) for n in range(N)]) if cell.any() else cell
    return dict(g_diff=m | wide, g_weight=m, g_img_rec=m)


@functools.lru_cache(maxsize=None)
def cotangents(case, mode):
    """-> dict g_diff, g_weight [N,1,H,W] (+ g_img_rec [N,3,H,W] for the chain), float32, zero on `mask`; item n of map m is scaled by
    10^((((3 n + 2 m) % 7) - 3) / 2)"""
    H, W, N, s = case
    rng = np.random.default_rng(9100 + 7 * H + W + N + int(s) + (0 if mode == "maps" else 50))
    zero = mask(case, mode)
    out = {}
    for m, (k, ch) in enumerate((("g_diff", 1), ("g_weight", 1), ("g_img_rec", 3))):
        if k not in zero:
            continue
        g = rng.standard_normal((N, ch, H, W))
        for n in range(N):
            g[n] *= 10.0 ** ((((3 * n + 2 * m) % 7) - 3) / 2)
        out[k] = np.ascontiguousarray(np.where(zero[k].reshape(N, 1, H, W), 0.0, g), np.float32)
    return out


def _grads(leaves_, names):
    return {k: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy()) for k, p in zip(names, leaves_)}


def maps_gradient(case, cot, dtype="f64", w_l1=W_L1, w_ssim=W_SSIM):
    """autograd through `assembly` on the shared leaves with the cotangents `cot` (a missing key is absent) -> dict g_rec, g_pd, g_cd"""
    dt = _dt(dtype)
    l = leaves(case)
    rec, pd, cd = (_T(l[k], dt).requires_grad_() for k in ("rec", "pd", "cd"))
    diff, weight = assembly(_T(l["tgt"], dt), rec, pd, cd, w_l1, w_ssim)
    outs = dict(g_diff=diff, g_weight=weight)
    sum((outs[k] * _T(cot[k], dt)).sum() for k in cot).backward()
    return _grads((rec, pd, cd), MAP_TENSORS)


@functools.lru_cache(maxsize=None)
def twin_maps(case, subset=MAP_COTS, dtype="f64"):
    """computed once per (case, subset, dtype) and shared: treat as read-only"""
    cot = cotangents(case, "maps")
    return maps_gradient(case, {k: cot[k] for k in subset}, dtype)


def chain_gradient(case, cot, dtype="f64", detached_mask=None):
    """autograd through oracle.torch_twin.photometric -> dict d_depth_t, d_depth_s, d_pose.  With `detached_mask` [N,1,H,W] the
    functional is the end-to-end scalar (diff mask weight).sum() / mask.sum() + 0.1 (1 - weight).mean() instead of the cotangents'."""
    dt = _dt(dtype)
    c = make_case(*case)
    d_t, d_s, pose = (_T(c[k], dt).requires_grad_() for k in ("depth_t", "depth_s", "pose"))
    r = tw.photometric(_T(c["tgt"], dt), _T(c["src"], dt), d_t, d_s, pose, _T(c["K"], dt))
    if detached_mask is not None:
        m = _T(detached_mask, dt)
        L = (r["diff"] * m * r["weight"]).sum() / m.sum() + 0.1 * (1 - r["weight"]).mean()
    else:
        outs = dict(g_diff=r["diff"], g_weight=r["weight"], g_img_rec=r["rec"])
        L = sum((outs[k] * _T(cot[k], dt)).sum() for k in cot)
    L.backward()
    return _grads((d_t, d_s, pose), CHAIN_TENSORS)


@functools.lru_cache(maxsize=None)
def twin_chain(case, subset=CHAIN_COTS, dtype="f64"):
    """computed once per (case, subset, dtype) and shared: treat as read-only"""
    cot = cotangents(case, "chain")
    return chain_gradient(case, {k: cot[k] for k in subset}, dtype)


def judge(got, ref, t32, tag, tensors, report=None, rel_l2_max=REL_L2_MAX):
    """warp_grad_inputs.judge for the tensors named in `tensors`; `rel_l2_max` None: no absolute cap (the chain)
    -> (failures, {tensor: (worst ratio to the float32 twin, largest relative L2)})"""
    fails, worst = [], {}
    for k in tensors:
        for n in range(ref[k].shape[0]):
            g, r = np.asarray(got[k][n], np.float64), ref[k][n]
            zero_bad = int(((r == 0) & (g != 0)).sum())
            (l2, mx), (l2_32, mx_32) = WG.errors(g, r), WG.errors(t32[k][n], r)
            ratio = max(l2 / l2_32 if l2_32 > 0 else (0.0 if l2 == 0 else float("inf")), mx / mx_32 if mx_32 > 0 else (0.0 if mx == 0 else float("inf")))
            if report:
                report(f"{tag}\t{k}[{n}]\trel_l2={l2:.3e}\tf32={l2_32:.3e}\tmax/rms={mx:.3e}\tf32={mx_32:.3e}\tratio={ratio:.3f}\tnonzero_at_exact_zero={zero_bad}")
            w = worst.get(k, (0.0, 0.0))
            worst[k] = (max(w[0], ratio), max(w[1], l2))
            if zero_bad:
                fails.append((tag, k, n, "exact zero", zero_bad, 0))
            if not l2 <= MARGIN * l2_32:
                fails.append((tag, k, n, "rel_l2 vs 4 x f32", l2, MARGIN * l2_32))
            if not mx <= MARGIN * mx_32:
                fails.append((tag, k, n, "max/rms vs 4 x f32", mx, MARGIN * mx_32))
            if rel_l2_max is not None and not l2 < rel_l2_max:
                fails.append((tag, k, n, "rel_l2 < 1e-4", l2, rel_l2_max))
    return fails, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel's formulas at numpy level (float64): the L1 part and the SSIM part of g_rec, the latter as a scatter over each window's
# nine reflected taps (the multiplicity m(q, p) arises by itself) or as the gather with m taken as 1
def _refl(i, n):
    i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return np.clip(i, 0, n - 1)


def l1_part(case, g_diff, w_l1=W_L1, only_at_one=False):
    l = leaves(case)
    d = l["rec"].astype(np.float64) - l["tgt"].astype(np.float64)
    sel = (np.abs(d) == 1) if only_at_one else (np.abs(d) <= 1)
    return np.where(sel, np.asarray(g_diff, np.float64) * (w_l1 / 3) * np.sign(d), 0.0)


def ssim_part(case, g_diff, w_ssim=W_SSIM, multiplicity=True):
    """sum_q m(q, p) g_diff[q] (w_ssim / 3) (-1/2) d s_q / d y_p  -> [N,3,H,W]"""
    H, W, N, _ = case
    l = leaves(case)
    x, y, g = l["tgt"].astype(np.float64), l["rec"].astype(np.float64), np.asarray(g_diff, np.float64)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    taps = [(_refl(vv + dv, H), _refl(uu + du, W), dv, du) for dv in (-1, 0, 1) for du in (-1, 0, 1)]
    xs, ys = np.stack([x[:, :, a, b] for a, b, _, _ in taps]), np.stack([y[:, :, a, b] for a, b, _, _ in taps])      # [9,N,3,H,W]
    mx, my = xs.mean(0), ys.mean(0)
    sx, sy, sxy = (xs * xs).mean(0) - mx * mx, (ys * ys).mean(0) - my * my, (xs * ys).mean(0) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + 1e-4, 2 * sxy + 9e-4, mx * mx + my * my + 1e-4, sx + sy + 9e-4
    s = A1 * A2 / (B1 * B2)
    v = (1 - s) / 2
    k = np.where((v >= 0) & (v <= 1), g * (w_ssim / 3) * -0.5, 0.0)
    out = np.zeros_like(y)
    nn, cc = np.meshgrid(np.arange(N), np.arange(3), indexing="ij")
    for i, (a, b, dv, du) in enumerate(taps):
        ds = ((2 * mx * A2 + 2 * (xs[i] - mx) * A1) / (B1 * B2) - s * (2 * my / B1 + 2 * (ys[i] - my) / B2)) / 9
        if multiplicity:
            np.add.at(out, (nn[:, :, None, None], cc[:, :, None, None], a[None, None], b[None, None]), k * ds)
        else:       # the gather with m = 1: window q = p - (dv, du) counts once if its UNREFLECTED tap q + (dv, du) is p
            ok = (vv + dv >= 0) & (vv + dv < H) & (uu + du >= 0) & (uu + du < W)
            np.add.at(out, (nn[:, :, None, None], cc[:, :, None, None], a[None, None], b[None, None]), np.where(ok, k * ds, 0.0))
    return out


def planted_faults(case):
    """-> {name: (faulty gradient dict, tensors the fault must be caught on)} from the float64 gradient of the maps with both cotangents"""
    H, W, N, _ = case
    ref, cot = twin_maps(case), cotangents(case, "maps")
    true = {k: ref[k].copy() for k in MAP_TENSORS}
    gd = cot["g_diff"]
    l1, ss = l1_part(case, gd), ssim_part(case, gd)
    out = {}
    f = dict(true); f["g_rec"] = true["g_rec"] - ss + ssim_part(case, gd, multiplicity=False)
    out["multiplicity_one"] = (f, ("g_rec",))
    f = dict(true); f["g_rec"] = l1 * (W_SSIM / W_L1) + (true["g_rec"] - l1) * (W_L1 / W_SSIM)
    out["weights_swapped"] = (f, ("g_rec",))
    f = dict(true); f["g_rec"] = true["g_rec"] * 3
    out["channel_mean_dropped"] = (f, ("g_rec",))
    f = dict(true); f["g_pd"] = -true["g_pd"]
    out["g_pd_sign"] = (f, ("g_pd",))
    f = dict(true); f["g_rec"] = true["g_rec"] - l1_part(case, gd, only_at_one=True)
    out["no_gradient_at_one"] = (f, ("g_rec",))
    first = {k: np.ascontiguousarray(np.repeat(v[:1], N, 0)) for k, v in cot.items()}
    out["item0_cotangents_for_all"] = (maps_gradient(case, first), MAP_TENSORS)
    return out
