"""Inputs, float64 reference and judging rules of the composed weight-tuning chain -- DepthNetModule -> slices ->
learning_helpers.disp_to_depth -> helpers.compute_photometric_error (forward and inverse pairs) -> losses.compute_optimization_loss ->
backward() --, shared by tests/test_tuning_chain_inputs_cpu.py and tests/test_gpu_tuning_chain.py.  No GPU here.

THE CHAIN is the reference's epoch body (optimization_experiments/optimizer.py:217-268) with B = 1, S = 2: the three images go through
the network as one batch, the disparity is sliced into the target and the two sources (optimizer.py:232-234), each slice becomes a
depth, the target's depth is repeated once per pair, and the loss is the reference's.  Poses and intrinsics are constants: the library
has no PoseNet backward, so the dependence of solve_pose_iteratively's poses on the depths is not imitated.

INPUTS.  Weights depthnet_twin.depthnet_params(SEED[shape]), images depthnet_twin.sample_images, a pinhole K (focal length 0.58 W,
principal point at the frame's centre), the depth range of loss_grad_inputs (0.1 .. 100), and two poses whose translation is scaled
so that the flow at the depth 1 / (a + b / 2) is FLOW_PX[shape] pixels.  The seed and the flow were searched over SEARCH (CPU, the
float32 twin network's disparities) for conditions() -- see there -- to hold.  MEASURED for the committed constants:
  32 x 64   seed 0, flow 1.5 px: validity keeps >= 90.8 % of a frame, float32 / float64 coordinate difference 1.3e-5 px, nearest
            cell or frame boundary 2.6e-4 px = 19.6 x that difference (the only one of the 40 candidates above 8 x)
  96 x 160  seed 9, flow 3.0 px: validity keeps >= 95.2 %, no cell or validity flip, coordinate difference 3.9e-5 px, nearest boundary
            8.9e-6 px = 0.23 x (the best of the 21 candidates without a flip)
THE HEADROOM of 8 x cannot be had at 96 x 160: the four pairs have 4 x 15 360 x 2 sample coordinates whose fractional parts are
spread evenly, so about 123 000 x 2 x 8 x 4e-5 = 80 of them lie inside the band whatever the seed, and the chance of none is e^-80
(at 32 x 64: 16 384 x 2 x 8 x 1.3e-5 = 3.4, one candidate in 30).  So the comparison of the loss side with float64 (which needs the
library, the float32 twin and float64 to take the same bilinear cell at every pixel) runs at 32 x 64, ACCURACY_SHAPE, alone;
96 x 160 serves the bitwise comparisons and the network's backward under the chain's cotangent, which do not depend on the cells,
and the CPU test reports its margin without asserting it.

REFERENCE of the loss side: loss_grad_inputs.e2e_twin (float64; the yardstick is the same code in float32) at disparity leaves.
JUDGES.  loss_judge: loss_grad_inputs.judge without the absolute relative-L2 cap (as the chain tests use it) on the disparity
gradient, split into d_disp_t [1,1,H,W] and d_disp_s [2,1,H,W].  param_judge: every parameter gradient against float64 by
test_gpu_depthnet_grad_exact._errs, held to that module's ENC_* (encoder) and DEC_* (decoder) bounds.
planted_faults: six faults of the composition, made at torch level from the float64 twin chain.
"""
import functools

import numpy as np
import torch

import depthnet_twin as dt
import loss_grad_inputs as LG

WG = LG.WG
SHAPES = [(32, 64), (96, 160)]            # layer 4 is 1 x 2 (the smallest frame with W != H) | odd deep maps, 3 x 5
IDS = [f"{H}x{W}" for H, W in SHAPES]
N_IMAGES = 3                              # B = 1 target and S = 2 sources
DEPTH_RANGE = LG.E2E_DEPTH_RANGE
ACCURACY_SHAPE = SHAPES[0]                # the one shape at which the cell headroom can hold (docstring)
SEED = {(32, 64): 0, (96, 160): 9}        # depthnet_params seed (docstring: how they were chosen)
FLOW_PX = {(32, 64): 1.5, (96, 160): 3.0}
SEARCH = [(seed, flow) for seed in range(10) for flow in (1.0, 1.5, 2.0, 3.0)]
HEADROOM = 8.0                            # a valid sample stays HEADROOM x the float32 / float64 coordinate difference off every boundary
POSE_DIRS = np.array([[1.0, 0.12, 0.35, 0.004, -0.010, 0.003], [-0.8, -0.15, -0.45, -0.003, 0.008, -0.004]])
OPTIONS = LG.E2E_OPTIONS
OPTIONS_DEFAULT = dict(LG.E2E_OPTIONS, diff_img_argmin=True, automasking=True)      # the reference's defaults for this loop
TENSORS = LG.E2E_TENSORS


def _T(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _scales():
    lo, hi = 1 / DEPTH_RANGE[1], 1 / DEPTH_RANGE[0]
    return lo, hi


def images(shape):
    H, W = shape
    return dt.sample_images(300 + H + W, N_IMAGES, H, W)


def intrinsics(shape):
    H, W = shape
    K = np.array([[0.58 * W, 0, (W - 1) / 2], [0, 0.58 * W, (H - 1) / 2], [0, 0, 1]])
    return np.ascontiguousarray(np.repeat(K[None], 2, 0), np.float32)


def poses(shape, flow_px=None):
    """[2,6] float32: POSE_DIRS with the translation scaled to a flow of `flow_px` at the depth 1 / (a + b / 2)"""
    lo, hi = _scales()
    z0 = 1 / (lo + (hi - lo) / 2)
    p = POSE_DIRS.copy()
    p[:, :3] *= (FLOW_PX[shape] if flow_px is None else flow_px) * z0 / (0.58 * shape[1])
    return np.ascontiguousarray(p, np.float32)


@functools.lru_cache(maxsize=None)
def _params(seed):
    return dt.depthnet_params(seed)


@functools.lru_cache(maxsize=None)
def twin_disparity(shape, seed=None):
    """the float32 CPU twin network's disparity of images(shape) -> [3,1,H,W] float32 (shared: read-only)"""
    sd = dict(_params(SEED[shape] if seed is None else seed))
    with torch.no_grad():
        return dt.forward(sd, torch.from_numpy(images(shape))).numpy()


def perturbed(disp_t):
    """the initial disparity of the accuracy case: the target disparity times 1 +- 5..15 % per pixel (as loss_grad_inputs.e2e_inputs),
    so that the depth-init term has a gradient"""
    rng = np.random.default_rng(4500)
    d = np.asarray(disp_t, np.float64)
    return np.ascontiguousarray(d * (1 + rng.choice([-1.0, 1.0], d.shape) * rng.uniform(0.05, 0.15, d.shape)), np.float32)


def chain_inputs(shape, disp, disp_init=None, flow_px=None):
    """the dict loss_grad_inputs.e2e_twin takes, at the disparity `disp` [3,1,H,W] (kept in its dtype)"""
    im = images(shape)
    disp = np.asarray(disp)
    return dict(tgt=im[:1], src=im[1:], disp_t=disp[:1], disp_s=disp[1:], pose=poses(shape, flow_px), K=intrinsics(shape),
                disp_init=perturbed(disp[:1]) if disp_init is None else np.asarray(disp_init))


def directed_pairs(inp, dtype=torch.float64):
    """the four directed pairs as warp_grad_inputs.geometry takes them (target -> source 1, 2; source 1, 2 -> target), the depths
    evaluated in `dtype` from the disparities"""
    lo, hi = _scales()
    depth = lambda d: (1 / (lo + (hi - lo) * _T(d, dtype))).numpy()
    zt, zs = depth(inp["disp_t"]), depth(inp["disp_s"])
    tgt2 = np.repeat(inp["tgt"], 2, 0)
    return [dict(src=inp["src"], K=inp["K"], pose=inp["pose"], depth_t=np.repeat(zt, 2, 0)),
            dict(src=tgt2, K=inp["K"], pose=-inp["pose"], depth_t=zs)]


def conditions(shape, disp, flow_px=None):
    """what the GPU tests rely on, at the disparity `disp` [3,1,H,W] float32 -> dict: disp_min, disp_max; valid_share (the smallest
    share of a frame that one of the four directed pairs' validity keeps); flips (pixels at which the float32 geometry takes another
    bilinear cell -- valid pixels -- or another validity than float64); coord_diff (largest |float32 - float64| of ix, iy, xp, yp);
    boundary (smallest distance of a valid sample to a cell border, and of any projected position to the frame edges 0, W - 1,
    H - 1, the pixels off the frame by more than a pixel aside); margin_ratio = boundary / coord_diff; z_min (smallest depth before
    the clamp at 1e-3); smooth_sign (edges of the target on which the float32 and the float64 smooth loss disagree in sign)"""
    H, W = shape
    inp = chain_inputs(shape, disp, flow_px=flow_px)
    out = dict(disp_min=float(np.min(disp)), disp_max=float(np.max(disp)), valid_share=1.0, flips=0, coord_diff=0.0, boundary=np.inf, z_min=np.inf)
    frac = lambda a: np.minimum(a - np.floor(a), np.ceil(a) - a)
    for c64, c32 in zip(directed_pairs(inp), directed_pairs(inp, torch.float32)):
        g, g32 = WG.geometry(c64), WG.geometry(c32, torch.float32)
        v = g["valid"]
        out["valid_share"] = min(out["valid_share"], float(v.mean(1).min()))
        cell = (np.floor(g32["ix"]) != np.floor(g["ix"])) | (np.floor(g32["iy"]) != np.floor(g["iy"]))
        out["flips"] += int((cell & v).sum() + (g32["valid"] != v).sum())
        out["coord_diff"] = max([out["coord_diff"]] + [float(np.abs(g32[k] - g[k]).max()) for k in ("ix", "iy", "xp", "yp")])
        near = (np.abs(g["xp"]) < 1) | (np.abs(g["xp"] - (W - 1)) < 1) | (np.abs(g["yp"]) < 1) | (np.abs(g["yp"] - (H - 1)) < 1) | v
        edge = np.minimum.reduce([np.abs(g["xp"]), np.abs(g["xp"] - (W - 1)), np.abs(g["yp"]), np.abs(g["yp"] - (H - 1))])
        out["boundary"] = min(out["boundary"], float(np.minimum(frac(g["ix"]), frac(g["iy"]))[v].min()), float(edge[near].min()))
        out["z_min"] = min(out["z_min"], float(g["p2"].min()))
    out["margin_ratio"] = out["boundary"] / out["coord_diff"]
    out["smooth_sign"] = LG.smooth_input_report(np.asarray(disp)[:1])[0]
    return out


def conditions_hold(c, headroom=True):
    """-> list of the conditions that do NOT hold (empty: the inputs are fit); `headroom` False: without the boundary headroom"""
    bad = []
    if not (0 < c["disp_min"] and c["disp_max"] < 1):
        bad.append("a disparity is not strictly inside (0, 1)")
    if not c["valid_share"] >= 0.5:
        bad.append("a directed pair's validity mask keeps less than half of the frame")
    if c["flips"]:
        bad.append("float32 and float64 geometry choose another bilinear cell or validity")
    if headroom and not c["boundary"] >= HEADROOM * c["coord_diff"]:
        bad.append("a valid sample is closer to a cell or frame boundary than 8 x the float32 / float64 coordinate difference")
    if not c["z_min"] > 2e-3:
        bad.append("a point comes near the depth clamp")
    if c["smooth_sign"]:
        bad.append("the float32 smooth loss takes another sign than float64 on an edge of the target disparity")
    return bad


def split(g_disp):
    """the network's disparity cotangent [3,1,H,W] as the twin's tensors"""
    g = np.asarray(g_disp, np.float64)
    return dict(d_disp_t=g[:1], d_disp_s=g[1:])


def join(g):
    return np.concatenate([g["d_disp_t"], g["d_disp_s"]], 0)


def loss_judge(got, ref, t32, tag, report=None):
    """loss_grad_inputs.judge on the split disparity cotangent, no absolute relative-L2 cap -> (failures, worst figures)"""
    return LG.judge(got, ref, t32, tag, TENSORS, report, None)


def param_judge(got, ref, report=None, tag=""):
    """got, ref: {parameter name: gradient tensor}, ref in float64 (None or all zero: `got` must be exactly zero) -> ({name: (relative
    L2, max error / RMS)} of the tensors over their bound, the worst (relative L2, max / RMS) per class "encoder" / "decoder")"""
    import test_gpu_depthnet_grad_exact as X
    bad, worst = {}, {}
    for k, g in got.items():
        e = X._errs(g, ref[k])
        enc = k.startswith(dt.ENC)
        if report:
            report(f"{tag}\t{k}\trel_l2={e[0]:.3e}\tmax/rms={e[1]:.3e}")
        w = worst.get("encoder" if enc else "decoder", (0.0, 0.0))
        worst["encoder" if enc else "decoder"] = (max(w[0], e[0]), max(w[1], e[1]))
        rel, elem = (X.ENC_REL, X.ENC_ELEM) if enc else (X.DEC_REL, X.DEC_ELEM)
        if not (e[0] <= rel and e[1] <= elem):
            bad[k] = e
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 twin chain from the weights, and the planted faults of the composition
@functools.lru_cache(maxsize=None)
def _twin_network(shape):
    """the float64 twin network's forward on images(shape), graph kept -> (parameters that take a gradient, disparity)"""
    sd = {k: v.double() for k, v in _params(SEED[shape]).items()}
    params = {k: v.requires_grad_() for k, v in sd.items() if not k.endswith(("running_mean", "running_var"))}
    return params, dt.forward(sd, torch.from_numpy(images(shape)).double())


def twin_param_gradients(shape, g_disp):
    """the float64 twin network's (unpinned) parameter gradients under the disparity cotangent g_disp [3,1,H,W] -> {name: tensor}"""
    params, disp = _twin_network(shape)
    return dict(zip(params, torch.autograd.grad(disp, list(params.values()), _T(g_disp, torch.float64), retain_graph=True)))


@functools.lru_cache(maxsize=None)
def twin_chain(shape):
    """the twin's loss side at the float32 twin network's disparities, with the float64 twin's own masks -> (inputs, masks, float64
    gradient dict, float32 gradient dict); shared: read-only"""
    inp = chain_inputs(shape, twin_disparity(shape))
    masks = LG.e2e_twin_masks("f64", inp, DEPTH_RANGE)
    return inp, masks, LG.e2e_twin(masks, "f64", inp, OPTIONS, DEPTH_RANGE)[0], LG.e2e_twin(masks, "f32", inp, OPTIONS, DEPTH_RANGE)[0]


def planted_faults(shape):
    """-> {name: faulty disparity cotangent as split() gives it}: what a wrong composition of correct stages would hand the network"""
    inp, masks, true, _ = twin_chain(shape)
    run = lambda options=OPTIONS, hooks=None: LG.e2e_twin(masks, "f64", inp, options, DEPTH_RANGE, hooks)[0]
    out = {}
    out["sources_detached"] = dict(true, d_disp_s=np.zeros_like(true["d_disp_s"]))
    out["repeat_counted_once"] = run(hooks=dict(repeat=lambda z: torch.cat([z[:1], z[1:].detach()], 0)))
    out["depth_init_dropped"] = dict(true, d_disp_t=run(dict(OPTIONS, l_depth_init=False))["d_disp_t"])
    out["smoothness_dropped"] = dict(true, d_disp_t=run(dict(OPTIONS, l_smooth=False))["d_disp_t"])
    out["inverse_ref_depth_dropped"] = run(hooks=dict(inv_ref_depth=lambda z: z.detach()))
    out["image1_cotangent_to_image2"] = dict(true, d_disp_s=np.repeat(true["d_disp_s"][:1], 2, 0))
    return out
