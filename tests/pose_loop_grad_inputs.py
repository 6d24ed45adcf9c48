"""Inputs, the torch twin and the input search of the coupled pose loop's gradient tests (tests/test_pose_loop_grad_inputs_cpu.py,
tests/test_gpu_pose_loop_grad.py).  No GPU in here.

THE LOOP is train_mono.solve_pose_iteratively (train_mono.py:41-81) on disparity leaves: depth = 1 / (lo + (hi - lo) disp),
pose_0 = PoseNet(tgt | src ; src | tgt), then NUM_ITER - 1 rounds of  rec, valid = inverse_warp2(src, d_t, d_s, -pose, K);
pose += PoseNet(tgt * valid | rec).  Every iterate after the first depends on the disparities through the warp and the network's input.

TWIN (twin_loop): oracle.torch_twin.warp and posenet_grad_inputs.forward_pinned -- standins.PoseNetTwin layer by layer with the ReLU
decisions supplied -- in float64 (the reference) or float32 (the yardstick).  SCALAR: sum R * stacked_poses with R exact in fp32.

INPUT SEARCH.  The gradient of a bilinear sample is discontinuous at cell borders and the validity is a step, so the comparison
with float64 needs the float32 and the float64 loop to take the same bilinear cell and the same validity at every sample of every
warp, with headroom: every valid sample stays HEADROOM = tuning_chain_inputs.HEADROOM (8) x the float32 / float64 coordinate
difference off every cell border, and every projected position the same off the frame edges (conditions, conditions_hold).
CANDIDATES are seeds of inputs(); the search runs on the CPU (tests/test_pose_loop_grad_inputs_cpu.py asserts that the candidate in
use holds; a candidate near the threshold can change sides with the float32 twin's rounding on another host).
At 16 x 24 a warp has N x 384 x 2 coordinates, NUM_ITER - 1 = 2 warps; with a coordinate difference of ~5e-6 px the expected number
of samples inside the band is about 0.6 per candidate at N = 4: roughly half of the candidates hold.
RECORDED OUTCOME (HOLDING; the tests use the first candidate of a configuration):
  few  (B 1, S 2, N 4): candidates 0, 1, 5, 6, 7, 10, 11 of 12 hold.  Candidate 0: coordinate difference 4.9e-6 px, nearest boundary
                        1.04e-4 px = 21.1 x, validity keeps >= 88 % of a frame, no ReLU decision differs between the two loops
  many (B 2, S 2, N 8): candidate 0 of 12 holds (twice the samples: e^-1.2 per candidate).  Coordinate difference 5.7e-6 px, nearest
                        boundary 7.9e-5 px = 13.8 x, validity keeps >= 88 %
"""
import functools

import numpy as np
import torch

import posenet_grad_inputs as GI
import standins
import warp_grad_inputs as WG
from oracle import torch_twin as tw
from tuning_chain_inputs import HEADROOM

H, W = 16, 24
NUM_ITER = 3
DEPTH_RANGE = (0.1, 100.0)
CONFIGS = {"few": (1, 2), "many": (2, 2)}          # (B, S): N = 2 S B = 4 (the few-images regime) and 8 (the many-images regime)
CANDIDATES = list(range(12))
PARAM_SEED = 0
# the search's outcome: configuration -> the candidates that hold, in order; the tests use the first
HOLDING = {"few": (0, 1, 5, 6, 7, 10, 11), "many": (0,)}


def params():
    return standins.posenet_params(PARAM_SEED)


def _scales():
    return 1 / DEPTH_RANGE[1], 1 / DEPTH_RANGE[0]


@functools.lru_cache(maxsize=None)
def inputs(config, seed):
    """-> dict of float32 numpy arrays: tgt [B,3,H,W], srcs [S,B,3,H,W], disp_t [B,1,H,W], disp_s [S,B,1,H,W] (depths 1 .. 5), K [B,3,3],
    R [2SB, NUM_ITER, 6] (multiples of 1/8)"""
    B, S = CONFIGS[config]
    rng = np.random.default_rng(31000 + 100 * seed + 10 * B + S)
    yy, xx = np.mgrid[0:H, 0:W]

    def smooth(n, lo, hi, noise):
        ph = rng.uniform(0, 2 * np.pi, size=(n, 1, 1))
        fx, fy = rng.uniform(0.5, 2.0, size=(2, n, 1, 1))
        s = 0.5 + 0.5 * np.sin(ph + fx * xx / W * 5.0 + fy * yy / H * 5.0)
        s = s + noise * rng.uniform(-1, 1, size=(n, H, W))
        s = (s - s.min()) / (s.max() - s.min())
        return lo + (hi - lo) * s

    img = smooth((1 + S) * B * 3, 0.1, 0.9, 0.15).reshape(1 + S, B, 3, H, W)
    lo, hi = _scales()
    depth = smooth((1 + S) * B, 1.0, 5.0, 0.05).reshape(1 + S, B, 1, H, W)
    disp = (1 / depth - lo) / (hi - lo)
    K = np.repeat(np.array([[0.58 * W, 0, (W - 1) / 2], [0, 0.58 * W, (H - 1) / 2], [0, 0, 1]])[None], B, 0)
    R = rng.integers(-8, 9, size=(2 * S * B, NUM_ITER, 6)) / 8.0
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(tgt=f(img[0]), srcs=f(img[1:]), disp_t=f(disp[0]), disp_s=f(disp[1:]), K=f(K), R=f(R))


def twin_loop(inp, dtype, masks=None, grad=False, record=None):
    """the loop in `dtype` -> dict: stacked [N, NUM_ITER, 6], masks (per PoseNet call, the decisions used), and with grad the gradients
    d_disp_t, d_disp_s of sum R * stacked (float64 numpy).  masks: per call 0 .. NUM_ITER - 1 the seven ReLU masks, or None (own).
    record: a list that receives, per warp, warp_grad_inputs.geometry of its samples, evaluated in `dtype` at this loop's poses and depths"""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    sd = params()
    S, B = inp["srcs"].shape[:2]
    split = S * B
    lo, hi = _scales()
    disp_t, disp_s = T(inp["disp_t"]).requires_grad_(grad), T(inp["disp_s"]).requires_grad_(grad)
    depth_t, depth_s = 1 / (lo + (hi - lo) * disp_t), 1 / (lo + (hi - lo) * disp_s)
    td, sdp = depth_t.repeat(S, 1, 1, 1), depth_s.reshape(split, 1, H, W)
    ti, si = T(inp["tgt"]).repeat(S, 1, 1, 1), T(inp["srcs"]).reshape(split, 3, H, W)
    tgt, src = torch.cat([ti, si], 0), torch.cat([si, ti], 0)
    d_t, d_s = torch.cat([td, sdp], 0), torch.cat([sdp, td], 0)
    K = T(inp["K"]).repeat(2 * S, 1, 1)
    used = []
    with torch.no_grad():
        p, m = GI.forward_pinned(sd, torch.cat([tgt, src], 1), None if masks is None else masks[0], dtype)
    used.append(m)
    stacked = [p]
    for it in range(1, NUM_ITER):
        if record is not None:
            record.append(WG.geometry(dict(src=src.detach().numpy(), K=K.numpy(), pose=p.detach().numpy(), depth_t=d_t.detach().numpy()), dtype))
        rec, valid, _, _ = tw.warp(src, d_t, d_s, -p, K)
        c, m = GI.forward_pinned(sd, torch.cat([tgt * valid, rec], 1), None if masks is None else masks[it], dtype)
        used.append(m)
        p = p + c
        stacked.append(p)
    st = torch.stack(stacked, 1)
    out = dict(stacked=st.detach().double().numpy(), masks=used)
    if grad:
        (st * T(inp["R"])).sum().backward()
        out["d_disp_t"], out["d_disp_s"] = disp_t.grad.double().numpy(), disp_s.grad.double().numpy()
    return out


def geometry_margins(g, g32):
    """two recordings of one warp (float64 | float32 or the library's) -> (flips, coordinate difference, distance of the float64
    samples to the nearest cell border / frame edge), as tuning_chain_inputs.conditions"""
    frac = lambda a: np.minimum(a - np.floor(a), np.ceil(a) - a)
    v = g["valid"]
    cell = (np.floor(g32["ix"]) != np.floor(g["ix"])) | (np.floor(g32["iy"]) != np.floor(g["iy"]))
    flips = int((cell & v).sum() + (g32["valid"] != v).sum())
    diff = max(float(np.abs(g32[k] - g[k]).max()) for k in ("ix", "iy", "xp", "yp"))
    near = (np.abs(g["xp"]) < 1) | (np.abs(g["xp"] - (W - 1)) < 1) | (np.abs(g["yp"]) < 1) | (np.abs(g["yp"] - (H - 1)) < 1) | v
    edge = np.minimum.reduce([np.abs(g["xp"]), np.abs(g["xp"] - (W - 1)), np.abs(g["yp"]), np.abs(g["yp"] - (H - 1))])
    boundary = min(float(np.minimum(frac(g["ix"]), frac(g["iy"]))[v].min()) if v.any() else np.inf, float(edge[near].min()) if near.any() else np.inf)
    return flips, diff, boundary


@functools.lru_cache(maxsize=None)
def conditions(config, seed):
    """the float64 and the float32 twin loop (own ReLU decisions) on inputs(config, seed) -> dict: flips, coord_diff, boundary,
    margin_ratio, valid_share (smallest share of a frame a warp's validity keeps), z_min, mask_flips (ReLU decisions on which the two
    loops differ: reported, the GPU test pins them)"""
    inp = inputs(config, seed)
    r64, r32 = [], []
    with torch.no_grad():
        a, b = twin_loop(inp, torch.float64, record=r64), twin_loop(inp, torch.float32, record=r32)
    out = dict(flips=0, coord_diff=0.0, boundary=np.inf, valid_share=1.0, z_min=np.inf)
    for g, g32 in zip(r64, r32):
        f, d, bd = geometry_margins(g, g32)
        out["flips"] += f
        out["coord_diff"], out["boundary"] = max(out["coord_diff"], d), min(out["boundary"], bd)
        out["valid_share"] = min(out["valid_share"], float(g["valid"].mean(1).min()))
        out["z_min"] = min(out["z_min"], float(g["p2"].min()))
    out["margin_ratio"] = out["boundary"] / out["coord_diff"]
    out["mask_flips"] = int(sum(int((x != y).sum()) for ma, mb in zip(a["masks"], b["masks"]) for x, y in zip(ma, mb)))
    return out


def conditions_hold(c):
    """-> list of the conditions that do NOT hold (empty: the inputs are fit)"""
    bad = []
    if c["flips"]:
        bad.append("float32 and float64 loop choose another bilinear cell or validity")
    if not c["boundary"] >= HEADROOM * c["coord_diff"]:
        bad.append("a sample is closer to a cell or frame boundary than 8 x the float32 / float64 coordinate difference")
    if not c["valid_share"] >= 0.5:
        bad.append("a warp's validity keeps less than half of a frame")
    if not c["z_min"] > 2e-3:
        bad.append("a point comes near the depth clamp")
    return bad


def search(config):
    """-> the candidates that hold, in order"""
    return tuple(s for s in CANDIDATES if not conditions_hold(conditions(config, s)))


def chosen(config):
    """the committed candidate of a configuration, or None when none holds (the GPU test then falls back to the unpinned bar)"""
    return HOLDING[config][0] if HOLDING[config] else None


def judge(got, ref, t32):
    """dicts with d_disp_t, d_disp_s -> (failures, {tensor: figures}): posenet_grad_inputs.judge per tensor"""
    fails, figs = [], {}
    for k in ("d_disp_t", "d_disp_s"):
        ok, f = GI.judge(torch.as_tensor(np.asarray(got[k], np.float64)), torch.as_tensor(ref[k]), torch.as_tensor(t32[k]))
        figs[k] = f
        if not ok:
            fails.append((k, f))
    return fails, figs
