#!/usr/bin/env python3
"""Generate the FOUR-source window fixture by running the reference itself (build container only; see make_golden.py).

    python tests/golden/make_golden_four_sources.py        # writes tests/golden/golden_winloss4src24x40.npz

The G13 fixture of make_golden.py at S = 4 -- the five-frame window t-2 .. t+2 of an SfMLearner-style snippet: the reference's
compute_optimization_loss (optimizer.py:29-134) on the outputs of solve_pose_iteratively (train_mono.py:41-120) with a stand-in PoseNet
whose output is a leaf, and the autograd gradients w.r.t. all 2 S B = 16 directed poses, the shared target depth and the source depths
(`full`), the complete default loss with the l_depth_init prior (`fullinit`, its sigmoid disparity as the leaf), + l_smooth
(`fullinit_smooth`), + l_pose_consist (`full_pc`), without the min over the sources (`noargmin_full`), and the reference's
quarter-resolution parametrisation (`qinit`, the quarter-resolution maps of target and sources as the leaf).  Keys as in G13.
The four sources have distinct poses (t-1, t+1, t-2, t+2) and depth maps made mildly inconsistent with the geometry, each in its own
way, so that the depth-consistency weights differ between all four and w_dc couples them.  Data only: nothing from the reference's
source text is copied.
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, import_reference  # noqa: E402  (the reference with its absent dependencies stubbed)

sys.path.insert(0, REPO)


class LeafPose(nn.Module):
    def __init__(self, first):
        super().__init__(); self.first = first

    def forward(self, x):
        return self.first


def main():
    from tightly_coupled_sfm_amd import synth
    ref = import_reference()
    losses = ref["losses"]
    DO = ref["optimizer"].DepthOptimizer
    T = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt)
    N = lambda t: t.detach().cpu().numpy()
    B, S, H, W = 2, 4, 24, 40
    ref["stn"].pixel_coords = None
    factors = (1.0, -1.0, 2.0, -2.0)               # sources t-1, t+1, t-2, t+2 of the five-frame window (distinct poses)
    tg, srcs, dts, dss, Ks, pgt = [], [[] for _ in range(S)], [], [[] for _ in range(S)], [], [[] for _ in range(S)]
    for b in range(B):
        for si in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * factors[si]
            p = synth.make_pair(H, W, seed=140 + b, pose_gt=base, dtype=np.float64)
            if si == 0:
                tg.append(p["tgt"]); dts.append(p["depth_t"]); Ks.append(p["K"])
            srcs[si].append(p["src"]); pgt[si].append(p["pose_gt"])
            dss[si].append(p["depth_s"] * (1.0 + 0.05 * (si + 1) * np.sin(np.arange(W) / (5.0 + 2 * si) + 0.4 * si)[None, :]))
    rng = np.random.default_rng(14)
    gt_f = np.concatenate([np.stack(x) for x in pgt])
    first = np.concatenate([gt_f, -gt_f]) + rng.normal(scale=1.5e-3, size=(2 * S * B, 6))
    g = dict(target=np.stack(tg), sources=np.stack([np.stack(x) for x in srcs]), depth_t=np.stack(dts)[:, None],
             depth_s=np.stack([np.stack(x) for x in dss])[:, :, None], K=np.stack(Ks), first=first)
    dt = torch.float64
    base_opts = {'epochs': 20, 'diff_img_argmin': True, 'automasking': True, 'l_depth_consist': False,
                 'l_depth_consist_weight': 0.15, 'l_depth_init': False, 'l_depth_init_weight': 0.1,
                 'l_inverse_reconstruction': False, 'l_smooth': False, 'l_smooth_weight': 2,
                 'l_pose_consist': False, 'num_source_imgs': S, 'plotting': False}
    srcs_t = lambda: [T(g["sources"][i], dt) for i in range(S)]

    def loss_of(upd, fp, depths, disp=None, disp0=None):
        _, _, outputs = ref["train_mono"].solve_pose_iteratively(1, depths, LeafPose(fp), T(g["target"], dt), srcs_t(), T(g["K"], dt),
                                                                 return_errors=True)
        o = object.__new__(DO)
        o.options = dict(base_opts, **upd); o.ssim_loss = losses.SSIM_Loss()
        if disp0 is not None:
            o.target_disparity = disp0
        return DO.compute_optimization_loss(o, 0, 0, T(g["target"], dt), disp, outputs['fwd'], outputs['inv']).reshape(-1)[0]

    full = {'l_inverse_reconstruction': True, 'l_depth_consist': True}
    for tag, upd in (("full", full), ("noargmin_full", dict(full, diff_img_argmin=False)), ("full_pc", dict(full, l_pose_consist=True))):
        fp = T(first, dt).clone().requires_grad_()
        d_t = T(g["depth_t"], dt).clone().requires_grad_()
        d_s = [T(g["depth_s"][i], dt).clone().requires_grad_() for i in range(S)]
        loss = loss_of(upd, fp, [d_t] + d_s)
        loss.backward()
        g[f"{tag}_loss"] = np.array(loss.item()); g[f"{tag}_grad_pose"] = N(fp.grad)
        if tag == "full":
            g["full_grad_depth_t"] = N(d_t.grad[:, 0]); g["full_grad_depth_s"] = np.stack([N(x.grad[:, 0]) for x in d_s])
    MIN_D, MAX_D = 0.06, 2.67
    r_d = 1.0 / MIN_D - 1.0 / MAX_D
    sig_np = (1.0 / g["depth_t"] - 1.0 / MAX_D) / r_d
    assert sig_np.min() > 0.0 and sig_np.max() < 1.0
    yy, xx = np.mgrid[0:H, 0:W]
    sig0_np = sig_np * (1.0 + 0.04 * np.cos(xx / 3.0 + 0.7 * yy)[None, None] + 0.02 * np.sin(yy / 2.0)[None, None])
    g["sig_t"] = sig_np[:, 0]; g["sig_t0"] = sig0_np[:, 0]; g["min_max_depth"] = np.array([MIN_D, MAX_D])
    init = dict(full, l_depth_init=True)
    for tag, upd in (("fullinit", init), ("fullinit_smooth", dict(init, l_smooth=True))):
        fp = T(first, dt).clone().requires_grad_()
        sig = T(sig_np, dt).clone().requires_grad_()
        d_t = ref["learning_helpers"].disp_to_depth(sig, MIN_D, MAX_D)[1]
        loss = loss_of(upd, fp, [d_t] + [T(g["depth_s"][i], dt) for i in range(S)], disp=sig, disp0=T(sig0_np, dt))
        loss.backward()
        g[f"{tag}_loss"] = np.array(loss.item()); g[f"{tag}_grad_pose"] = N(fp.grad); g[f"{tag}_grad_sig_t"] = N(sig.grad[:, 0])
    # the reference's parametrisation (optimizer.py:194-198, 235-239): quarter-resolution sigmoid disparities of the target and every source
    F = torch.nn.functional
    sig_s_np = (1.0 / g["depth_s"] - 1.0 / MAX_D) / r_d
    assert sig_s_np.min() > 0.0 and sig_s_np.max() < 1.0
    fullmaps = torch.cat([T(sig_np, dt)] + [T(sig_s_np[i], dt) for i in range(S)], 1)
    quarter = F.interpolate(fullmaps, (H // 4, W // 4), mode='bilinear').clone().detach().requires_grad_()
    up = F.interpolate(quarter, (H, W), mode='bilinear')
    dl = [up[:, i:i + 1] for i in range(S + 1)]
    fp = T(first, dt).clone().requires_grad_()
    loss = loss_of(init, fp, [ref["learning_helpers"].disp_to_depth(d, MIN_D, MAX_D)[1] for d in dl], disp=dl[0], disp0=T(sig0_np, dt))
    loss.backward()
    g["q_sig"] = N(quarter.detach()); g["q_up"] = N(up.detach())
    g["qinit_loss"] = np.array(loss.item()); g["qinit_grad_pose"] = N(fp.grad); g["qinit_grad_q"] = N(quarter.grad)
    path = os.path.join(HERE, "golden_winloss4src24x40.npz")
    np.savez_compressed(path, **g)
    print(f"winloss4src24x40 {os.path.getsize(path) / 1024:8.1f} KiB  keys={len(g)}")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main()
