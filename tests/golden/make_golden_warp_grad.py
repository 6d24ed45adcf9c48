#!/usr/bin/env python3
"""Generate the warp-gradient fixture by running the reference's own inverse_warp2 under autograd (build container only).

    python tests/golden/make_golden_warp_grad.py   # writes tests/golden/golden_warp_grad.npz

models.stn.inverse_warp2 in float64 at 24 x 40, N = 3 (synth.make_batch, seeded): item 0 at its ground-truth pose, item 1 at a
perturbed one, item 2 at a strong yaw plus a backwards translation, which gives out-of-frame and Z-clamped pixels.  The gradients
of sum(rec * g_rec) + sum(proj_depth * g_pd) + sum(comp_depth * g_cd) with seeded normal cotangents, with respect to depth,
ref_depth and the pose 6-vector the call sites hold (the warp is called with -pose).  Data only: nothing from the reference's
source text is copied.
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, import_reference  # noqa: E402

N, H, W = 3, 24, 40
SEED, G_SEED = 31, 17


def main():
    from tightly_coupled_sfm_amd import synth
    stn = import_reference()["stn"]
    b = synth.make_batch(N, H, W, seed0=SEED)
    pose = b["pose_gt"].astype(np.float64).copy()
    pose[1] = synth.perturb_pose(pose[1], SEED + 1)
    pose[2] = np.array([0.05, -0.02, 1.2, 0.02, 0.3, -0.04])
    rng = np.random.RandomState(G_SEED)
    cot = dict(g_rec=rng.standard_normal((N, 3, H, W)), g_pd=0.5 * rng.standard_normal((N, 1, H, W)), g_cd=2.0 * rng.standard_normal((N, 1, H, W)))
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    src, K = T(b["src"]), T(b["K"])
    dt, ds, po = (T(a).clone().requires_grad_() for a in (b["depth_t"], b["depth_s"], pose))
    stn.pixel_coords = None       # the reference caches its pixel grid in a module global keyed only on height
    rec, valid, pd, cd = stn.inverse_warp2(src, dt, ds, -po, K, "zeros")
    ((rec * T(cot["g_rec"])).sum() + (pd * T(cot["g_pd"])).sum() + (cd * T(cot["g_cd"])).sum()).backward()
    n_oob, n_clamp = int((valid == 0).sum()), int((cd.detach() == 1e-3).sum())
    assert n_oob > 0 and n_clamp > 0, (n_oob, n_clamp)
    out = dict(src=b["src"].astype(np.float64), depth_t=b["depth_t"].astype(np.float64), depth_s=b["depth_s"].astype(np.float64),
               K=b["K"].astype(np.float64), pose=pose, **cot,
               rec=rec.detach().numpy(), valid=valid.detach().numpy(), proj_depth=pd.detach().numpy(), comp_depth=cd.detach().numpy(),
               d_depth_t=dt.grad.numpy(), d_depth_s=ds.grad.numpy(), d_pose=po.grad.numpy())
    path = os.path.join(HERE, "golden_warp_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; out-of-frame pixels", n_oob, "clamped", n_clamp)


if __name__ == "__main__":
    main()
