#!/usr/bin/env python3
"""Generate the depth-network gradient fixture by running the reference's own module under autograd (build container only).

    python tests/golden/make_golden_depthnet_grad.py   # writes tests/golden/golden_depthnet_grad.npz

models.depth_w_access.depth_model (num_scales = 1, evaluation mode) in float64 with the seeded parameters of
tests/depthnet_twin.depthnet_params, on seeded images of depthnet_twin.sample_images (N = 2, 64 x 192); the gradients of
(disp * R).sum() with respect to every parameter, R standard normal from numpy RandomState(R_SEED).  Stored per tensor: the L2 norm
and a fixed strided sample of at most SAMPLES elements (flat index i * stride).  The torchvision stand-in of make_golden_depthnet.py
provides ResNet18.  Data only: nothing from the reference's source text is copied.
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, REF  # noqa: E402
from make_golden_depthnet import install_torchvision_standin  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
from depthnet_twin import depthnet_params, sample_images  # noqa: E402

SEED, IMG_SEED, R_SEED = 0, 21, 5
N, H, W = 2, 64, 192
SAMPLES = 64


def main():
    install_torchvision_standin()
    sys.path.insert(0, REF)
    from models.depth_w_access import depth_model
    net = depth_model({"num_scales": 1}).double().eval()
    params = depthnet_params(SEED)
    net.load_state_dict({k: v.double() for k, v in params.items()}, strict=False)
    x = torch.from_numpy(sample_images(IMG_SEED, N, H, W)).double()
    R = torch.from_numpy(np.random.RandomState(R_SEED).standard_normal((N, 1, H, W)))
    disps, _ = net(x=x)
    (disps[0] * R).sum().backward()
    named = dict(net.named_parameters())
    names = [k for k in params if not k.endswith(("running_mean", "running_var"))]
    out = {"seed": np.int64(SEED), "img_seed": np.int64(IMG_SEED), "r_seed": np.int64(R_SEED), "size": np.array([N, H, W]),
           "names": np.array(names)}
    for i, k in enumerate(names):
        g = named[k].grad.detach().numpy().reshape(-1)
        stride = max(1, g.size // SAMPLES)
        out[f"g{i}_norm"] = np.float64(np.linalg.norm(g))
        out[f"g{i}_stride"] = np.int64(stride)
        out[f"g{i}_val"] = g[::stride][:SAMPLES].astype(np.float64)
    path = os.path.join(HERE, "golden_depthnet_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "tensors")


if __name__ == "__main__":
    main()
