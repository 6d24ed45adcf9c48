"""CPU: the float64 twin of tests/depthnet_twin.py under autograd against the reference module's own parameter gradients (fixture
tests/golden/golden_depthnet_grad.npz, tests/golden/make_golden_depthnet_grad.py): the twin the GPU gradient tests compare with is
the reference's network under differentiation too."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def golden_grad_inputs(g):
    """(images [N,3,H,W] float32, R [N,1,H,W] float64) of the fixture"""
    import depthnet_twin as dt
    N, H, W = (int(v) for v in g["size"])
    x = torch.from_numpy(dt.sample_images(int(g["img_seed"]), N, H, W))
    R = torch.from_numpy(np.random.RandomState(int(g["r_seed"])).standard_normal((N, 1, H, W)))
    return x, R


def check_against_golden(g, grads, tol_of):
    """grads: name -> gradient tensor; per tensor the norm (relative) and the strided samples (error over the samples' share of the
    tensor norm) within tol_of(name)"""
    bad = {}
    for i, k in enumerate(g["names"]):
        k = str(k)
        v = grads[k].detach().double().cpu().reshape(-1).numpy()
        ref_n, st, ref_v = float(g[f"g{i}_norm"]), int(g[f"g{i}_stride"]), g[f"g{i}_val"]
        s = v[::st][:len(ref_v)]
        en = abs(np.linalg.norm(v) - ref_n) / ref_n
        es = np.linalg.norm(s - ref_v) / (ref_n * np.sqrt(len(ref_v) / v.size))      # in units of the tensor's RMS element
        if max(en, es) > tol_of(k):
            bad[k] = (en, es)
    return bad


def test_float64_twin_gradients_match_reference_module():
    import depthnet_twin as dt
    g = load_golden("depthnet_grad")
    x, R = golden_grad_inputs(g)
    sd = {k: v.double() for k, v in dt.depthnet_params(int(g["seed"])).items()}
    for k, v in sd.items():
        if not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    (dt.forward(sd, x.double()) * R).sum().backward()
    assert sorted(str(k) for k in g["names"]) == sorted(k for k, v in sd.items() if v.grad is not None)
    bad = check_against_golden(g, {k: v.grad for k, v in sd.items() if v.grad is not None}, lambda k: 1e-9)
    assert not bad, bad
