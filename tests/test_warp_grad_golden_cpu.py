"""The float64 reference of the warp-gradient tests (autograd through oracle.torch_twin.warp) against the reference's own
inverse_warp2 under autograd: tests/golden/golden_warp_grad.npz (tests/golden/make_golden_warp_grad.py; 24 x 40, N = 3, one pose
with out-of-frame and Z-clamped pixels).  Outputs and the three gradients agree to 1e-9 relative, the figure
golden_depthnet_grad.npz is held to."""
import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
REL = 1e-9


def test_twin_gradients_equal_the_reference():
    from oracle import torch_twin as tw
    g = load_golden("warp_grad")
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    d_t, d_s, pose = (T(g[k]).requires_grad_() for k in ("depth_t", "depth_s", "pose"))
    rec, valid, pd, cd = tw.warp(T(g["src"]), d_t, d_s, -pose, T(g["K"]))
    assert np.array_equal(valid.numpy(), g["valid"])
    assert (g["valid"] == 0).sum() > 0 and (g["comp_depth"] == 1e-3).sum() > 0          # the fixture reaches the sentinel and the clamp
    for got, k in ((rec, "rec"), (pd, "proj_depth"), (cd, "comp_depth")):
        assert np.abs(got.detach().numpy() - g[k]).max() <= REL * np.abs(g[k]).max(), k
    ((rec * T(g["g_rec"])).sum() + (pd * T(g["g_pd"])).sum() + (cd * T(g["g_cd"])).sum()).backward()
    for p, k in ((d_t, "d_depth_t"), (d_s, "d_depth_s"), (pose, "d_pose")):
        got, ref = p.grad.numpy(), g[k]
        for n in range(ref.shape[0]):
            err = np.linalg.norm(got[n] - ref[n]) / np.linalg.norm(ref[n])
            print(k, n, "relative L2", err)
            assert err <= REL, (k, n, err)
        assert not got[ref == 0].any(), k
