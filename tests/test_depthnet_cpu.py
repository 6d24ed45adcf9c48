"""CPU: the plain-PyTorch twin of the reference's depth network (tests/depthnet_twin.py) in fp32 against the golden G14 produced by
the reference's own module in float64 -- the bars the HIP depth network is held to on the GPU are reachable in fp32 -- and the
parameter set / module detection the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = {"s64x192": (3, 64, 192), "s192x640": (1, 192, 640)}


@pytest.mark.parametrize("tag", sorted(SIZES))
def test_depthnet_twin_fp32_vs_reference_golden(tag):
    import depthnet_twin as dt
    g = load_golden("depthnet")
    N, H, W = SIZES[tag]
    x = dt.sample_images(int(g[f"{tag}_img_seed"]), N, H, W)
    assert np.allclose([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()], [g[f"{tag}_img_sum"], g[f"{tag}_img_sumsq"]], rtol=1e-12)
    net = dt.DepthNetTwin(dt.depthnet_params(int(g["seed"])))
    with torch.no_grad():
        disps, skips = net(x=torch.from_numpy(x))
    st = int(g[f"{tag}_disp_step"])
    assert np.max(np.abs(disps[0].numpy()[:, :, ::st, ::st] - g[f"{tag}_disp"])) <= 2e-5
    for k, s in enumerate(skips):
        v = s.numpy().reshape(-1)[g[f"{tag}_skip{k}_idx"]]
        assert np.max(np.abs(v - g[f"{tag}_skip{k}_val"])) <= 1e-4 * g[f"{tag}_skip{k}_stats"][0], k
    assert g[f"{tag}_disp_stats"][2] > 0.05          # the sigmoid is not saturated


def test_depthnet_params_match_the_reference_names_and_shapes():
    import depthnet_twin as dt
    g = load_golden("depthnet")
    p = dt.depthnet_params(int(g["seed"]))
    assert list(p) == [str(n) for n in g["names"]]
    for n, s in zip(g["names"], g["shapes"]):
        assert tuple(p[str(n)].shape) == tuple(int(d) for d in s if d > 0), n
    assert all(v.dtype == torch.float32 for v in p.values())


def test_is_reference_depthnet_tells_the_twin_from_posenet():
    import depthnet_twin as dt
    import standins
    from tightly_coupled_sfm_amd.depthnet import is_reference_depthnet
    assert is_reference_depthnet(dt.DepthNetTwin(dt.depthnet_params(0)))
    assert not is_reference_depthnet(standins.PoseNetTwin(standins.posenet_params(0)))
    two = dict(dt.depthnet_params(0))
    two["feature_convs.1.0.conv.weight"] = torch.zeros(8, 64, 3, 3)
    assert not is_reference_depthnet(dt.DepthNetTwin(two))
    assert not is_reference_depthnet(object())
