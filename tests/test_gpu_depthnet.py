"""GPU: the HIP depth network (csrc/depthnet_kernel.h: fp32 matrix-core convolutions, BatchNorm folded at load time, padding /
up-sampling / normalisation / mirroring in the operand gather) against the golden G14 produced by the reference's own module, against
the plain-PyTorch fp32 twin (tests/depthnet_twin.py) on other sizes, its determinism contract, and the optimizer / helpers shims."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = {"s64x192": (3, 64, 192), "s192x640": (1, 192, 640)}


def _net(H, W, max_images, seed=0):
    import depthnet_twin as dt
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    return DepthNetHIP(Engine(H, W, 2), max_images, dt.depthnet_params(seed))


def _imgs(seed, N, H, W):
    import depthnet_twin as dt
    return torch.from_numpy(dt.sample_images(seed, N, H, W)).cuda()


def _check(disp, skips_nchw, ref_disp, ref_skips):
    assert disp.shape == ref_disp.shape
    assert float((disp - ref_disp).abs().max()) <= 2e-5
    for k, (s, r) in enumerate(zip(skips_nchw, ref_skips)):
        assert s.shape == r.shape, k
        assert float((s - r).abs().max()) <= 1e-4 * float(r.abs().max()), k


@pytest.mark.parametrize("tag", sorted(SIZES))
def test_depthnet_forward_vs_reference_golden(tag):
    g = load_golden("depthnet")
    N, H, W = SIZES[tag]
    net = _net(H, W, N, int(g["seed"]))
    x = _imgs(int(g[f"{tag}_img_seed"]), N, H, W)
    disps, skips = net(x=x)
    st = int(g[f"{tag}_disp_step"])
    d = disps[0].cpu().numpy()
    assert np.max(np.abs(d[:, :, ::st, ::st] - g[f"{tag}_disp"])) <= 2e-5
    for k, s in enumerate(skips):
        v = s.cpu().numpy().reshape(-1)[g[f"{tag}_skip{k}_idx"]]
        assert np.max(np.abs(v - g[f"{tag}_skip{k}_val"])) <= 1e-4 * g[f"{tag}_skip{k}_stats"][0], k
    # the C ABI's forward (no skips exposed) gives the same bits
    assert torch.equal(net.forward(x), disps[0])


@pytest.mark.parametrize("N,H,W", [(2, 256, 448), (5, 96, 320)])
def test_depthnet_vs_fp32_twin(N, H, W):
    import depthnet_twin as dt
    net = _net(H, W, N, 3)
    twin = dt.DepthNetTwin(dt.depthnet_params(3), device="cuda")
    x = _imgs(40 + N, N, H, W)
    disps, skips = net(x=x)
    with torch.no_grad():
        rd, rs = twin(x=x)
    _check(disps[0], skips, rd[0], rs)


def test_depthnet_determinism_contract():
    """decode(encode(x)) == forward(x); flip == forward(torch.flip(x)); one image alone == the same image inside a batch of 5"""
    H, W = 96, 320
    net = _net(H, W, 5, 1)
    x = _imgs(5, 5, H, W)
    full = net.forward(x)
    _, skips = net(x=x, return_disp=False)
    assert all(s.shape[0] == 5 and s.permute(0, 2, 3, 1).is_contiguous() for s in skips)
    dec, _ = net(x=None, skips=skips)
    assert torch.equal(dec[0], full)
    dec2, _ = net(x=None, skips=[s.contiguous() for s in skips])       # NCHW-contiguous skips are re-laid out
    assert torch.equal(dec2[0], full)
    assert torch.equal(net.forward(x, flip=True), net.forward(torch.flip(x, [3]).contiguous()))
    for i in (0, 3):
        assert torch.equal(net.forward(x[i:i + 1].contiguous()), full[i:i + 1])
    torch.cuda.synchronize()


def test_depthnet_refusals():
    import depthnet_twin as dt
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    with pytest.raises(RuntimeError, match="multiples of 32"):
        DepthNetHIP(Engine(240, 320, 2), 1)
    net = DepthNetHIP(Engine(64, 192, 2), 1)
    two = dict(dt.depthnet_params(0))
    two["feature_convs.1.0.conv.weight"] = torch.zeros(8, 64, 3, 3)
    with pytest.raises(RuntimeError, match="feature_convs.1.0.conv.weight"):
        net.load(two)
    wide = dict(dt.depthnet_params(0))
    wide["predict_disps.0.0.conv.weight"] = torch.zeros(1, 16, 3, 3)
    with pytest.raises(RuntimeError, match="predict_disps.0.0.conv.weight"):
        net.load(wide)
    short = dict(dt.depthnet_params(0))
    del short["iconvs.2.0.conv.bias"]
    with pytest.raises(RuntimeError, match="iconvs.2.0.conv.bias"):
        net.load(short)
    bad = dict(dt.depthnet_params(0))
    bad["encoder.encoder.layer3.0.bn2.running_var"] = torch.ones(128)
    with pytest.raises(RuntimeError, match="layer3.0.bn2.running_var"):
        net.load(bad)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        net.forward(_imgs(0, 1, 64, 192))


def test_optimize_window_with_depthnet_hip_against_the_twin():
    import depthnet_twin as dt
    import standins
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.optimizer import DepthOptimizer
    from tightly_coupled_sfm_amd._shared import get_engine
    from test_gpu_optimizer_shim import OPTIONS, _config
    B, S, H, W, iters = 1, 2, 64, 192, 3
    w = standins.make_window(B, S, H, W, seed0=70)
    pose_model, _ = standins.window_models(w, iters, device="cuda")
    twin = dt.DepthNetTwin(dt.depthnet_params(2), device="cuda")
    hip = DepthNetHIP(get_engine(H, W, 1), 4, dt.depthnet_params(2))
    res = {}
    for name, dm, extra in (("twin", twin, {}), ("hip", hip, {}), ("opt_in", twin, {"library_depth_net": True})):
        pm, _ = standins.window_models(w, iters, device="cuda")
        opt = DepthOptimizer(dict(OPTIONS, **extra), _config(B, iters), pm, dm, "09_02")
        res[name] = opt.optimize_window(0, standins.loader_batch(w, device="cuda"))
    a = res["twin"]
    for name in ("hip", "opt_in"):
        r = res[name]
        assert sorted(r) == sorted(a)
        for k in a:
            va, vr = a[k], r[k]
            if isinstance(va, (list, tuple)):
                assert len(va) == len(vr)
                va, vr = va[0], vr[0]
            if isinstance(va, (torch.Tensor, np.ndarray)):
                assert tuple(va.shape) == tuple(vr.shape) and str(va.dtype) == str(vr.dtype), k
        for key in ("depths_init", "disp_opt"):
            for x, y in zip(a[key] if isinstance(a[key], (list, tuple)) else [a[key]], r[key] if isinstance(r[key], (list, tuple)) else [r[key]]):
                x, y = torch.as_tensor(x).double().cpu(), torch.as_tensor(y).double().cpu()
                assert float(((x - y).abs() / x.abs().clamp_min(1e-6)).max()) <= 1e-4, key
        for key in ("poses_init", "poses_inv_init", "poses_opt"):
            if key in a:
                assert float((torch.as_tensor(a[key]).double() - torch.as_tensor(r[key]).double()).abs().max()) <= 1e-4, key
    # the opt-in path really ran the library's kernels: the cached wrapper exists for the twin
    from tightly_coupled_sfm_amd import depthnet
    assert id(twin) in depthnet._NETS


def test_get_disp_for_eigen_with_depthnet_hip():
    import depthnet_twin as dt
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.helpers import get_disp_for_eigen
    from tightly_coupled_sfm_amd._shared import get_engine
    H, W = 64, 192
    x = _imgs(9, 2, H, W)
    cfg = {"min_depth": 0.06, "max_depth": 2.67}
    hip = DepthNetHIP(get_engine(H, W, 1), 4, dt.depthnet_params(4))
    twin = dt.DepthNetTwin(dt.depthnet_params(4), device="cuda")
    a, b = get_disp_for_eigen(hip, x, cfg), get_disp_for_eigen(twin, x, cfg)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b) / np.abs(b).clip(1e-6)) <= 1e-4
