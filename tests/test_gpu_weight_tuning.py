"""GPU: DepthOptimizer(options['weight_tuning'] = True) -- the reference's own epoch loop (optimization_experiments/optimizer.py:136-297)
on the library's differentiable operators.  32 x 64, B = 1, S = 2, config['iterations'] = 2, three epochs at lr 2e-4: the tuning chain's
images and intrinsics (tests/tuning_chain_inputs.py), a DepthNetModule of depthnet_twin.depthnet_params(0), standins.PoseNetTwin of
pose_loop_grad_inputs.params() as pose model, the 11-tuple batch form.

1. optimize_depth_encoder with fused_loss = False is, bit for bit, the loop written here from the public operators (INTEGRATION.md's
   tune_depth_encoder_coupled plus the get_disp_for_eigen call, without a step after the last epoch).
2. each switch moves the tensors it names and no others; the models given to the constructor keep their bits.
3. fused_loss = True (the default) against False: the epoch-0 losses, computed from the same weights, agree to 1e-3 relative with each
   other and with the float64 twin (loss_grad_inputs.e2e_twin at the library's poses and warp validity, as test_gpu_tuning_chain.py
   uses it for this shape).  Later epochs are printed, not judged: Adam's first steps are sign-like.
4. the result dict has golden G9's schema and the placement of the non-tuning path.
5. weight_tuning without a switch is a ValueError; options['optimizer'] = 'sgd' runs.
"""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depthnet_twin as dt  # noqa: E402
import pose_loop_grad_inputs as LI  # noqa: E402
import tuning_chain_inputs as TC  # noqa: E402

LG = TC.LG
SHAPE = TC.SHAPES[0]
B, S, ITERS, EPOCHS, LR = 1, 2, 2, 3, 2e-4
SWITCHES = ("optimize_depth_weights_bottleneck_beyond", "optimize_depth_weights_all", "optimize_depth_encoder", "optimize_pose_weights_all",
            "optimize_depth_pred", "optimize_depth_bottleneck_values")
CONFIG = {"minibatch": B, "device": "cuda", "min_depth": TC.DEPTH_RANGE[0], "max_depth": TC.DEPTH_RANGE[1], "iterations": ITERS,
          "camera_height": 1.65, "flow_type": "none"}


def _options(base=None, **kw):
    o = dict(TC.OPTIONS if base is None else base, epochs=EPOCHS, lr=LR, optimizer="adam", mode="scaled", avg_final_epochs=2, plotting=False,
             weight_tuning=True)
    o.update({k: False for k in SWITCHES})
    o.update(kw)
    return o


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _same(a, b):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _window():
    im = _t(TC.images(SHAPE))
    target, sources, K = im[:1].contiguous(), [im[1:2].contiguous(), im[2:3].contiguous()], _t(TC.intrinsics(SHAPE))[:1].contiguous()
    gts = [torch.zeros((B, 6), device="cuda") for _ in range(S)]
    return target, sources, K, (target, sources, gts, gts, None, K, None, None, None, None, None)


def _models():
    import standins
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    return DepthNetModule(dt.depthnet_params(0), max_images=TC.N_IMAGES).cuda(), standins.PoseNetTwin(LI.params()).cuda().eval()


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _unchanged(m, before):
    return all(_same(v, before[k]) for k, v in m.state_dict().items()) and all(p.grad is None for p in m.parameters())


def _run(options, depth_model=None, pose_model=None, capture=None):
    """-> (result dict, the optimiser, depth model given, pose model given); `capture`: list that receives the models the loop tuned"""
    from tightly_coupled_sfm_amd import optimizer as O
    d, p = _models()
    depth_model, pose_model = depth_model or d, pose_model or p
    opt = O.DepthOptimizer(options, dict(CONFIG), pose_model, depth_model, "09_02")
    r = opt.optimize_window(0, _window()[3])
    if capture is not None:
        capture.extend(opt.tuned_models)
    return r, opt, depth_model, pose_model


def _hand_loop(depth_model, pose_model, options, epochs):
    """INTEGRATION.md's tune_depth_encoder_coupled with the reference's last-epoch rule and its get_disp_for_eigen call -> (copy, losses)"""
    from tightly_coupled_sfm_amd import helpers, learning_helpers, losses
    from tightly_coupled_sfm_amd.train_mono import solve_pose_iteratively
    target, sources, K, _ = _window()
    imgs = torch.cat([target] + sources, 0)
    with torch.no_grad():
        disp_init = depth_model(x=imgs)[0][0][0:1].clone()
    model = copy.deepcopy(depth_model).eval()
    for name, p in model.named_parameters():
        p.requires_grad_(name.startswith("encoder."))
    opt = torch.optim.Adam(model.encoder.parameters(), lr=LR)
    depth = lambda d: learning_helpers.disp_to_depth(d, CONFIG["min_depth"], CONFIG["max_depth"])[1]
    history = []
    for epoch in range(epochs):
        opt.zero_grad()
        disp = model(x=imgs)[0][0]
        depths = [depth(disp[i:i + 1]) for i in range(S + 1)]
        _, _, outputs = solve_pose_iteratively(ITERS, depths, pose_model, target, sources, K, return_errors=True)
        loss = losses.compute_optimization_loss(options, target, disp[0:1], disp_init, outputs["fwd"], outputs["inv"], losses.SSIM_Loss())
        if epoch < epochs - 1:
            loss.backward()
            opt.step()
        history.append(loss.detach().reshape(()))
        helpers.get_disp_for_eigen(model, target, CONFIG)
    return model, torch.stack(history).cpu()


def test_encoder_tuning_is_the_hand_written_loop_bit_for_bit():
    o = _options(optimize_depth_encoder=True, fused_loss=False)
    tuned = []
    depth_model, pose_model = _models()
    before = _state(depth_model)
    r, _, _, _ = _run(o, depth_model, pose_model, capture=tuned)
    ref_model, ref_losses = _hand_loop(depth_model, pose_model, o, EPOCHS)
    print("losses", r["losses"].tolist(), "hand loop", ref_losses.tolist())
    assert _same(r["losses"], ref_losses)
    assert len(set(r["losses"].tolist())) == EPOCHS
    moved = 0
    for (k, a), (_, b) in zip(tuned[0].state_dict().items(), ref_model.state_dict().items()):
        assert _same(a, b), k
        moved += not _same(a, before[k])
    assert moved >= 20 and _unchanged(depth_model, before)
    # epochs = 1: the reference does not step after the last epoch
    tuned1 = []
    r1, _, _, _ = _run(dict(o, epochs=1), depth_model=depth_model, pose_model=pose_model, capture=tuned1)
    assert all(_same(v, before[k]) for k, v in tuned1[0].state_dict().items())
    assert r1["losses"].shape == (1,) and _same(r1["losses"], ref_losses[:1])


# every mode on the tuning chain's options; two of them on the reference's default switches (argmin, automasking) as well
MODES = [(s, "e2e") for s in SWITCHES] + [("optimize_depth_weights_all", "reference"), ("optimize_pose_weights_all", "reference")]


@pytest.mark.parametrize("switch,base", MODES, ids=[f"{s}-{b}" for s, b in MODES])
def test_each_switch_moves_what_it_names(switch, base):
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    from tightly_coupled_sfm_amd.posenet_train import PoseNetModule
    d, p = _models()
    bd, bp = _state(d), _state(p)
    tuned = []
    r, _, _, _ = _run(_options(TC.OPTIONS if base == "e2e" else TC.OPTIONS_DEFAULT, **{switch: True}), d, p, capture=tuned)
    td, tp = tuned
    assert _unchanged(d, bd) and _unchanged(p, bp)          # the models given to the constructor
    assert isinstance(td, DepthNetModule)
    enc = [k for k in bd if k.startswith("encoder.") and not k.endswith(("running_mean", "running_var"))]
    dec = [k for k in bd if not k.startswith("encoder.")]
    sd = td.state_dict()
    enc_moved, dec_moved = sum(not _same(sd[k], bd[k]) for k in enc), sum(not _same(sd[k], bd[k]) for k in dec)
    print(switch, "encoder tensors moved", enc_moved, "of", len(enc), "decoder", dec_moved, "of", len(dec), "losses", r["losses"].tolist())
    want = {"optimize_depth_encoder": (True, False), "optimize_depth_weights_bottleneck_beyond": (False, True),
            "optimize_depth_weights_all": (True, True)}.get(switch, (False, False))
    assert (enc_moved >= len(enc) // 2) == want[0] and (enc_moved > 0) == want[0]
    assert (dec_moved >= len(dec) // 2) == want[1] and (dec_moved > 0) == want[1]
    if switch == "optimize_depth_weights_bottleneck_beyond":
        assert all(q.grad is None for q in td.encoder.parameters())
    if switch == "optimize_pose_weights_all":
        assert isinstance(tp, PoseNetModule) and tp is not p
        moved = [not _same(v, bp[k]) for k, v in tp.state_dict().items() if k in bp]
        assert len(moved) >= 29 and sum(moved) >= len(moved) // 2
    else:
        assert tp is p
    if switch in ("optimize_depth_bottleneck_values", "optimize_depth_pred"):
        assert td is d
        assert not _same(r["depths_opt"][0], r["depths_init"][0])
    assert r["losses"].shape == (EPOCHS,) and bool(torch.isfinite(r["losses"]).all())


def _twin_epoch0_loss(r, depth_model):
    """the float64 twin of the epoch-0 loss, built as loss_grad_inputs.e2e_twin builds the chain's (disparities -> 1 / (a + b disp) ->
    torch_twin.photometric for the forward and the inverse pairs -> losses.compute_optimization_loss on the CPU with torch_twin.ssim) at
    the first pass's disparities, the library's warp validity and the library's epoch-0 poses -- the inverse pairs with the PoseNet's own
    inverse poses, which e2e_twin (inverse = -pose) cannot take"""
    from tightly_coupled_sfm_amd import losses
    from tightly_coupled_sfm_amd._shared import get_engine
    tw = LG.tw
    target, sources, K, _ = _window()
    imgs = torch.cat([target] + sources, 0)
    lo, hi = 1 / TC.DEPTH_RANGE[1], 1 / TC.DEPTH_RANGE[0]
    with torch.no_grad():
        disp = depth_model(x=imgs)[0][0]
        depths = [1.0 / (lo + (hi - lo) * disp[i:i + 1]) for i in range(S + 1)]
        pose_f, pose_i = r["poses_init"].cuda().contiguous(), r["poses_inv_init"].cuda().contiguous()
        tgt2, src, K2 = target.repeat(S, 1, 1, 1), torch.cat(sources, 0), K.repeat(S, 1, 1).contiguous()
        dt2, ds = depths[0].repeat(S, 1, 1, 1).contiguous(), torch.cat(depths[1:], 0).contiguous()
        e = get_engine(*SHAPE, 2 * S * B)
        mf = e.compute_photometric_error(tgt2, src, dt2, ds, pose_f, K2)["warp_valid"]
        mi = e.compute_photometric_error(src, tgt2, ds, dt2, pose_i, K2)["warp_valid"]
    f64 = lambda t: t.detach().cpu().double()
    d64 = f64(disp)
    z = [1.0 / (lo + (hi - lo) * d64[i:i + 1]) for i in range(S + 1)]
    zt2, zs = z[0].repeat(S, 1, 1, 1), torch.cat(z[1:], 0)
    fwd = tw.photometric(f64(tgt2), f64(src), zt2, zs, f64(pose_f), f64(K2))
    inv = tw.photometric(f64(src), f64(tgt2), zs, zt2, f64(pose_i), f64(K2))
    pack = lambda q, valid, p: dict(diff_img=q["diff"], valid_mask=f64(valid), weight_mask=q["weight"], poses=p)
    L = losses.compute_optimization_loss(TC.OPTIONS, f64(target), d64[:1], d64[:1], pack(fwd, mf, f64(pose_f)), pack(inv, mi, f64(pose_i)), tw.ssim)
    return float(L)


def test_fused_loss_against_unfused_and_schema():
    from conftest import load_golden
    d, p = _models()
    o = _options(optimize_depth_encoder=True)
    assert "fused_loss" not in o                     # the default
    rf, opt, _, _ = _run(o, d, p)
    ru, _, _, _ = _run(dict(o, fused_loss=False), d, p)
    L64 = _twin_epoch0_loss(rf, d)
    lf, lu = rf["losses"].tolist(), ru["losses"].tolist()
    print(f"epoch-0 loss fused {lf[0]:.9e} unfused {lu[0]:.9e} float64 twin {L64:.9e}; later epochs fused {lf[1:]} unfused {lu[1:]}")
    assert abs(lf[0] - lu[0]) <= 1e-3 * abs(lu[0]) and abs(lf[0] - L64) <= 1e-3 * abs(L64) and abs(lu[0] - L64) <= 1e-3 * abs(L64)
    assert len(lf) == EPOCHS and all(np.isfinite(lf)) and all(np.isfinite(lu))

    # schema: golden G9's keys, container kinds and dtypes, the placement of the non-tuning path
    H, W = SHAPE
    shapes = {"depths": (B, 1, H, W), "disp_opt": (B, H, W), "poses": (S * B, 6), "gt": (S * B, 6), "scale": (1,), "stacked": (S * B, ITERS, 6)}
    for line in load_golden("window48x160")["schema"]:
        key, kind, _, dtype, dev = str(line).split("|")
        assert key in rf, key
        v = rf[key]
        if kind.startswith("list"):
            assert isinstance(v, list) and len(v) == S + 1
            v = v[0]
        else:
            assert isinstance(v, torch.Tensor)
        on_device = key.startswith("depths_") or key in ("stacked_poses_opt", "stacked_poses_inv_opt")
        assert str(v.dtype) == dtype and v.device.type == ("cuda" if on_device else dev), (key, v.dtype, v.device)
        assert tuple(v.shape) == next(s for k, s in shapes.items() if key.startswith(k)), (key, v.shape)
    assert rf["stacked_poses_opt"].shape == (S * B, ITERS, 6) and rf["stacked_poses_inv_opt"].shape == (S * B, ITERS, 6)
    assert len(opt.full_results) == EPOCHS and set(rf) <= set(opt.full_results[0])
    assert torch.equal(rf["scale_factor"], torch.FloatTensor([1])) and torch.equal(rf["scale_factor_init"], torch.FloatTensor([1]))
    # poses_opt: the average of the last avg_final_epochs (2) epochs' poses
    last = torch.stack([opt.full_results[k]["poses_opt"] for k in (EPOCHS - 2, EPOCHS - 1)]).mean(0)
    assert torch.allclose(rf["poses_opt"], last, rtol=1e-6, atol=1e-9)
    assert not rf["depths_opt"][0].requires_grad and rf["depths_opt"][0].grad_fn is None


def test_no_switch_is_an_error_and_sgd_runs():
    from tightly_coupled_sfm_amd import optimizer as O
    d, p = _models()
    with pytest.raises(ValueError):
        O.DepthOptimizer(_options(), dict(CONFIG), p, d, "09_02")
    before = _state(d)
    tuned = []
    r, _, _, _ = _run(_options(optimize_depth_weights_all=True, optimizer="sgd", lr=1e-3, mode="unscaled"), d, p, capture=tuned)
    assert bool(torch.isfinite(r["losses"]).all()) and _unchanged(d, before)
    assert any(not _same(v, before[k]) for k, v in tuned[0].state_dict().items())
    assert r["scale_factor"].shape == (1,) and r["scale_factor_init"].shape == (1,)          # (DNet's ground-plane scale of a random frame: its value is not judged)
