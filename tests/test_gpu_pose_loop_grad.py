"""GPU: train_mono.solve_pose_iteratively under autograd -- the coupled PoseNet / warp loop as the composition of
Engine.posenet_input_autograd (tcsfm_warp_backward) and PoseNetHIP.__call__ (tcsfm_posenet_backward), so that the poses carry the
gradient with respect to the depths that the reference's loss.backward() follows.

Frames 16 x 24, (B, S) = (1, 2) and (2, 2): N = 4 and 8, the network's two work-split regimes; num_iter = 3; disparity / depth leaves,
no depth network (tests/pose_loop_grad_inputs.py: inputs, the float64 twin of the loop, the CPU search of the inputs).

  1  under grad, stacked_poses, the poses and every map of outputs['fwd' | 'inv'] have the bits of the no-grad (fused) call
  2  the depth gradients of sum R * stacked_poses equal, bit for bit, the hand-composed sequence of PoseNetHIP.backward,
     Engine.inverse_warp2_backward and torch adds (x + 0.0 on both sides, for -0.0); a repeat run gives the same bits
  3  the same scalar's disparity gradient against float64 autograd of the torch twin of the loop -- PoseNetTwin.double() with the
     library's ReLU decisions pinned and the warp twin of the warp-gradient tests -- on inputs at which every sample of every warp
     keeps its bilinear cell and validity with 8 x headroom (committed candidates hold for both configurations: the fallback bar of
     relative L2 <= 1e-2 is not in use); judged by the ratio rule of posenet_grad_inputs.judge
  4  32 x 64, DepthNetModule, tuning_chain_inputs' images and options (+ l_pose_consist): one epoch of INTEGRATION.md's tune_depth_encoder_coupled gives
     finite encoder gradients that differ from those with the same poses detached; three Adam epochs at lr 2e-4 move the parameters
  5  solve_pose_iteratively's poses have a grad_fn (fails before the feature exists)

MEASURED on an MI355X (TCSFM_TEST_POSE_LOOP_REPORT=<file> keeps the lines):
  check 3, |hip - f64| against |float32 twin loop - f64| (the float32 twin's warp is the larger error: ratios far below 1):
    few  (N 4)   d_disp_t  relative L2 1.7e-6 (twin 3.2e-5, ratio 0.05) | max/RMS 1.1e-5 (1.6e-4, 0.07)
                 d_disp_s  relative L2 1.1e-6 (twin 2.9e-5, ratio 0.04) | max/RMS 7.0e-6 (3.7e-4, 0.02)
    many (N 8)   d_disp_t  relative L2 1.2e-6 (twin 2.5e-5, ratio 0.05) | max/RMS 6.9e-6 (2.3e-4, 0.03)
                 d_disp_s  relative L2 9.2e-7 (twin 2.3e-5, ratio 0.04) | max/RMS 8.6e-6 (3.3e-4, 0.03)
    the library's warps against the float64 loop's: no cell or validity flip, coordinate difference 3.0e-7 .. 4.3e-7 px, nearest
    boundary 7.9e-5 .. 1.8e-4 px (>= 180 x the difference)
  check 4: the encoder's 60 gradients differ by 0.58 .. 1.07 (relative L2) from those with the poses detached, l_pose_consist on;
    losses of the three epochs 0.29872, 0.31612, 0.31275 (a seeded random PoseNet: the loop moves, it is not asked to descend)
  checks 1, 2 and 5 are bitwise and hold as stated; in 2 the three-term sum into an iterate's gradient is autograd's order: the
    stacked row, the next iterate's gradient, then the warp's
"""
import copy
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pose_loop_grad_inputs as LI      # noqa: E402
import posenet_layers as PL             # noqa: E402
import standins                         # noqa: E402
import warp_grad_inputs as WG           # noqa: E402

CONFIGS = list(LI.CONFIGS)
UNPINNED_REL_L2 = 1e-2                  # the bar of tests/test_gpu_depthnet_grad.py, only where no committed candidate holds


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_POSE_LOOP_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _same(a, b):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _model():
    return standins.PoseNetTwin(LI.params()).cuda().eval()


def _seed(config):
    s = LI.chosen(config)
    return LI.CANDIDATES[0] if s is None else s


@functools.lru_cache(maxsize=None)
def _dev(config):
    inp = LI.inputs(config, _seed(config))
    B, S = LI.CONFIGS[config]
    return dict(tgt=_t(inp["tgt"]), srcs=[_t(inp["srcs"][i]) for i in range(S)], disp_t=_t(inp["disp_t"]),
                disp_s=[_t(inp["disp_s"][i]) for i in range(S)], K=_t(inp["K"]), R=_t(inp["R"]))


def _depths(config, leaves=False):
    """depth maps [target, source 1 .. S] from the disparities (learning_helpers.disp_to_depth, no grad): leaves of their own"""
    from tightly_coupled_sfm_amd import learning_helpers
    d = _dev(config)
    with torch.no_grad():
        out = [learning_helpers.disp_to_depth(x, *LI.DEPTH_RANGE)[1].clone() for x in [d["disp_t"]] + d["disp_s"]]
    return [x.requires_grad_(True) for x in out] if leaves else out


def _solve(config, depths, return_errors=True):
    from tightly_coupled_sfm_amd import train_mono
    d = _dev(config)
    return train_mono.solve_pose_iteratively(LI.NUM_ITER, depths, _model(), d["tgt"], d["srcs"], d["K"], return_errors=return_errors)


def _stacked(config, outputs):
    return torch.cat([outputs["fwd"]["poses"], outputs["inv"]["poses"]], 0)


# ---- 5 and 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
def test_poses_carry_a_grad_fn_and_keep_the_fused_bits(config):
    with torch.no_grad():
        p0, pi0, o0 = _solve(config, _depths(config))
    assert all(p.grad_fn is None for p in p0 + pi0)
    leaves = _depths(config, leaves=True)
    p1, pi1, o1 = _solve(config, leaves)
    assert all(p.grad_fn is not None for p in p1 + pi1), "the poses do not depend on the depths"
    assert all(_same(a, b) for a, b in zip(p0 + pi0, p1 + pi1))
    for side in ("fwd", "inv"):
        assert sorted(o0[side]) == sorted(o1[side])
        for k in o0[side]:
            assert _same(o0[side][k].float(), o1[side][k].float()), (side, k)
        assert o1[side]["poses"].grad_fn is not None and o1[side]["diff_img"].grad_fn is not None
    for k in o0["comb"]:
        assert _same(o0["comb"][k], o1["comb"][k]), k
    # the pose model's parameters take no gradient, whatever their requires_grad says (documented: a frozen copy is evaluated)
    assert all(p.requires_grad for p in _model().parameters())
    _stacked(config, o1).sum().backward()
    assert all(p.grad is None for p in _model().parameters()) and all(l.grad is not None for l in leaves)
    # every other case keeps today's path: one iteration, or no depth that requires grad
    from tightly_coupled_sfm_amd import train_mono
    d = _dev(config)
    one = train_mono.solve_pose_iteratively(1, _depths(config, leaves=True), _model(), d["tgt"], d["srcs"], d["K"])
    assert all(p.grad_fn is None for p in one[0] + one[1])
    assert all(p.grad_fn is None for p in _solve(config, _depths(config), return_errors=False)[0])


# ---- 2 --------------------------------------------------------------------------------------------------------------------------
def _hand_composed(config):
    """the loop and its backward by explicit calls -> (stacked [N, iters, 6], depth gradients [target, source 1 .. S], tapes)"""
    from tightly_coupled_sfm_amd import train_mono
    from tightly_coupled_sfm_amd._shared import get_engine
    d = _dev(config)
    B, S = LI.CONFIGS[config]
    split, N = S * B, 2 * S * B
    eng = get_engine(LI.H, LI.W, N)
    net = train_mono._library_posenet(_model(), eng, N)
    depths = _depths(config)
    td, sdp = depths[0].repeat(S, 1, 1, 1), torch.cat(depths[1:], 0)
    ti, si = d["tgt"].repeat(S, 1, 1, 1), torch.cat(d["srcs"], 0)
    tgt, src = torch.cat([ti, si], 0).contiguous(), torch.cat([si, ti], 0).contiguous()
    d_t, d_s = torch.cat([td, sdp], 0).contiguous(), torch.cat([sdp, td], 0).contiguous()
    K = d["K"].repeat(2 * S, 1, 1).contiguous()
    with torch.no_grad():
        p = [net(torch.cat([tgt, src], 1).contiguous())]
        tapes = []
        for it in range(1, LI.NUM_ITER):
            c, tape = net.forward_train(eng.posenet_input(tgt, src, d_t, d_s, p[-1], K))
            tapes.append(tape)
            p.append(p[-1] + c)
        R = d["R"]
        g_dt = g_ds = None
        g_p = R[:, -1].contiguous()
        for it in range(LI.NUM_ITER - 1, 0, -1):
            g_x = net.backward(tapes[it - 1], g_p)
            want_pose = it > 1                                   # the first iterate does not depend on the depths
            a, b, g_neg = eng.inverse_warp2_backward(src, d_t, d_s, -p[it - 1], K, g_rec=g_x[:, 3:6].contiguous(), want=(True, True, want_pose))
            g_dt, g_ds = (a, b) if g_dt is None else (g_dt + a, g_ds + b)
            if want_pose:
                g_p = (R[:, it - 1] + g_p) + (-g_neg)            # stack's row, the next iterate's, then the warp's: autograd's order
        g_target = g_ds[split:] + g_dt[:split]
        g_source = g_ds[:split] + g_dt[split:]
        grads = [g_target.view(S, B, 1, LI.H, LI.W).sum(0)] + [g_source[B * i:B * (i + 1)] for i in range(S)]
    return torch.stack(p, 1), grads, tapes, net


def _autograd_run(config):
    leaves = _depths(config, leaves=True)
    _, _, out = _solve(config, leaves)
    st = _stacked(config, out)
    (st * _dev(config)["R"]).sum().backward()
    return st.detach(), [l.grad.clone() for l in leaves]


@pytest.mark.parametrize("config", CONFIGS)
def test_composition_is_exact_and_repeatable(config):
    st, grads = _autograd_run(config)
    st_h, grads_h, _, _ = _hand_composed(config)
    assert _same(st, st_h)
    for k, (a, b) in enumerate(zip(grads, grads_h)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k
        assert _same(a + 0.0, b + 0.0), ("depth", k, float((a - b).abs().max()))
    st2, grads2 = _autograd_run(config)
    assert _same(st, st2) and all(_same(a, b) for a, b in zip(grads, grads2))


# ---- 3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
def test_disparity_gradient_against_the_float64_twin_loop(config):
    from tightly_coupled_sfm_amd import learning_helpers
    d, inp = _dev(config), LI.inputs(config, _seed(config))
    B, S = LI.CONFIGS[config]
    N = 2 * S * B
    leaves = [x.clone().requires_grad_(True) for x in [d["disp_t"]] + d["disp_s"]]
    depths = [learning_helpers.disp_to_depth(x, *LI.DEPTH_RANGE)[1] for x in leaves]
    _, _, out = _solve(config, depths)
    st = _stacked(config, out)
    (st * d["R"]).sum().backward()
    got = dict(d_disp_t=leaves[0].grad.cpu().numpy(), d_disp_s=torch.stack([l.grad for l in leaves[1:]], 0).cpu().numpy())
    # the library's ReLU decisions, call by call: the plain first call's from its read-out, the others from the hand-composed tapes
    st_h, _, tapes, net = _hand_composed(config)
    assert _same(st, st_h)
    relu = lambda raw, scsh: (torch.relu(raw * scsh[:, :, 0, None, None] + scsh[:, :, 1, None, None]) > 0).cpu()
    ti, si = d["tgt"].repeat(S, 1, 1, 1), torch.cat(d["srcs"], 0)
    net(torch.cat([torch.cat([ti, si], 0), torch.cat([si, ti], 0)], 1).contiguous())
    masks = [[relu(*net.layer(l, N)) for l in range(1, 8)]]       # (first call: no backward ran on it; its gradient is not needed)
    masks += [[(net.tape_layer(t, l, N)[3] > 0).cpu() for l in range(1, 8)] for t in tapes]
    r64, r32 = [], []
    ref = LI.twin_loop(inp, torch.float64, masks=masks, grad=True, record=r64)
    t32 = LI.twin_loop(inp, torch.float32, masks=masks, grad=True, record=r32)
    st = st.detach()
    assert float(np.abs(ref["stacked"] - st.cpu().double().numpy()).max()) < 1e-5, "the pinned float64 loop is not the library's loop"
    # the library's warps, in float64 at its own fp32 poses and depths, against the float64 loop's: same cells, same validity, headroom
    tag = f"loop/{config}"
    held = LI.chosen(config) is not None
    with torch.no_grad():
        dep = [x.cpu().numpy() for x in depths]
    td, sdp = np.tile(dep[0], (S, 1, 1, 1)), np.concatenate(dep[1:], 0)
    geo = dict(src=np.zeros((N, 3, LI.H, LI.W)), K=np.tile(inp["K"], (2 * S, 1, 1)), depth_t=np.concatenate([td, sdp], 0))
    for it in range(1, LI.NUM_ITER):
        flips, diff, boundary = LI.geometry_margins(r64[it - 1], WG.geometry(dict(geo, pose=st[:, it - 1].cpu().numpy())))
        _report(f"{tag}\twarp {it}\tflips={flips}\tcoordinate difference library / float64={diff:.3e}\tnearest boundary={boundary:.3e}")
        if held:
            assert flips == 0 and boundary >= LI.HEADROOM * diff, (it, flips, diff, boundary)
    fails, figs = LI.judge(got, ref, t32)
    for k, f in figs.items():
        _report(f"{tag}\t{k}\trel L2 hip-f64={f['rel_l2']:.3e} f32-f64={f['f32_rel_l2']:.3e} ratio={f['ratio_rel_l2']:.2f}"
                f"\tmax/RMS hip-f64={f['max_rms']:.3e} f32-f64={f['f32_max_rms']:.3e} ratio={f['ratio_max_rms']:.2f}")
    if held:
        assert not fails, fails
    else:
        assert all(f["rel_l2"] <= UNPINNED_REL_L2 for f in figs.values()), figs


# ---- 4 --------------------------------------------------------------------------------------------------------------------------
def test_tuning_epoch_with_the_coupled_poses():
    """INTEGRATION.md's tune_depth_encoder_coupled on the tuning chain's 32 x 64 inputs: the PoseNet path contributes to the encoder's
    gradients, and the loop moves"""
    import depthnet_twin as dt
    import tuning_chain_inputs as TC
    from tightly_coupled_sfm_amd import learning_helpers, losses, train_mono
    from tightly_coupled_sfm_amd._shared import get_engine
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    shape = TC.SHAPES[0]
    im = _t(TC.images(shape))
    target, sources, K = im[:1].contiguous(), [im[1:2].contiguous(), im[2:3].contiguous()], _t(TC.intrinsics(shape))[:1].contiguous()
    options = dict(TC.OPTIONS, l_pose_consist=True)
    pose_model = _model()
    orig = DepthNetModule(dt.depthnet_params(TC.SEED[shape]), max_images=TC.N_IMAGES).cuda()
    depth = lambda x: learning_helpers.disp_to_depth(x, *TC.DEPTH_RANGE)[1]
    with torch.no_grad():
        disp_init = orig(x=im)[0][0][0:1].clone()

    def epoch(model, detach):
        disp = model(x=im)[0][0]
        depths = [depth(disp[i:i + 1]) for i in range(3)]
        if detach:      # the same poses as constants: what the chain was before the PoseNet's backward
            with torch.no_grad():
                _, _, po = train_mono.solve_pose_iteratively(LI.NUM_ITER, [x.detach() for x in depths], pose_model, target, sources, K, return_errors=True)
            S = 2
            d_t, d_s = depths[0].repeat(S, 1, 1, 1), torch.cat(depths[1:], 0)
            tgt, src = target.repeat(S, 1, 1, 1), torch.cat(sources, 0)
            eng = get_engine(*shape, 2 * S)
            pf, pi = po["fwd"]["poses"][:, -1].contiguous(), po["inv"]["poses"][:, -1].contiguous()
            rf = eng.compute_photometric_error(tgt, src, d_t, d_s, pf, K.repeat(S, 1, 1))
            ri = eng.compute_photometric_error(src, tgt, d_s, d_t, pi, K.repeat(S, 1, 1))
            fwd, inv = (dict(r, valid_mask=r["warp_valid"], poses=q) for r, q in ((rf, po["fwd"]["poses"]), (ri, po["inv"]["poses"])))
        else:
            _, _, out = train_mono.solve_pose_iteratively(LI.NUM_ITER, depths, pose_model, target, sources, K, return_errors=True)
            fwd, inv = out["fwd"], out["inv"]
        return losses.compute_optimization_loss(options, target, disp[0:1], disp_init, fwd, inv, losses.SSIM_Loss())

    def encoder_grads(detach):
        model = copy.deepcopy(orig).eval()
        for name, p in model.named_parameters():
            p.requires_grad_(name.startswith("encoder."))
        L = epoch(model, detach)
        L.backward()
        return L.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    L1, G1 = encoder_grads(False)
    L0, G0 = encoder_grads(True)
    assert abs(float(L1) - float(L0)) <= 1e-6 * abs(float(L0)), "the detached chain is not the same forward"
    assert len(G1) == 60 and sorted(G1) == sorted(G0)
    assert all(bool(torch.isfinite(g).all()) for g in G1.values())
    rel = {k: PL.rel_l2(G1[k], G0[k]) for k in G1}
    _report(f"loop/chain 32x64\tencoder gradients with / without the PoseNet path: relative difference {min(rel.values()):.3e} .. {max(rel.values()):.3e}")
    assert max(rel.values()) > 1e-4 and sum(not torch.equal(G1[k], G0[k]) for k in G1) >= 55, rel
    # the snippet itself, three epochs at the reference's learning rate
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    ns = {}
    exec(re.search(r"```python\n(# the same loop with the poses recomputed in every epoch.*?)```", text, re.S).group(1), ns)
    before = {k: v.clone() for k, v in orig.state_dict().items()}
    config = dict(min_depth=TC.DEPTH_RANGE[0], max_depth=TC.DEPTH_RANGE[1], iterations=LI.NUM_ITER)
    model, hist = ns["tune_depth_encoder_coupled"](orig, pose_model, target, sources, K, options, config, epochs=3, lr=2e-4)
    _report("loop/chain 32x64\tlosses\t" + "\t".join(f"{v:.9e}" for v in hist))
    assert all(np.isfinite(hist)) and len(set(hist)) == 3 and abs(hist[0] - float(L1)) <= 1e-6 * abs(float(L1))
    tuned = model.state_dict()
    assert any(not torch.equal(tuned[k], before[k]) for k in before if k.startswith("encoder."))
    assert all(torch.equal(tuned[k], before[k]) for k in before if not k.startswith("encoder."))
    assert all(torch.equal(v, before[k]) for k, v in orig.state_dict().items())
    assert all(p.grad is None for p in pose_model.parameters())
