"""GPU: the PoseNet's gradient with respect to its PARAMETERS (csrc/posenet_wgrad_kernel.h; tcsfm_posenet_param_backward /
tcsfm_posenet_load_device, PoseNetHIP.param_backward / .load_device, posenet_train.PoseNetModule) against float64.

tests/posenet_param_grad_inputs.py holds the references: the float64 twin with the ReLU decisions pinned to the library's own
(act_out > 0 of tcsfm_debug_posenet_tape_layer) and its parameters requiring grad, the same twin in float32 as the yardstick, the
judge per tensor -- relative L2 and max error / RMS each within max(floor, 4 x the yardstick's own figure) -- and the derived
bound n u D_c of the degenerate conv1.0.bias.  tests/test_posenet_param_grad_inputs_cpu.py shows that nine planted faults fail
that judge at every small shape used here.

  1  all 30 gradients under the judge: dense and one-hot cotangents; base, offset and gamma parameter sets; a frame of 0.45f (there
     conv1.0.weight's reference gradient is exactly zero: the library's must be finite, the other tensors are judged)
  2  bitwise: d_imgs is tcsfm_posenet_backward's; d_imgs = NULL and any subset of requested gradients leave the others' bits
     unchanged; a second run gives the same bits; an all-zero d_pose gives exactly zero everywhere; the pose after load_device is the
     pose after load of the same values
  3  every filter of every conv*.0.weight gradient sums to zero: |mean| <= FLOOR_REL_L2 x the filter's RMS (the chain rule's two
     terms each sum to zero in double; the n fp32 roundings of the results give at most u x RMS)
  4  PoseNetModule: autograd gradients equal param_backward's bit for bit; two calls in one graph accumulate; a frozen parameter's
     .grad stays None; a deep copy is independent; an in-place update followed by a forward changes the pose, and a backward of the
     older graph raises; bad arguments are refused before the device is touched

MEASURED on an MI355X (TCSFM_TEST_POSENET_PARAM_GRAD_REPORT=<file> keeps one line per case, cotangent and tensor, and a summary line).
Worst  error / bound  over the parameter sets, the two cotangents and the 29 judged tensors (1 = the judge's limit; the bound is
max(floor, 4 x the float32 twin's error), so 0.25 means "as accurate as the float32 twin") -- relative L2 | max error / RMS | largest
relative L2 | conv1.0.bias: worst |g_c| / (n u D_c):
    5x9-N1of1          0.33 (conv2.0.bias; base, one-hot         ) | 0.44 (conv2.0.bias; base, dense           ) | 3.5e-06 | 1.4e-01
    17x33-N2of2        0.26 (conv3.1.weight; base, dense         ) | 0.33 (conv7.0.weight; gamma, one-hot      ) | 1.9e-06 | 2.5e-03
    17x33-N5of5        0.39 (conv1.1.weight; gamma, dense        ) | 0.45 (conv1.1.weight; gamma, dense        ) | 2.5e-06 | 1.3e-03
    37x53-N7of12       0.29 (conv5.1.bias; gamma, one-hot        ) | 0.42 (conv4.1.weight; gamma, one-hot      ) | 1.9e-06 | 2.4e-04
    64x64-N5of5        0.26 (conv3.1.weight; base, one-hot       ) | 0.35 (conv7.1.weight; gamma, one-hot      ) | 1.8e-06 | 1.3e-04
    96x100-N2of2       0.33 (conv2.0.bias; base, dense           ) | 0.40 (conv2.0.bias; base, dense           ) | 2.1e-06 | 7.4e-05
    192x640-N2of2      0.22 (conv5.0.weight; base, one-hot       ) | 0.27 (conv6.1.bias; base, one-hot         ) | 1.6e-06 | 3.9e-06
    all-0.45-17x33     0.26 (conv4.1.bias; base, one-hot         ) | 0.27 (conv5.0.weight; gamma, one-hot      ) |    -    | 1.3e-03
In the frame of 0.45f the float64 reference of conv1.1.weight is rounding noise (1e-14) where library and float32 twin give
exactly zero: its relative L2 of 1 sits inside 4 x the yardstick's own 1 and is left out of the "largest relative L2" column.
Checks 2, 3 and 4 are bitwise or structural and hold as stated; in 3 a filter whose channel no ReLU lets through has an identically
zero gradient (gamma set) and is required to be exactly zero instead.
"""
import copy
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import posenet_grad_inputs as GI           # noqa: E402
import posenet_layers as PL                # noqa: E402
import posenet_param_grad_inputs as PG     # noqa: E402


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_POSENET_PARAM_GRAD_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _net(H, W, M, sd):
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    return PoseNetHIP(Engine(H, W, M), M, sd)


def _masks(net, tape, N):
    return [(net.tape_layer(tape, l, N)[3] > 0).cpu().contiguous() for l in range(1, 8)]


def _same(a, b):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _accuracy(tag, sd, x, net, cotangents, zero_conv1_weight=False):
    N = x.shape[0]
    xg = x.cuda()
    pose, tape = net.forward_train(xg)
    masks = _masks(net, tape, N)
    fails = []
    for name, d in cotangents:
        d_imgs, g = net.param_backward(xg, tape, d.cuda())
        assert _same(d_imgs, net.backward(tape, d.cuda()))
        ref, _ = PG.param_grads_pinned(sd, x, masks, d)
        yard, _ = PG.param_grads_pinned(sd, x, masks, d, torch.float32)
        skip = ()
        if zero_conv1_weight:
            assert float(ref["conv1.0.weight"].abs().max()) == 0.0
            assert bool(torch.isfinite(g["conv1.0.weight"]).all())
            skip = ("conv1.0.weight",)
        bad, figs = PG.judge_all(g, ref, yard, PG.conv1_bias_bound(sd, x, masks, d), skip=skip)
        for k, f in figs.items():
            if k == PG.DEGENERATE:
                _report(f"accuracy\t{tag}\t{name}\t{k}\tworst |g| / (n u D)={f['worst_over_bound']:.3e}")
            else:
                _report(f"accuracy\t{tag}\t{name}\t{k}\trel L2 hip-f64={f['rel_l2']:.3e} f32-f64={f['f32_rel_l2']:.3e} bound={f['bound_rel_l2']:.3e}"
                        f"\tmax/RMS hip-f64={f['max_rms']:.3e} f32-f64={f['f32_max_rms']:.3e} bound={f['bound_max_rms']:.3e}")
        (r1, k1), (r2, k2), big = PG.worst({k: f for k, f in figs.items()})
        _report(f"summary\t{tag}\t{name}\tworst rel L2 / bound={r1:.2f} ({k1})\tworst max/RMS / bound={r2:.2f} ({k2})\tlargest rel L2={big:.1e}"
                f"\tconv1.0.bias / bound={figs[PG.DEGENERATE]['worst_over_bound']:.2e}")
        if bad:
            fails.append((name, {k: figs[k] for k in bad}))
    assert not fails, (tag, fails)


def _cotangents(N, seed):
    return [("dense", GI.cotangent_dense(N, seed)), (f"one-hot[{N - 1},4]", GI.cotangent_onehot(N, N - 1, 4))]


_ACC = [(c, p) for c in PG.CASES for p in ("base", "offset", "gamma") if c[0] < 192 or p == "base"]


# ---- 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pset", _ACC, ids=[f"{PG.CASE_IDS[PG.CASES.index(c)]}-{p}" for c, p in _ACC])
def test_parameter_gradients_vs_pinned_float64(case, pset):
    H, W, N, M = case
    sd = PL.PARAM_SETS[pset](3)
    x = PL.images(H, W, N, seed=5)
    _accuracy(f"{H}x{W}-N{N}of{M}-{pset}", sd, x, _net(H, W, M, sd), _cotangents(N, H + N))


@pytest.mark.parametrize("pset", ["base", "gamma"])
def test_constant_frame_zero_variance_groups(pset):
    H, W, N = 17, 33, 2
    sd = PL.PARAM_SETS[pset](3)
    x = GI.constant_frames(H, W, N)
    _accuracy(f"all-0.45-{H}x{W}-{pset}", sd, x, _net(H, W, N, sd), _cotangents(N, 1), zero_conv1_weight=True)


# ---- 2 and 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", [(17, 33, 2), (37, 53, 5), (96, 100, 2)])
def test_bitwise_subsets_repeats_zero_cotangent_and_filter_sums(H, W, N):
    sd = PL.PARAM_SETS["gamma"](3)
    net = _net(H, W, N, sd)
    x = PL.images(H, W, N, seed=5).cuda()
    d = GI.cotangent_dense(N, 2).cuda()
    d[d == 0] = 0.5
    _, tape = net.forward_train(x)
    d_imgs, full = net.param_backward(x, tape, d)
    assert _same(d_imgs, net.backward(tape, d)) and sorted(full) == sorted(PG.NAMES)
    again_imgs, again = net.param_backward(x, tape, d)
    assert _same(again_imgs, d_imgs) and all(_same(again[k], full[k]) for k in PG.NAMES)
    subsets = [["conv1.0.weight"], ["conv4.1.weight", "pose_pred.bias"], ["conv7.0.bias", "conv2.0.weight", "conv2.1.bias"],
               [k for k in PG.NAMES if k.endswith("0.weight")], ["pose_pred.weight"], []]
    for want in subsets:
        for need in (True, False):
            di, g = net.param_backward(x if "conv1.0.weight" in want else None, tape, d, want=want, need_d_imgs=need)
            assert (di is None) == (not need) and sorted(g) == sorted(want)
            assert di is None or _same(di, d_imgs)
            assert all(_same(g[k], full[k]) for k in want), (want, need)
    zi, zg = net.param_backward(x, tape, torch.zeros_like(d))
    assert not bool(zi.any()) and all(not bool(v.any()) for v in zg.values())
    for l in range(1, 8):
        w = full[f"conv{l}.0.weight"].double().flatten(1)
        rms = w.pow(2).mean(1).sqrt()
        live = rms > 0                     # (a filter whose channel no ReLU lets through has an exactly zero gradient)
        assert int(live.sum()) >= w.shape[0] // 2 and not bool(w[~live].any())
        assert float((w[live].mean(1).abs() / rms[live]).max()) <= PL.FLOOR_REL_L2, l


def test_load_device_gives_the_bits_of_load():
    H, W, N = 37, 53, 5
    sd = PL.PARAM_SETS["offset"](3)
    x = PL.images(H, W, N, seed=5).cuda()
    a = _net(H, W, N, sd)
    b = _net(H, W, N, PL.PARAM_SETS["base"](4))
    b.load_device({k: torch.as_tensor(v).cuda() for k, v in sd.items()})
    pa, ta = a.forward_train(x)
    pb, tb = b.forward_train(x)
    assert _same(pa, pb) and _same(ta, tb) and _same(a(x[:2].contiguous()), b(x[:2].contiguous()))
    d = GI.cotangent_dense(N, 1).cuda()
    (ia, ga), (ib, gb) = a.param_backward(x, ta, d), b.param_backward(x, tb, d)
    assert _same(ia, ib) and all(_same(ga[k], gb[k]) for k in PG.NAMES)
    # absent biases / affine parameters: 0, 1, 0 on both paths
    bare = {k: v for k, v in sd.items() if k.endswith("0.weight") or k.startswith("pose_pred")}
    a.load(bare)
    b.load_device({k: torch.as_tensor(v).cuda() for k, v in bare.items()})
    assert _same(a(x), b(x))


# ---- 4 --------------------------------------------------------------------------------------------------------------------------
def test_module_autograd_accumulation_freezing_copies_and_stale_graphs():
    from tightly_coupled_sfm_amd.posenet_train import PoseNetModule
    H, W, N = 37, 53, 4
    sd = PL.PARAM_SETS["base"](3)
    x = PL.images(H, W, N, seed=5).cuda()
    x2 = PL.images(H, W, N, seed=6).cuda()
    d = GI.cotangent_dense(N, 4).cuda()
    net = _net(H, W, N, sd)
    pe, te = net.forward_train(x)
    ie, ge = net.param_backward(x, te, d)
    mod = PoseNetModule(sd, max_images=N).cuda()
    with torch.no_grad():
        plain = mod(x)
    assert plain.grad_fn is None and _same(plain, pe)
    xr = x.clone().requires_grad_(True)
    pose = mod(xr)
    assert pose.grad_fn is not None and _same(pose, pe)
    pose.backward(d)
    assert _same(xr.grad, ie)
    assert all(_same(p.grad, ge[k]) for k, p in mod.named_parameters())
    # two calls in one graph accumulate
    _, t2 = net.forward_train(x2)
    _, g2 = net.param_backward(x2, t2, d)
    mod.zero_grad(set_to_none=True)
    ((mod(x) * d).sum() + (mod(x2) * d).sum()).backward()
    for k, p in mod.named_parameters():
        assert _same(p.grad, ge[k] + g2[k]) or _same(p.grad, g2[k] + ge[k]), k
    # a frozen parameter takes none, the others keep their bits
    mod.zero_grad(set_to_none=True)
    mod.get_parameter("conv3.0.weight").requires_grad_(False)
    mod.get_parameter("conv1.1.bias").requires_grad_(False)
    (mod(x) * d).sum().backward()
    for k, p in mod.named_parameters():
        assert (p.grad is None) if k in ("conv3.0.weight", "conv1.1.bias") else _same(p.grad, ge[k]), k
    mod.requires_grad_(True)
    # a deep copy is independent
    twin = copy.deepcopy(mod)
    with torch.no_grad():
        twin.get_parameter("pose_pred.bias").add_(1.0)
        assert not _same(twin(x), pe) and _same(mod(x), pe)
    # an in-place update and a forward: the pose moves, and the older graph's backward is refused
    old = mod(x)
    with torch.no_grad():
        mod.get_parameter("conv2.0.weight").mul_(1.5).add_(0.01)
        assert _same(mod(x), pe) is False
    with pytest.raises(RuntimeError, match="changed in place"):
        old.backward(d)
    fresh = _net(H, W, N, {k: p.detach().cpu().numpy() for k, p in mod.named_parameters()})
    with torch.no_grad():
        assert _same(mod(x), fresh(x))


def test_bad_arguments_are_refused():
    from tightly_coupled_sfm_amd.posenet_train import PoseNetModule
    sd = PL.PARAM_SETS["base"](3)
    net = _net(17, 33, 2, sd)
    x = PL.images(17, 33, 2, seed=9).cuda()
    _, tape = net.forward_train(x)
    d = torch.zeros((2, 6)).cuda()
    with pytest.raises(AssertionError):
        net.param_backward(x, tape[:-4], d)
    with pytest.raises(KeyError):
        net.param_backward(x, tape, d, want=["conv8.0.weight"])
    with pytest.raises(ValueError):
        net.param_backward(None, tape, d, want=["conv1.0.weight"])
    with pytest.raises(AssertionError):
        net.param_backward(x[:, :, :-1], tape, d)
    with pytest.raises(KeyError):
        net.load_device({k: torch.as_tensor(v).cuda() for k, v in sd.items() if k != "conv5.0.weight"})
    with pytest.raises(AssertionError):
        net.load_device({k: torch.as_tensor(v).cuda()[..., :-1] if k == "conv2.0.weight" else torch.as_tensor(v).cuda() for k, v in sd.items()})
    with pytest.raises(ValueError):
        net.load_device({k: torch.as_tensor(v) for k, v in sd.items()})            # host tensors
    # the C entry point itself: conv1's weight gradient without the images, N beyond max_images
    import ctypes as C
    e = net.eng
    g1 = torch.empty((16, 6, 7, 7), device="cuda")
    tab = (C.c_void_p * 7)(g1.data_ptr(), *[None] * 6)
    assert net.lib.tcsfm_posenet_param_backward(net._pn, 2, None, e._p(tape), e._p(d), None, tab, None, None, None, None, None) != 0
    assert b"imgs is NULL" in net.lib.tcsfm_last_error(e._h)
    assert net.lib.tcsfm_posenet_param_backward(net._pn, 3, e._p(x), e._p(tape), e._p(d), None, tab, None, None, None, None, None) != 0
    assert net.lib.tcsfm_posenet_load_device(net._pn, None, None, None, None, None, None) != 0
    mod = PoseNetModule(sd).cuda()
    with pytest.raises(NotImplementedError):
        mod(x, return_features=True)
    with pytest.raises(ValueError):
        mod(x[:, :3])
    with pytest.raises(ValueError):
        PoseNetModule(sd)(x)            # parameters on the host
