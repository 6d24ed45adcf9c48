"""GPU: the reference's test-time weight tuning end to end -- network weights -> DepthNetModule -> slices ->
learning_helpers.disp_to_depth -> helpers.compute_photometric_error (forward and inverse pairs) -> losses.compute_optimization_loss ->
backward() -- the composition the differentiable stages exist for (tests/tuning_chain_inputs.py holds the inputs, the float64 twin
and the judges; tests/test_tuning_chain_inputs_cpu.py checks them without a GPU).  B = 1, S = 2, three images at 32 x 64 and
96 x 160.  Poses and intrinsics are constants: the library has no PoseNet backward, so solve_pose_iteratively's dependence on the
depths is not imitated.

What only the composition can get wrong: the network owns its Engine (depthnet_train._Native.eng) while the loss side runs on the
shared engines of _shared.get_engine, which are replaced by a larger one mid-graph; both follow torch's current stream; the target's
disparity fans out into four consumers whose contributions autograd sums; the cotangent that reaches the network is the output of
slice and repeat backward nodes, zero where the masks are zero and with the 1 / Z^2 range of the warp; the stamp check runs with the
other autograd Functions in the graph.

1. COMPOSITION IS EXACT (bitwise): the cotangent the network receives is the gradient of a disparity leaf put through the same chain;
   the network's gradients are those of the network alone under that cotangent; a second run, a run on a side stream and the run
   during which the shared engine is created and replaced all give the same bits.  With separate target and source leaves both
   sides are compared after x + 0.0: a gradient of -0.0 at a leaf becomes +0.0 where autograd adds the padded slices, no other bit moves.
2. TUNING MODES of the reference: encoder only, decoder with fixed skips (the bits of the full run), bottleneck values (skips 3 and
   4 as leaves, against float64 autograd of the decoder under the float64 twin's cotangent).
3. THE LOSS SIDE at network-made disparities against the float64 twin, by the project's ratio to the float32 twin (32 x 64: see the
   inputs module on why not 96 x 160).
4. THE NETWORK'S BACKWARD under the chain's own cotangent against float64 autograd through depthnet_twin.forward_pinned, held to the
   bounds of test_gpu_depthnet_grad_exact.py (measured there with dense random cotangents).
5. THE LOOP MOVES: three Adam epochs at the reference's learning rate on a deep copy.

Measured on an MI355X (worst value; bound) -- TCSFM_TEST_TUNING_CHAIN_REPORT=<file> keeps one line per tensor:
  3. loss side, 32 x 64, worst ratio to the float32 twin | largest relative L2 ... d_disp_t 0.040 | 1.3e-7, d_disp_s 0.029 | 1.7e-7; bound 4
     the loss .................................................................. 0.2644348145 against 0.2644348247 in float64; 1e-3
     at the library's disparities: no cell or validity flip, nearest boundary 2.6e-4 px = 17 x the coordinate difference
     96 x 160, the loss only ................................................... 0.2405333221 against 0.2405333283 in float64; 1e-3
     (reported, not judged, there: the library's relative L2 is 1.9e-7 .. 3.3e-7 while the float32 twin's own is 2.0e-3 on two of the
     three tensors -- with 0.22 x headroom the yardstick itself takes other discrete decisions than float64)
  4. encoder (60 tensors), relative L2 ......... 3.6e-6 at 32 x 64, 6.5e-6 at 96 x 160 (layer 4); 1e-4
     encoder, max error / RMS .................. 1.7e-4 at 32 x 64, 1.1e-4 at 96 x 160; 2e-3
     decoder parameters, relative L2 ........... 2.5e-6 at 32 x 64, 3.5e-6 at 96 x 160 (depth_upconvs.0.1.conv.weight); 5e-5
     decoder parameters, max error / RMS ....... 3.4e-5 at both shapes; 5e-4
     forward_pinned evaluated in float32 on the same tape and cotangent (the yardstick a bound would have come from; none was
     needed): encoder 3.9e-6 | 1.6e-4 at 32 x 64 and 5.0e-6 | 7.9e-5 at 96 x 160, decoder 3.0e-6 | 5.0e-5 and 3.1e-6 | 3.0e-5
  2. bottleneck values, skips 3 and 4 ........... relative L2 1.7e-6, max error / RMS 1.0e-5 (skip 3); 4e-5, 5e-4
  5. losses of the three epochs and after them .. 0.26079, 0.26573, 0.26117, 0.25750
  1. every bitwise comparison holds, 1(b) included (after x + 0.0, see above)
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depthnet_twin as dt  # noqa: E402
import test_gpu_depthnet_grad_exact as X  # noqa: E402
import tuning_chain_inputs as TC  # noqa: E402

LG = TC.LG
SMALL = TC.SHAPES[0]
LR = 2e-4                                   # the reference's options['lr'] for this loop (run_sequential_optimization.py:95)
OPTION_SETS = dict(e2e=TC.OPTIONS, reference=TC.OPTIONS_DEFAULT)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """bit for bit"""
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_TUNING_CHAIN_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _key(shape):
    return (torch.cuda.current_device(), *shape)


@functools.lru_cache(maxsize=None)
def _consts(shape):
    im, pose, K = _t(TC.images(shape)), _t(TC.poses(shape)), _t(TC.intrinsics(shape))
    return dict(imgs=im, tgt=im[:1].contiguous(), src=im[1:].contiguous(), tgt2=im[:1].repeat(2, 1, 1, 1), pose=pose, K=K)


@functools.lru_cache(maxsize=None)
def _orig(shape):
    """the module every run deep-copies; never run under grad itself"""
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    return DepthNetModule(dt.depthnet_params(TC.SEED[shape]), max_images=TC.N_IMAGES).cuda()


@functools.lru_cache(maxsize=None)
def _first_pass(shape):
    """the module's own first pass (optimizer.py:143-154): the skips, the target disparity detached, and that disparity perturbed as
    loss_grad_inputs.e2e_inputs does (the depth-init term then has a gradient)"""
    with torch.no_grad():
        disps, skips = _orig(shape)(x=_consts(shape)["imgs"])
    init = disps[0][0:1].detach().clone()
    return dict(skips=[s.detach().clone() for s in skips], init=init, perturbed=_t(TC.perturbed(_np(init))))


def _loss_side(shape, disps, disp_init, options, trace=None):
    """steps 3 to 7 of the chain from the three disparities [1,1,H,W] (target, source 1, source 2) -> (loss, fwd, inv).  With
    automasking the dicts carry what train_mono.solve_pose_iteratively emits beyond helpers.compute_photometric_error's keys (the
    warp validity as valid_mask, auto_mask_error, auto_mask), from a plain call on the shared engine: masks take no gradient.
    `trace`: gets the shared engine after the first disp_to_depth and after the first compute_photometric_error."""
    from tightly_coupled_sfm_amd import _shared, helpers, learning_helpers, losses
    c = _consts(shape)
    depths = []
    for d in disps:
        depths.append(learning_helpers.disp_to_depth(d, *TC.DEPTH_RANGE)[1])
        if trace is not None and not trace:
            trace.append(_shared._engines.get(_key(shape)))
    dt2, ds = depths[0].repeat(2, 1, 1, 1), torch.cat(depths[1:], 0)
    fwd = helpers.compute_photometric_error(c["tgt2"], c["src"], dt2, ds, c["pose"], c["K"])
    if trace is not None:
        trace.append(_shared._engines.get(_key(shape)))
    inv = helpers.compute_photometric_error(c["src"], c["tgt2"], ds, dt2, -c["pose"], c["K"])
    if options["automasking"]:
        e = _shared.get_engine(*shape, 2)
        with torch.no_grad():
            mf = e.compute_photometric_error(c["tgt2"], c["src"], dt2.detach(), ds.detach(), c["pose"], c["K"])
            mi = e.compute_photometric_error(c["src"], c["tgt2"], ds.detach(), dt2.detach(), -c["pose"], c["K"])
        fwd, inv = (dict(r, valid_mask=m["warp_valid"], auto_mask_error=m["auto_mask_error"], auto_mask=m["auto_mask"])
                    for r, m in ((fwd, mf), (inv, mi)))
    L = losses.compute_optimization_loss(options, c["tgt"], disps[0], disp_init, fwd, inv, losses.SSIM_Loss())
    return L, fwd, inv


def _slices(disp):
    """optimizer.py:232-234 with B = 1"""
    return [disp[0:1], disp[1:2], disp[2:3]]


def _chain(shape, options, mod, disp_init, skips=None, trace=None):
    """the whole chain from the module -> (loss, the network's disparity with its gradient retained, fwd, inv)"""
    disps, _ = mod(x=_consts(shape)["imgs"]) if skips is None else mod(x=None, skips=skips)
    disp = disps[0]
    if disp.requires_grad:
        disp.retain_grad()
    L, fwd, inv = _loss_side(shape, _slices(disp), disp_init, options, trace)
    return L, disp, fwd, inv


def _grads(mod):
    return {k: p.grad.detach().clone() for k, p in mod.named_parameters() if p.grad is not None}


def _run_full(shape, opt, trace=None):
    """one full run on a fresh deep copy, every parameter requiring grad -> dict: G (a gradient per parameter), g_disp (the cotangent the
    network received), disp, loss, fwd_valid, inv_valid"""
    mod = copy.deepcopy(_orig(shape))
    L, disp, fwd, inv = _chain(shape, OPTION_SETS[opt], mod, _first_pass(shape)["perturbed"], trace=trace)
    L.backward()
    G = _grads(mod)
    assert sorted(G) == sorted(k for k, _ in mod.named_parameters()) and disp.grad is not None
    return dict(G=G, g_disp=disp.grad.detach().clone(), disp=disp.detach().clone(), loss=L.detach().clone(),
                fwd_valid=fwd["valid_mask"].detach().clone(), inv_valid=inv["valid_mask"].detach().clone())


@functools.lru_cache(maxsize=None)
def _full(shape, opt):
    """computed once per (shape, option set) and shared: read-only"""
    return _run_full(shape, opt)


def _assert_same_run(a, b, what):
    assert _same(a["loss"], b["loss"]), (what, "loss", float(a["loss"]), float(b["loss"]))
    assert _same(a["g_disp"], b["g_disp"]), (what, "g_disp")
    assert sorted(a["G"]) == sorted(b["G"])
    diff = [k for k in a["G"] if not _same(a["G"][k], b["G"][k])]
    assert not diff, (what, diff)


@functools.lru_cache(maxsize=None)
def _twin(shape):
    """the float64 and the float32 twin of the loss side at the library's own disparities and masks (E2E options) -> dict: ref, t32
    (d_disp_t, d_disp_s), L64, conditions (tuning_chain_inputs.conditions at the library's disparities)"""
    full, fp = _full(shape, "e2e"), _first_pass(shape)
    disp = _np(full["disp"])
    inp = TC.chain_inputs(shape, disp, disp_init=_np(fp["perturbed"]))
    masks = dict(fwd_valid=_np(full["fwd_valid"]), inv_valid=_np(full["inv_valid"]))
    (ref, L64), (t32, _) = (LG.e2e_twin(masks, d, inp, TC.OPTIONS, TC.DEPTH_RANGE) for d in ("f64", "f32"))
    return dict(ref=ref, t32=t32, L64=L64, conditions=TC.conditions(shape, disp), masks=masks)


# ---- 1. composition is exact ---------------------------------------------------------------------------------------------------

def test_engine_replacement_mid_graph():
    """1(f): the run is the first use of its frame size: the chain's first disp_to_depth creates the shared engine (one pair),
    compute_photometric_error replaces it by a larger one while _DispToDepth's nodes still hold the first; the backward then runs on
    both.  The result has the bits of a later run on the settled engine."""
    from tightly_coupled_sfm_amd import _shared
    _shared._engines.pop(_key(SMALL), None)            # (whatever ran before: this run creates the engine)
    trace = []
    first = _run_full(SMALL, "e2e", trace)
    created, replaced = trace
    assert created is not None and created.max_pairs == 1, "disp_to_depth did not create a one-pair engine"
    assert replaced is not created and replaced.max_pairs >= 2, "compute_photometric_error did not replace the engine"
    assert _shared._engines[_key(SMALL)] is replaced
    later = _run_full(SMALL, "e2e")
    assert _shared._engines[_key(SMALL)] is replaced, "the settled engine was replaced again"
    _assert_same_run(first, later, "engine replaced mid-graph")
    _assert_same_run(first, _full(SMALL, "e2e"), "engine replaced mid-graph, shared run")


@pytest.mark.parametrize("opt", list(OPTION_SETS))
@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.IDS)
def test_composition_is_exact(shape, opt):
    """1(a) to 1(d)"""
    full, options, init = _full(shape, opt), OPTION_SETS[opt], _first_pass(shape)["perturbed"]
    # (a) one disparity leaf, sliced the same way
    leaf = full["disp"].clone().requires_grad_()
    L = _loss_side(shape, _slices(leaf), init, options)[0]
    L.backward()
    assert _same(L, full["loss"]) and _same(leaf.grad, full["g_disp"]), "leaf path"
    # (b) separate target and source leaves.  The target's three direct consumers (disp_to_depth, SSIM_Loss, get_smooth_loss) send
    # their gradients in the same order to the leaf's accumulator as to the slice node's input buffer, so the sums are the same;
    # only a -0.0 of a leaf turns into +0.0 where the padded slices are added: x + 0.0 does the same to both sides and changes no
    # other bit
    leaves = [full["disp"][n:n + 1].clone().requires_grad_() for n in range(TC.N_IMAGES)]
    L = _loss_side(shape, leaves, init, options)[0]
    L.backward()
    assert _same(L, full["loss"]) and _same(torch.cat([l.grad for l in leaves], 0) + 0.0, full["g_disp"] + 0.0), "separate leaves"
    # (c) the network alone under that cotangent
    mod = copy.deepcopy(_orig(shape))
    (mod(_consts(shape)["imgs"])[0][0] * full["g_disp"]).sum().backward()
    G = _grads(mod)
    diff = [k for k in full["G"] if not _same(G[k], full["G"][k])]
    assert not diff, ("network alone", diff)
    # (d) a second full run
    _assert_same_run(_run_full(shape, opt), full, "repeat")
    assert bool(torch.isfinite(full["g_disp"]).all()) and all(bool(full["g_disp"][n].any()) for n in range(TC.N_IMAGES))


def test_side_stream():
    """1(e): the whole chain, forward and backward, inside `with torch.cuda.stream(side)`: the network's engine and the shared one
    both follow it"""
    full = _full(SMALL, "e2e")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run_full(SMALL, "e2e")
    torch.cuda.current_stream().wait_stream(side)
    _assert_same_run(got, full, "side stream")


# ---- 2. the reference's tuning modes -------------------------------------------------------------------------------------------

def test_mode_optimize_depth_encoder():
    full = _full(SMALL, "e2e")
    mod = copy.deepcopy(_orig(SMALL))
    for p in mod.parameters():
        p.requires_grad_(False)
    for p in mod.encoder.parameters():
        p.requires_grad_(True)
    L, disp, _, _ = _chain(SMALL, TC.OPTIONS, mod, _first_pass(SMALL)["perturbed"])
    L.backward()
    G = _grads(mod)
    assert sorted(G) == sorted(k for k in full["G"] if k.startswith(dt.ENC)) and len(G) == 60
    diff = [k for k in G if not _same(G[k], full["G"][k])]
    assert not diff and _same(L, full["loss"]) and _same(disp.grad, full["g_disp"]), diff


def test_mode_optimize_depth_weights_bottleneck_beyond():
    full, fp = _full(SMALL, "e2e"), _first_pass(SMALL)
    mod = copy.deepcopy(_orig(SMALL))
    L, disp, _, _ = _chain(SMALL, TC.OPTIONS, mod, fp["perturbed"], skips=[s.clone() for s in fp["skips"]])
    L.backward()
    G = _grads(mod)
    assert sorted(G) == sorted(k for k in full["G"] if not k.startswith(dt.ENC)) and G
    diff = [k for k in G if not _same(G[k], full["G"][k])]
    assert not diff and _same(L, full["loss"]) and _same(disp.grad, full["g_disp"]), diff


def test_mode_optimize_depth_bottleneck_values():
    """skips 3 and 4 as leaves, the parameters frozen: their gradients against float64 autograd of depthnet_twin._decode on the same
    skip values under the float64 twin's disparity cotangent (test 3's), bounds SKIP_REL / SKIP_ELEM"""
    full, fp, tw = _full(SMALL, "e2e"), _first_pass(SMALL), _twin(SMALL)
    mod = copy.deepcopy(_orig(SMALL))
    for p in mod.parameters():
        p.requires_grad_(False)
    leaves = [s.clone().requires_grad_(k >= 3) for k, s in enumerate(fp["skips"])]
    L, disp, _, _ = _chain(SMALL, TC.OPTIONS, mod, fp["perturbed"], skips=leaves)
    L.backward()
    assert _same(disp, full["disp"]) and _same(disp.grad, full["g_disp"]), "the decoder on the first pass's skips is not the full forward: test 3's twin does not apply"
    assert all(l.grad is None for l in leaves[:3]) and all(p.grad is None for p in mod.parameters())
    sd = X._ref_params(TC.SEED[SMALL], lambda k: False)
    ref_leaves = [s.detach().double().requires_grad_(k >= 3) for k, s in enumerate(fp["skips"])]
    (dt._decode(sd, ref_leaves) * torch.from_numpy(TC.join(tw["ref"])).cuda()).sum().backward()
    errs = {f"skip{k}": X._errs(leaves[k].grad, ref_leaves[k].grad) for k in (3, 4)}
    for k, e in errs.items():
        _report(f"32x64/bottleneck_values\t{k}\trel_l2={e[0]:.3e}\tmax/rms={e[1]:.3e}")
    bad = X._over(errs, X.SKIP_REL, X.SKIP_ELEM)
    assert not bad, bad


# ---- 3. the loss side at network-made disparities ------------------------------------------------------------------------------

def test_loss_side_against_float64():
    shape = TC.ACCURACY_SHAPE
    full, tw = _full(shape, "e2e"), _twin(shape)
    c = tw["conditions"]
    _report(f"{shape[0]}x{shape[1]}/loss_side\tinputs at the library's disparities\t" + "\t".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in c.items()))
    bad = TC.conditions_hold(c, headroom=False)
    assert not bad, ("bad input: at the library's own disparities", bad)
    assert tw["masks"]["fwd_valid"].sum() > 0 and tw["masks"]["inv_valid"].sum() > 0
    L = float(full["loss"])
    tag = f"{shape[0]}x{shape[1]}/loss_side"
    _report(f"{tag}\tloss={L:.9e}\tfloat64 twin={tw['L64']:.9e}")
    assert abs(L - tw["L64"]) < 1e-3 * abs(tw["L64"])          # (the bound of test_gpu_loss_grad.py::test_end_to_end_optimization_loss)
    fails, worst = TC.loss_judge(TC.split(_np(full["g_disp"])), tw["ref"], tw["t32"], tag, _report)
    _report(f"{tag}\tworst ratio to the float32 twin | largest relative L2\t" + "\t".join(f"{k}={v[0]:.3f}|{v[1]:.2e}" for k, v in worst.items()))
    assert not fails, fails


def test_loss_value_against_float64_at_the_larger_shape():
    """96 x 160 has no headroom for the gradient comparison (tests/tuning_chain_inputs.py), but the loss itself is continuous across
    a cell border: the same 1e-3 bound; the gradient's figures are reported, not judged"""
    shape = TC.SHAPES[1]
    full, tw = _full(shape, "e2e"), _twin(shape)
    L, tag = float(full["loss"]), f"{shape[0]}x{shape[1]}/loss_side"
    _report(f"{tag}\tloss={L:.9e}\tfloat64 twin={tw['L64']:.9e}\tflips at the library's disparities={tw['conditions']['flips']}\tmargin_ratio={tw['conditions']['margin_ratio']:.3f}")
    TC.loss_judge(TC.split(_np(full["g_disp"])), tw["ref"], tw["t32"], tag + " (not judged)", _report)
    assert tw["masks"]["fwd_valid"].sum() > 0 and tw["masks"]["inv_valid"].sum() > 0
    assert abs(L - tw["L64"]) < 1e-3 * abs(tw["L64"])


# ---- 4. the network's backward under the chain's cotangent ---------------------------------------------------------------------

@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.IDS)
def test_network_backward_under_the_chain_cotangent(shape):
    """G_full against float64 autograd through forward_pinned on the module's own tape, cotangent g_disp (exact in float64); the
    same pinned network evaluated in float32 is reported next to it (the yardstick a bound would come from, were one needed)"""
    full, imgs = _full(shape, "e2e"), _consts(shape)["imgs"]
    entries = X.tape_entries(copy.deepcopy(_orig(shape)), imgs)
    grads = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        sd = {k: v.to(dtype) for k, v in X._ref_params(TC.SEED[shape], lambda k: False).items()}
        for k in full["G"]:
            sd[k].requires_grad_(True)
        disp, _ = dt.forward_pinned(sd, imgs.to(dtype), entries)
        if name == "f64":
            assert float((disp.detach() - full["disp"].double()).abs().max()) < 1e-4, "the pinned float64 forward is not the module's forward"
        (disp * full["g_disp"].to(dtype)).sum().backward()
        grads[name] = {k: sd[k].grad for k in full["G"]}
    tag = f"{shape[0]}x{shape[1]}/network_backward"
    _, w32 = TC.param_judge(grads["f32"], grads["f64"], _report, tag + "/float32 pinned twin")
    bad, worst = TC.param_judge(full["G"], grads["f64"], _report, tag)
    for cls in worst:
        _report(f"{tag}\t{cls}\tworst rel_l2={worst[cls][0]:.3e} (float32 pinned twin {w32[cls][0]:.3e})\tworst max/rms={worst[cls][1]:.3e} (float32 pinned twin {w32[cls][1]:.3e})")
    assert len([k for k in full["G"] if k.startswith(dt.ENC)]) == 60
    assert not bad, bad


# ---- 5. the loop moves ---------------------------------------------------------------------------------------------------------

def test_the_loop_moves():
    """deep copy, the copy's encoder parameters in Adam at the reference's learning rate, three epochs of the chain (disp_init: the
    first pass's target disparity as optimizer.py:154 takes it): the loss after the third step is below the first, every epoch's
    forward differs from the one before (the re-fold ran), the original is untouched, and a backward after an in-place update and
    another forward is refused with the loss-side Functions in the graph"""
    orig, imgs, init = _orig(SMALL), _consts(SMALL)["imgs"], _first_pass(SMALL)["init"]
    before = {k: v.clone() for k, v in orig.state_dict().items()}
    cp = copy.deepcopy(orig)
    opt = torch.optim.Adam(cp.encoder.parameters(), lr=LR)
    losses, prev = [], None
    for epoch in range(3):
        opt.zero_grad()
        L, disp, _, _ = _chain(SMALL, TC.OPTIONS, cp, init)
        assert prev is None or not torch.equal(disp.detach(), prev), f"epoch {epoch}: the forward did not change"
        prev = disp.detach().clone()
        L.backward()
        opt.step()
        losses.append(float(L.detach()))
    L, disp, _, _ = _chain(SMALL, TC.OPTIONS, cp, init)
    losses.append(float(L.detach()))
    _report("32x64/loop\tlosses\t" + "\t".join(f"{v:.9e}" for v in losses))
    assert not torch.equal(disp.detach(), prev) and losses[3] < losses[0], losses
    for k, v in orig.state_dict().items():
        assert _same(v, before[k]), k
    assert any(not torch.equal(v, before[k]) for k, v in cp.state_dict().items() if k.startswith(dt.ENC))
    opt.step()                                               # an in-place update (the last epoch's gradients) ...
    cp(x=imgs)                                               # ... and another forward re-folds the new weights
    with pytest.raises(RuntimeError, match="changed in place"):
        L.backward()
