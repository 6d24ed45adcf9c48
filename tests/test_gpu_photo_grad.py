"""The photometric assembly's backward pass on the GPU -- tcsfm_photometric_maps_backward, tcsfm_photometric_backward, their Engine
wrappers and compute_photometric_error under autograd -- against autograd through the float64 twin (tests/photo_grad_inputs.py holds
the cases, the masks, the cotangents and the judge; tests/test_photo_grad_inputs_cpu.py checks them without a GPU).  Every tensor of
every item is held to 4 x the float32 twin's own error (relative L2 and max error over RMS) and to exact zeros where float64 is
exactly zero; the maps alone also to a relative L2 below 1e-4.

TCSFM_TEST_PHOTO_GRAD_REPORT=<file> keeps one line per tensor and item, and one per case with the worst ratio and the largest
relative L2 (the table of DESIGN.md section 4 is made from it).
"""
import ctypes as C
import os

import numpy as np
import pytest

import photo_grad_inputs as PG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
WG = PG.WG


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_PHOTO_GRAD_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _engine_for(case):
    from tightly_coupled_sfm_amd.engine import Engine
    H, W, N, _ = case
    return Engine(H, W, WG.MANY_MAX_PAIRS if (H, W, N) == WG.MANY else N)


def _id(case):
    return PG.IDS[PG.CASES.index(case)]


def _maps(e, l, cot, subset=PG.MAP_COTS, want=(True, True, True)):
    g = {k: (cot[k] if k in subset else None) for k in PG.MAP_COTS}
    out = e.photometric_maps_backward(l["tgt"], l["rec"], l["pd"], l["cd"], g["g_diff"], g["g_weight"], want)
    return dict(zip(PG.MAP_TENSORS, (_np(x) for x in out)))


def _chain(e, d, cot, subset=PG.CHAIN_COTS, want=(True, True, True)):
    g = {k: (cot[k] if k in subset else None) for k in PG.CHAIN_COTS}
    out = e.compute_photometric_error_backward(d["tgt"], d["src"], d["depth_t"], d["depth_s"], d["pose"], d["K"], g["g_diff"], g["g_weight"],
                                               g["g_img_rec"], want)
    return dict(zip(PG.CHAIN_TENSORS, (_np(x) for x in out)))


def _judge(got, ref, t32, tag, tensors, rel_l2_max):
    fails, worst = PG.judge(got, ref, t32, tag, tensors, _report, rel_l2_max)
    _report(f"{tag}\tworst ratio to the float32 twin | largest relative L2\t" + "\t".join(f"{k}={v[0]:.3f}|{v[1]:.2e}" for k, v in worst.items()))
    assert not fails, fails


@pytest.mark.parametrize("case", PG.CASES, ids=PG.IDS)
def test_maps_all_cotangents_and_each_alone(case):
    """the kernel alone on the shared float32 leaves; without g_diff g_rec is exactly zero, without g_weight g_pd and g_cd are"""
    l, cot = {k: _t(v) for k, v in PG.leaves(case).items()}, {k: _t(v) for k, v in PG.cotangents(case, "maps").items()}
    e = _engine_for(case)
    for subset in PG.MAP_SUBSETS:
        got = _maps(e, l, cot, subset)
        _judge(got, PG.twin_maps(case, subset), PG.twin_maps(case, subset, "f32"), f"{_id(case)}/maps/{'+'.join(subset)}", PG.MAP_TENSORS, PG.REL_L2_MAX)
        if "g_diff" not in subset:
            assert not got["g_rec"].any()
        if "g_weight" not in subset:
            assert not got["g_pd"].any() and not got["g_cd"].any()
    e.close()


@pytest.mark.parametrize("case", PG.CASES, ids=PG.IDS)
def test_chain_against_float64(case):
    """tcsfm_photometric_backward against autograd through torch_twin.photometric with respect to depth_t, depth_s and pose: all three
    cotangents together, and each alone at the sizes below 100 x 333 (the reference is computed on the CPU)"""
    H, W, N, _ = case
    d, cot = {k: _t(v) for k, v in PG.make_case(*case).items()}, {k: _t(v) for k, v in PG.cotangents(case, "chain").items()}
    e = _engine_for(case)
    for subset in (PG.CHAIN_SUBSETS if H * W < 30000 else PG.CHAIN_SUBSETS[:1]):
        got = _chain(e, d, cot, subset)
        _judge(got, PG.twin_chain(case, subset), PG.twin_chain(case, subset, "f32"), f"{_id(case)}/chain/{'+'.join(subset)}", PG.CHAIN_TENSORS, None)
    e.close()


BIT_CASES = [(5, 9, 3, 30.0), (37, 53, 3, 1.0), (192, 640, 2, 30.0), WG.MANY + (30.0,)]


@pytest.mark.parametrize("case", BIT_CASES, ids=[_id(c) for c in BIT_CASES])
def test_bits(case):
    """the same call twice gives the same bits (maps and chain); an output requested alone has the bits of the all-outputs call; item n
    of a batch has the bits of a one-item call; with only g_img_rec given the chain is tcsfm_warp_backward with g_rec, bit for bit"""
    H, W, N, _ = case
    d, cot = {k: _t(v) for k, v in PG.make_case(*case).items()}, {k: _t(v) for k, v in PG.cotangents(case, "chain").items()}
    l, mcot = {k: _t(v) for k, v in PG.leaves(case).items()}, {k: _t(v) for k, v in PG.cotangents(case, "maps").items()}
    e = _engine_for(case)
    m1, m2 = _maps(e, l, mcot), _maps(e, l, mcot)
    c1, c2 = _chain(e, d, cot), _chain(e, d, cot)
    for a, b, tensors in ((m1, m2, PG.MAP_TENSORS), (c1, c2, PG.CHAIN_TENSORS)):
        for k in tensors:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), ("repeat", k)
    for j in range(3):
        want = tuple(i == j for i in range(3))
        for full, alone, tensors in ((m1, _maps(e, l, mcot, want=want), PG.MAP_TENSORS), (c1, _chain(e, d, cot, want=want), PG.CHAIN_TENSORS)):
            assert all(alone[o] is None for i, o in enumerate(tensors) if i != j)
            assert np.array_equal(_bits(alone[tensors[j]]), _bits(full[tensors[j]])), ("alone", tensors[j])
    for n in (0, N - 1):
        one = _chain(e, {k: v[n:n + 1].contiguous() for k, v in d.items()}, {k: v[n:n + 1].contiguous() for k, v in cot.items()})
        for k in PG.CHAIN_TENSORS:
            assert np.array_equal(_bits(one[k][0]), _bits(c1[k][n])), ("item", n, k)
    only = _chain(e, d, cot, ("g_img_rec",))
    warp = e.inverse_warp2_backward(d["src"], d["depth_t"], d["depth_s"], -d["pose"], d["K"], cot["g_img_rec"], None, None)
    for k, w, sign in zip(PG.CHAIN_TENSORS, warp, (1, 1, -1)):        # (inverse_warp2_backward returns the gradient of ITS pose argument, -pose)
        assert np.array_equal(_bits(only[k]), _bits(sign * _np(w))), ("warp", k)
    e.close()


def test_host_pointers_and_refusals():
    """numpy arrays through the C ABI (opts.host_ptrs) give the device call's bits; depth_is_disp, a bad N and NULL inputs are refused"""
    from tightly_coupled_sfm_amd.engine import default_opts
    case = (17, 33, 3, 30.0)
    H, W, N, _ = case
    c, cot, l, mcot = PG.make_case(*case), PG.cotangents(case, "chain"), PG.leaves(case), PG.cotangents(case, "maps")
    d, dcot = {k: _t(v) for k, v in c.items()}, {k: _t(v) for k, v in cot.items()}
    e = _engine_for(case)
    P = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
    o = default_opts(host_ptrs=1)
    dev = _chain(e, d, dcot)
    outs = [np.full((N, 1, H, W), np.nan, np.float32), np.full((N, 1, H, W), np.nan, np.float32), np.full((N, 6), np.nan, np.float32)]
    ins = [np.ascontiguousarray(c[k], np.float32) for k in ("tgt", "src", "depth_t", "depth_s", "pose", "K")] + [cot[k] for k in PG.CHAIN_COTS]
    e._call(e.lib.tcsfm_photometric_backward(e._h, C.byref(o), N, *[P(a) for a in ins], *[P(a) for a in outs]))
    for k, got in zip(PG.CHAIN_TENSORS, outs):
        assert np.array_equal(_bits(got), _bits(dev[k])), k
    devm = _maps(e, {k: _t(v) for k, v in l.items()}, {k: _t(v) for k, v in mcot.items()}, ("g_diff",))
    outs = [np.full((N, 3, H, W), np.nan, np.float32), np.full((N, 1, H, W), np.nan, np.float32), None]
    e._call(e.lib.tcsfm_photometric_maps_backward(e._h, C.byref(o), N, P(l["tgt"]), P(l["rec"]), P(l["pd"]), P(l["cd"]), P(mcot["g_diff"]), None,
                                                  P(outs[0]), P(outs[1]), None))
    assert np.array_equal(_bits(outs[0]), _bits(devm["g_rec"])) and not outs[1].any()
    out = torch.empty_like(d["depth_t"])
    call = lambda o, n, tgt: e.lib.tcsfm_photometric_backward(e._h, C.byref(o), n, e._p(tgt), e._p(d["src"]), e._p(d["depth_t"]), e._p(d["depth_s"]),
                                                             e._p(d["pose"]), e._p(d["K"]), e._p(dcot["g_diff"]), None, None, e._p(out), None, None)
    assert call(default_opts(), N, d["tgt"]) == 0
    assert call(default_opts(depth_is_disp=1), N, d["tgt"]) == -1          # TCSFM_E_ARG
    assert call(default_opts(), N + 1, d["tgt"]) == -1
    assert call(default_opts(), N, None) == -1
    e.close()


def test_autograd_drop_in():
    """helpers.compute_photometric_error with leaves that require grad: the plain call's bits forward, masks without grad, backward()
    with the bits of the Engine call; only the pose; an absent cotangent is passed as NULL; an image that requires grad raises"""
    from tightly_coupled_sfm_amd import helpers
    from tightly_coupled_sfm_amd._shared import get_engine
    case = (37, 53, 3, 1.0)
    H, W, N, _ = case
    d, cot = {k: _t(v) for k, v in PG.make_case(*case).items()}, {k: _t(v) for k, v in PG.cotangents(case, "chain").items()}
    args = lambda dt, ds, p: (d["tgt"], d["src"], dt, ds, p, d["K"])
    plain = helpers.compute_photometric_error(*args(d["depth_t"], d["depth_s"], d["pose"]))
    assert all(not t.requires_grad and t.grad_fn is None for t in plain.values())
    with torch.no_grad():
        quiet = helpers.compute_photometric_error(*args(d["depth_t"].clone().requires_grad_(), d["depth_s"], d["pose"]))
    assert all(t.grad_fn is None for t in quiet.values())
    direct = get_engine(H, W, N).compute_photometric_error_backward(*args(d["depth_t"], d["depth_s"], d["pose"]), cot["g_diff"], cot["g_weight"], cot["g_img_rec"])
    for req in ((True, True, True), (False, False, True), (True, False, False)):
        leaves = [t.clone().requires_grad_(r) for t, r in zip((d["depth_t"], d["depth_s"], d["pose"]), req)]
        r = helpers.compute_photometric_error(*args(*leaves))
        for k in ("diff_img", "img_rec", "valid_mask", "weight_mask"):
            assert np.array_equal(_bits(_np(r[k])), _bits(_np(plain[k]))), k
        assert not r["valid_mask"].requires_grad and all(r[k].grad_fn is not None for k in ("diff_img", "img_rec", "weight_mask"))
        ((r["diff_img"] * cot["g_diff"]).sum() + (r["weight_mask"] * cot["g_weight"]).sum() + (r["img_rec"] * cot["g_img_rec"]).sum()).backward()
        for leaf, rq, ref in zip(leaves, req, direct):
            assert (leaf.grad is None) == (not rq)
            if rq:
                assert np.array_equal(_bits(_np(leaf.grad)), _bits(_np(ref))), req
    full = get_engine(H, W, N).compute_photometric_error(*args(d["depth_t"].clone().requires_grad_(), d["depth_s"], d["pose"]))
    assert not any(full[k].requires_grad for k in ("valid_mask", "warp_valid", "auto_mask", "auto_mask_error"))
    leaf = d["depth_s"].clone().requires_grad_()
    r = helpers.compute_photometric_error(*args(d["depth_t"], leaf, d["pose"]))
    (r["weight_mask"] * cot["g_weight"]).sum().backward()
    only = get_engine(H, W, N).compute_photometric_error_backward(*args(d["depth_t"], d["depth_s"], d["pose"]), None, cot["g_weight"], None, (False, True, False))
    assert np.array_equal(_bits(_np(leaf.grad)), _bits(_np(only[1])))
    with pytest.raises(NotImplementedError, match="DESIGN"):
        helpers.compute_photometric_error(d["tgt"].clone().requires_grad_(), d["src"], d["depth_t"], d["depth_s"], d["pose"], d["K"])
    with pytest.raises(NotImplementedError, match="DESIGN"):
        helpers.compute_photometric_error(d["tgt"], d["src"], d["depth_t"].clone().requires_grad_(), d["depth_s"], d["pose"], d["K"].clone().requires_grad_())


def test_end_to_end_scalar_loss():
    """17 x 33: L = (diff mask weight).sum() / mask.sum() + 0.1 (1 - weight).mean() with the library's mask, detached, in the library
    and in the twins; gradients with respect to the depths and the pose against float64, the float32 twin's error times 4 as bound.
    (No pixel is masked here: the scalar's cotangents are what they are.  The bound is asserted for the whole tensors.)"""
    from tightly_coupled_sfm_amd import helpers
    for s in (1.0,):                # (at poses x30 no pixel of this size survives the auto-mask: the scalar would be 0 / 0)
        case = (17, 33, 3, s)
        d = {k: _t(v) for k, v in PG.make_case(*case).items()}
        leaves = [d[k].clone().requires_grad_() for k in ("depth_t", "depth_s", "pose")]
        r = helpers.compute_photometric_error(d["tgt"], d["src"], leaves[0], leaves[1], leaves[2], d["K"])
        mask = r["valid_mask"].detach()
        assert float(mask.sum()) > 0
        L = (r["diff_img"] * mask * r["weight_mask"]).sum() / mask.sum() + 0.1 * (1 - r["weight_mask"]).mean()
        L.backward()
        got = dict(zip(PG.CHAIN_TENSORS, (_np(l.grad) for l in leaves)))
        m = _np(mask)
        ref, t32 = PG.chain_gradient(case, None, "f64", m), PG.chain_gradient(case, None, "f32", m)
        _judge(got, ref, t32, f"{_id(case)}/end_to_end", PG.CHAIN_TENSORS, None)
