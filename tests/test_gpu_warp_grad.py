"""The warp's backward pass on the GPU -- tcsfm_warp_backward, Engine.inverse_warp2_backward, stn.inverse_warp2 under autograd --
against autograd through the float64 twin (tests/warp_grad_inputs.py holds the cases, the tie mask, the cotangents and the judge;
tests/test_warp_grad_inputs_cpu.py checks them without a GPU).  Every tensor of every item is held to 4 x the float32 twin's own
error (relative L2 and max error over RMS), to a relative L2 below 1e-4, and to exact zeros where float64 is exactly zero.

MEASURED on an MI355X (TCSFM_TEST_WARP_GRAD_REPORT=<file> keeps one line per tensor and item, and one per case with the worst ratio):
per case the worst over items and over the four cotangent sets (all three, each alone).

    case                 d_depth_t        d_depth_s        d_pose           (worst ratio to the float32 twin | largest relative L2)
    5x9-N3-pose_x1       0.56 | 4.1e-08  0.10 | 6.0e-08  0.38 | 4.2e-08
    5x9-N3-pose_x30      1.00 | 3.6e-08  0.55 | 1.1e-06  0.78 | 3.7e-08
    17x33-N3-pose_x1     0.75 | 2.7e-08  0.05 | 1.7e-07  0.16 | 4.0e-08
    17x33-N3-pose_x30    0.64 | 3.9e-08  1.57 | 8.0e-06  0.51 | 4.0e-08
    37x53-N3-pose_x1     0.73 | 3.4e-08  0.06 | 3.5e-07  1.00 | 3.4e-08
    37x53-N3-pose_x30    0.78 | 3.2e-08  0.71 | 1.3e-05  0.15 | 4.3e-08
    100x333-N2-pose_x1   0.69 | 2.8e-08  0.03 | 9.6e-07  0.10 | 3.2e-08
    100x333-N2-pose_x30  0.69 | 3.0e-08  0.47 | 2.2e-05  0.13 | 4.0e-08
    192x640-N2-pose_x1   0.64 | 2.6e-08  0.07 | 3.2e-06  0.07 | 3.2e-08
    192x640-N2-pose_x30  0.58 | 2.6e-08  0.60 | 7.4e-05  0.06 | 4.3e-08
    37x53-N19-pose_x1    0.73 | 3.1e-08  0.12 | 3.6e-07  0.47 | 4.7e-08
    37x53-N19-pose_x30   0.88 | 4.3e-08  0.91 | 1.3e-05  0.96 | 5.5e-08

Every ratio is inside the margin of 4 and every relative L2 below 1e-4; no exact zero of float64 was missed.
"""
import ctypes as C
import os

import numpy as np
import pytest

import warp_grad_inputs as WG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_WARP_GRAD_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _engine_for(case):
    from tightly_coupled_sfm_amd.engine import Engine
    H, W, N, _ = case
    return Engine(H, W, WG.MANY_MAX_PAIRS if (H, W, N) == WG.MANY else N)


def _dev(case):
    c, cot = WG.make_case(*case), WG.cotangents(case)
    return {k: _t(v) for k, v in c.items()}, {k: _t(v) for k, v in cot.items()}


def _backward(e, d, cot, subset=WG.COTS, want=(True, True, True), items=slice(None)):
    """Engine.inverse_warp2_backward in the reference's convention (the warp is called with -pose; the gradient is returned with
    respect to +pose, as the twin's) -> dict of numpy arrays (None where not wanted)"""
    g = {k: (cot[k][items].contiguous() if k in subset else None) for k in WG.COTS}
    a, b, p = e.inverse_warp2_backward(d["src"][items].contiguous(), d["depth_t"][items].contiguous(), d["depth_s"][items].contiguous(),
                                       -d["pose"][items], d["K"][items].contiguous(), g["g_rec"], g["g_pd"], g["g_cd"], want)
    return dict(d_depth_t=None if a is None else _np(a), d_depth_s=None if b is None else _np(b), d_pose=None if p is None else -_np(p))


def _judge(case, subset, got, tag):
    ref, t32 = WG.twin(case, subset), WG.twin(case, subset, "f32")
    fails, worst = WG.judge(got, ref, t32, tag, _report)
    _report(f"{tag}\tworst ratio to the float32 twin\t" + "\t".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not fails, fails
    return ref


@pytest.mark.parametrize("case", WG.CASES, ids=WG.IDS)
def test_all_cotangents(case):
    d, cot = _dev(case)
    e = _engine_for(case)
    _judge(case, WG.COTS, _backward(e, d, cot), WG.IDS[WG.CASES.index(case)] + "/all")
    e.close()


@pytest.mark.parametrize("case", WG.CASES, ids=WG.IDS)
def test_each_cotangent_alone(case):
    """one cotangent, the other two NULL: judged as above; d_depth_s is exactly zero unless g_proj_depth is given; with g_comp_depth
    alone d_depth_t is exactly zero wherever the forward's comp_depth is 1e-3f and non-zero at the other out-of-frame pixels; with
    g_rec or g_proj_depth alone d_depth_t is exactly zero wherever the forward's valid is 0"""
    H, W, N, s = case
    d, cot = _dev(case)
    e = _engine_for(case)
    _, valid, _, cd = (_np(x) for x in e.inverse_warp2(d["src"], d["depth_t"], d["depth_s"], -d["pose"], d["K"]))
    clamped = cd == np.float32(1e-3)
    for k in WG.COTS:
        got = _backward(e, d, cot, (k,))
        _judge(case, (k,), got, WG.IDS[WG.CASES.index(case)] + "/" + k)
        if k != "g_pd":
            assert not got["d_depth_s"].any(), k
        if k == "g_cd":
            assert not got["d_depth_t"][clamped].any()
            live = (valid == 0) & ~clamped & (_np(cot["g_cd"]) != 0)
            assert (got["d_depth_t"][live] != 0).all()
            if s == 30.0:
                assert clamped.sum() > 0 and live.sum() > 0, (case, int(clamped.sum()), int(live.sum()))
        else:
            assert not got["d_depth_t"][valid == 0].any(), k
    e.close()


BIT_CASES = [(5, 9, 3, 30.0), (37, 53, 3, 1.0), (192, 640, 2, 30.0), WG.MANY + (1.0,), WG.MANY + (30.0,)]
BIT_IDS = [WG.IDS[WG.CASES.index(c)] for c in BIT_CASES]


@pytest.mark.parametrize("case", BIT_CASES, ids=BIT_IDS)
def test_bits_outputs_alone_repeat_and_items(case):
    """each output requested alone has the bits of the all-outputs call; two identical calls give identical bits; item n of a batch
    has the bits of a one-item call on item n (the 19-item call on the 24-pair engine included)"""
    H, W, N, s = case
    d, cot = _dev(case)
    e = _engine_for(case)
    full = _backward(e, d, cot)
    again = _backward(e, d, cot)
    for j, k in enumerate(WG.TENSORS):
        assert np.array_equal(_bits(full[k]), _bits(again[k])), ("repeat", k)
        want = tuple(i == j for i in range(3))
        alone = _backward(e, d, cot, want=want)
        assert all(alone[o] is None for o in WG.TENSORS if o != k)
        assert np.array_equal(_bits(alone[k]), _bits(full[k])), ("alone", k)
    for n in range(N):
        one = _backward(e, d, cot, items=slice(n, n + 1))
        for k in WG.TENSORS:
            assert np.array_equal(_bits(one[k][0]), _bits(full[k][n])), ("item", n, k)
    e.close()


def test_host_pointers_give_the_device_call_bits():
    """numpy arrays through the C ABI (opts.host_ptrs) at 17 x 33, with and without optional arguments"""
    from tightly_coupled_sfm_amd.engine import default_opts
    case = (17, 33, 3, 30.0)
    H, W, N, _ = case
    c, cot = WG.make_case(*case), WG.cotangents(case)
    d, dcot = _dev(case)
    e = _engine_for(case)
    def P(a):
        assert a is None or (a.flags.c_contiguous and a.dtype == np.float32)
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    o = default_opts(host_ptrs=1)
    for subset, want in ((WG.COTS, (True, True, True)), (("g_pd",), (False, True, True)), (("g_cd", "g_rec"), (True, False, False))):
        dev = _backward(e, d, dcot, subset, want)
        g = [cot[k] if k in subset else None for k in WG.COTS]
        outs = [np.full((N, 1, H, W), np.nan, np.float32) if want[0] else None, np.full((N, 1, H, W), np.nan, np.float32) if want[1] else None,
                np.full((N, 6), np.nan, np.float32) if want[2] else None]
        e._call(e.lib.tcsfm_warp_backward(e._h, C.byref(o), N, P(c["src"]), P(c["depth_t"]), P(c["depth_s"]), P(c["pose"]), P(c["K"]),
                                          P(g[0]), P(g[1]), P(g[2]), P(outs[0]), P(outs[1]), P(outs[2])))
        for k, got in zip(WG.TENSORS, outs):
            if got is not None:
                assert np.array_equal(_bits(got), _bits(dev[k])), (subset, k)       # (the ABI's pose argument is the case's pose)
    e.close()


def test_abi_refuses_what_the_forward_refuses():
    from tightly_coupled_sfm_amd.engine import default_opts
    case = (17, 33, 3, 1.0)
    d, cot = _dev(case)
    e = _engine_for(case)
    out = torch.empty_like(d["depth_t"])
    neg = (-d["pose"]).contiguous()
    call = lambda o, N, K: e.lib.tcsfm_warp_backward(e._h, C.byref(o), N, e._p(d["src"]), e._p(d["depth_t"]), e._p(d["depth_s"]), e._p(neg), e._p(K),
                                                     None, None, e._p(cot["g_cd"]), e._p(out), None, None)
    assert call(default_opts(), 3, d["K"]) == 0
    assert call(default_opts(depth_is_disp=1), 3, d["K"]) == -1           # TCSFM_E_ARG
    assert call(default_opts(), 4, d["K"]) == -1
    bad = d["K"].clone(); bad[1, 0, 1] = 0.5
    assert call(default_opts(), 3, bad) != 0                               # TCSFM_E_INTRINSICS
    e.close()


def test_autograd_drop_in():
    """stn.inverse_warp2 with requires_grad inputs: the forward's bits, a non-differentiable valid_mask, backward() of a random linear
    functional with the bits of Engine.inverse_warp2_backward; only-pose and only-depth; an eight-column pose; img.requires_grad"""
    from tightly_coupled_sfm_amd import stn
    from tightly_coupled_sfm_amd._shared import get_engine
    case = (37, 53, 3, 1.0)
    H, W, N, _ = case
    d, cot = _dev(case)
    pose = (-d["pose"]).contiguous()                                     # what a call site passes
    plain = stn.inverse_warp2(d["src"], d["depth_t"], d["depth_s"], pose, d["K"])
    assert all(not t.requires_grad and t.grad_fn is None for t in plain)
    direct = get_engine(H, W, N).inverse_warp2_backward(d["src"], d["depth_t"], d["depth_s"], pose, d["K"], cot["g_rec"], cot["g_pd"], cot["g_cd"])

    def run(req, pose_in=pose):
        leaves = [t.clone().requires_grad_(r) for t, r in zip((d["depth_t"], d["depth_s"], pose_in), req)]
        outs = stn.inverse_warp2(d["src"], leaves[0], leaves[1], leaves[2], d["K"])
        for a, b in zip(outs, plain):
            assert np.array_equal(_bits(_np(a)), _bits(_np(b)))
        assert not outs[1].requires_grad
        ((outs[0] * cot["g_rec"]).sum() + (outs[2] * cot["g_pd"]).sum() + (outs[3] * cot["g_cd"]).sum()).backward()
        return [l.grad for l in leaves]

    for req in ((True, True, True), (False, False, True), (True, False, False)):
        grads = run(req)
        for g, r, ref in zip(grads, req, direct):
            assert (g is None) == (not r)
            if r:
                assert np.array_equal(_bits(_np(g)), _bits(_np(ref))), req
    pose8 = torch.cat([pose, torch.full((N, 2), 7.0, device=pose.device)], 1)
    g8 = run((False, False, True), pose8)[2]
    assert g8.shape == (N, 8) and not _np(g8[:, 6:]).any() and np.array_equal(_bits(_np(g8[:, :6])), _bits(_np(direct[2])))
    # a cotangent autograd does not supply is passed as NULL: the bits of the one-cotangent call
    leaf = d["depth_s"].clone().requires_grad_()
    outs = stn.inverse_warp2(d["src"], d["depth_t"], leaf, pose, d["K"])
    (outs[2] * cot["g_pd"]).sum().backward()
    only = get_engine(H, W, N).inverse_warp2_backward(d["src"], d["depth_t"], d["depth_s"], pose, d["K"], None, cot["g_pd"], None, (False, True, False))
    assert np.array_equal(_bits(_np(leaf.grad)), _bits(_np(only[1])))
    with pytest.raises(NotImplementedError, match="DESIGN"):
        stn.inverse_warp2(d["src"].clone().requires_grad_(), d["depth_t"], d["depth_s"], pose, d["K"])
    with pytest.raises(NotImplementedError, match="DESIGN"):
        stn.inverse_warp2(d["src"], d["depth_t"], d["depth_s"], pose, d["K"].clone().requires_grad_())
