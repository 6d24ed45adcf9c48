"""The window loss of optimizer.py:47-86 on the GPU -- tcsfm_window_loss, tcsfm_window_loss_backward, their Engine wrappers and
losses.compute_optimization_loss(fused=True) -- against losses.compute_optimization_loss on the CPU in float64 under autograd
(tests/window_loss_inputs.py holds the cases, the reference and the closed forms; tests/test_window_loss_inputs_cpu.py checks them without
a GPU).

Bounds.  The library evaluates every product and sum in double and rounds once, so the scalar and every gradient entry are held to ONE
float32 rounding of the float64 value, |x - x64| <= 2^-23 |x64|: the double summation error n 2^-53 <= 1e-10 and the few double
operations of a gradient entry are far below half a float32 ulp, and at the handful of weight-gradient pixels where q - w / n nearly
cancels (down to ~2^-18 of the terms among 245 760 pixels) the double error is still 2^-52 x 2^18 = 2^-34 of the entry.  Each sum of
`stats` is within 1e-9 relative of numpy's float64 sum.  Where the closed form is exactly zero the output is exactly zero.
The depth-consistency weight is float32(0.15) on both sides: tcsfm_opts.w_dc is a float (tests/window_loss_inputs.W_DC)."""
import numpy as np
import pytest

import loss_grad_inputs as LG
import window_loss_inputs as WL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
IDS = ["x".join(map(str, c)) for c in WL.CASES]


def _t(a):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _sw(case, combo):
    return dict(S=case[3], argmin=combo[0], automasking=combo[1], inverse=combo[2], w_dc=combo[3])


@pytest.fixture(scope="module")
def dev():
    """{case: ({key: device tensor}, Engine)}, made on first use"""
    from tightly_coupled_sfm_amd.engine import Engine
    made = {}

    def get(case):
        if case not in made:
            H, W, B, S = case
            made[case] = ({k: _t(v) for k, v in WL.inputs(case).items()}, Engine(H, W, S * B))
        return made[case]
    yield get
    for _, e in made.values():
        e.close()


def _maps(t):
    return [t[k] for k in WL.KEYS]


@pytest.mark.parametrize("case", WL.CASES, ids=IDS)
def test_forward(dev, case):
    t, e = dev(case)
    for combo in WL.COMBOS:
        loss, stats = e.window_loss(*_maps(t), **_sw(case, combo))
        assert loss.shape == () and loss.dtype == torch.float32 and stats.shape == (7,) and stats.dtype == torch.float64
        L64 = float(WL.reference64(case, combo)[0].reshape(-1)[0])
        _, s64, _, _, _ = WL.closed_forms(case, combo)
        L, s = float(loss), _np(stats)
        print(f"{case} {combo}: loss {L:.9e} float64 {L64:.9e} rel {abs(L - L64) / abs(L64):.2e}; stats rel {np.max(np.abs(s - s64) / np.maximum(np.abs(s64), 1e-300)):.2e}")
        assert abs(L - L64) <= EPS * abs(L64), (case, combo, L, L64)
        assert np.all(np.abs(s - s64) <= 1e-9 * np.abs(s64)), (case, combo, s, s64)
        if not combo[2]:
            assert s[2] == 0 and s[3] == 0 and s[5] == 0


@pytest.mark.parametrize("case", WL.CASES, ids=IDS)
def test_backward(dev, case):
    H, W, B, S = case
    t, e = dev(case)
    one, g17 = torch.tensor(1.0, device="cuda"), torch.tensor(1.7, device="cuda")
    worst = 0.0
    for combo in WL.COMBOS:
        sw = _sw(case, combo)
        _, stats = e.window_loss(*_maps(t), **sw)
        got = dict(zip(WL.GRADS, (_np(g) for g in e.window_loss_backward(*_maps(t), stats, one, **sw))))
        g64 = WL.reference64(case, combo)[1]
        _, _, closed, arg, _ = WL.closed_forms(case, combo)
        for k in WL.GRADS:
            err = np.abs(got[k].astype(np.float64) - g64[k])
            assert np.all(err <= EPS * np.abs(g64[k])), (case, combo, k, float(np.max(err / np.maximum(np.abs(g64[k]), 1e-300))))
            worst = max(worst, float(np.max(err[g64[k] != 0] / np.abs(g64[k][g64[k] != 0]))) if np.any(g64[k] != 0) else 0.0)
            # exact zeros wherever the closed form is zero: invalid pixels, the sources that are not the arg-min, inverse = 0
            assert np.all(got[k][closed[k] == 0] == 0), (case, combo, k)
        if not combo[2]:
            assert not got["i_diff"].any() and not got["i_weight"].any()
        if combo[0] and WL.planted(case) and S > 1:        # ties of the min go to the lowest source index
            gd = got["f_diff"].reshape(S, B, H * W)[:, :, WL.PATCH["tie"]]
            assert np.all(gd[0] > 0) and not gd[1:].any()
        # g_loss scales linearly: the same double value times 1.7, rounded once
        scaled = dict(zip(WL.GRADS, (_np(g) for g in e.window_loss_backward(*_maps(t), stats, g17, **sw))))
        g17d = float(np.float32(1.7))
        for k in WL.GRADS:
            assert np.all(np.abs(scaled[k].astype(np.float64) - g17d * g64[k]) <= EPS * np.abs(g17d * g64[k])), (case, combo, k)
        # an output requested alone has the bits it has next to the others
        if combo in (WL.COMBOS[0], WL.COMBOS[-1]) or case == WL.CASES[2]:
            for j, k in enumerate(WL.GRADS):
                alone = e.window_loss_backward(*_maps(t), stats, one, want=tuple(i == j for i in range(4)), **sw)
                assert all((a is None) == (i != j) for i, a in enumerate(alone))
                assert _same(_np(alone[j]), got[k]), (case, combo, k)
    print(f"{case}: largest relative error of a gradient entry {worst:.3e} (bound {EPS:.3e})")


def test_no_output_and_bad_arguments_are_errors(dev):
    case = WL.CASES[2]
    t, e = dev(case)
    sw = _sw(case, WL.COMBOS[0])
    _, stats = e.window_loss(*_maps(t), **sw)
    with pytest.raises(RuntimeError, match="no output requested"):
        e.window_loss_backward(*_maps(t), stats, torch.tensor(1.0, device="cuda"), want=(False,) * 4, **sw)
    import ctypes as C
    from tightly_coupled_sfm_amd._lib import default_opts
    p = [e._p(m) for m in _maps(t)]
    loss, st = torch.empty((), device="cuda"), torch.empty(7, dtype=torch.float64, device="cuda")
    assert e.lib.tcsfm_window_loss(e._h, C.byref(default_opts()), 1, 5, 1, 1, *p, e._p(loss), e._p(st)) != 0      # S > 4
    assert "S must be 1 .. 4" in e.last_error()
    assert e.lib.tcsfm_window_loss(e._h, C.byref(default_opts()), 2, 0, 1, 1, *p, e._p(loss), e._p(st)) != 0
    with pytest.raises(ValueError):
        e.window_loss(*_maps(t), **dict(sw, S=3))          # 4 maps are not 3 sources of B targets


@pytest.mark.parametrize("case", [WL.CASES[1], WL.CASES[3], WL.CASES[6]], ids=[IDS[1], IDS[3], IDS[6]])
def test_reproducible(dev, case):
    """a second call and a call on a side stream give the same bits; under no_grad the fused loss saves nothing"""
    from tightly_coupled_sfm_amd import losses
    t, e = dev(case)
    one = torch.tensor(1.0, device="cuda")
    for combo in (WL.COMBOS[0], WL.COMBOS[-1]):
        sw = _sw(case, combo)
        a = e.window_loss(*_maps(t), **sw)
        ga = e.window_loss_backward(*_maps(t), a[1], one, **sw)
        b = e.window_loss(*_maps(t), **sw)
        gb = e.window_loss_backward(*_maps(t), b[1], one, **sw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = e.window_loss(*_maps(t), **sw)
            gc = e.window_loss_backward(*_maps(t), c[1], one, **sw)
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        for x in (b, c):
            assert _same(_np(a[0]), _np(x[0])) and np.array_equal(_np(a[1]).view(np.uint64), _np(x[1]).view(np.uint64))
        for gx in (gb, gc):
            assert all(_same(_np(p), _np(q)) for p, q in zip(ga, gx))
    H, W, B, S = case
    fwd, inv = WL.data_dicts(t)
    with torch.no_grad():
        L = losses.compute_optimization_loss(WL.options(WL.COMBOS[0], S), t["f_diff"][:B].repeat(1, 3, 1, 1), None, None, fwd, inv, None, fused=True)
    assert L.grad_fn is None and not L.requires_grad and L.shape == (1,)
    assert _same(_np(L), _np(e.window_loss(*_maps(t), **_sw(case, WL.COMBOS[0]))[0]).reshape(1))


def test_autograd_function(dev):
    """_WindowLoss: gradients only where needs_input_grad asks, the library's bits, masks without a gradient"""
    from tightly_coupled_sfm_amd import losses
    case = WL.CASES[3]
    H, W, B, S = case
    t, e = dev(case)
    for combo in (WL.COMBOS[0], WL.COMBOS[5], WL.COMBOS[-1]):
        x = {k: v.clone() for k, v in t.items()}
        for k in ("f_diff", "i_weight"):
            x[k].requires_grad_()
        fwd, inv = WL.data_dicts(x)
        L = losses.compute_optimization_loss(WL.options(combo, S), x["f_diff"][:B].detach().repeat(1, 3, 1, 1), None, None, fwd, inv, None, fused=True)
        assert L.shape == ((1,) if combo[0] else ()) and L.dtype == torch.float32 and L.grad_fn is not None
        (L.sum() * 1.7).backward()
        assert x["f_weight"].grad is None and x["i_diff"].grad is None and x["f_valid"].grad is None
        sw = _sw(case, combo)
        _, stats = e.window_loss(*_maps(t), **sw)
        ref = e.window_loss_backward(*_maps(t), stats, torch.tensor(1.7, device="cuda"), want=(True, False, False, True), **sw)
        assert _same(_np(x["f_diff"].grad), _np(ref[0]))
        if combo[2]:
            assert _same(_np(x["i_weight"].grad), _np(ref[3]))
        else:
            assert x["i_weight"].grad is None or not _np(x["i_weight"].grad).any()


def _e2e(fused):
    from tightly_coupled_sfm_amd import helpers, learning_helpers, losses
    i = {k: _t(v) for k, v in LG.e2e_inputs().items()}
    disp_t, disp_s = i["disp_t"].clone().requires_grad_(), i["disp_s"].clone().requires_grad_()
    depth_t, depth_s = (learning_helpers.disp_to_depth(d, *LG.E2E_DEPTH_RANGE)[1] for d in (disp_t, disp_s))
    tgt2, dt2 = i["tgt"].repeat(2, 1, 1, 1), depth_t.repeat(2, 1, 1, 1)
    fwd = helpers.compute_photometric_error(tgt2, i["src"], dt2, depth_s, i["pose"], i["K"])
    inv = helpers.compute_photometric_error(i["src"], tgt2, depth_s, dt2, -i["pose"], i["K"])
    assert fwd["valid_mask"].grad_fn is None and inv["valid_mask"].grad_fn is None
    L = losses.compute_optimization_loss(LG.E2E_OPTIONS, i["tgt"], disp_t, i["disp_init"], fwd, inv, losses.SSIM_Loss(), fused=fused)
    L.backward()
    masks = dict(fwd_valid=_np(fwd["valid_mask"]), inv_valid=_np(inv["valid_mask"]))
    return L.detach(), dict(d_disp_t=_np(disp_t.grad), d_disp_s=_np(disp_s.grad)), masks, (fwd, inv, i)


def test_compute_optimization_loss_fused_end_to_end():
    """17 x 33, B = 1, S = 2 (tests/loss_grad_inputs.e2e_inputs): disparity leaves -> disp_to_depth -> compute_photometric_error, forward
    and inverse -> compute_optimization_loss(fused=True) -> backward(), judged as test_gpu_loss_grad.py judges the unfused chain"""
    from tightly_coupled_sfm_amd import losses
    L, got, masks, (fwd, inv, i) = _e2e(True)
    L0, got0, masks0, _ = _e2e(False)
    assert L.shape == L0.shape and L.dtype == L0.dtype == torch.float32
    assert all(np.array_equal(masks[k], masks0[k]) for k in masks) and masks["fwd_valid"].sum() > 0 and masks["inv_valid"].sum() > 0
    (ref, L64), (t32, _) = LG.e2e_twin(masks), LG.e2e_twin(masks, "f32")
    print(f"17x33-B1-S2/fused end_to_end\tloss={float(L):.9e}\tunfused={float(L0):.9e}\tfloat64 twin={L64:.9e}")
    assert abs(float(L) - L64) < 1e-3 * abs(L64)
    fails, worst = LG.judge(got, ref, t32, "17x33-B1-S2/fused_end_to_end", LG.E2E_TENSORS, print, None)
    print("17x33-B1-S2/fused_end_to_end\tworst ratio to the float32 twin | largest relative L2\t" + "\t".join(f"{k}={v[0]:.3f}|{v[1]:.2e}" for k, v in worst.items()))
    assert not fails, fails
    # the argmin form has the reference's shape too
    opts = dict(LG.E2E_OPTIONS, diff_img_argmin=True, l_depth_init=False, l_smooth=False)
    with torch.no_grad():
        a, b = (losses.compute_optimization_loss(opts, i["tgt"], None, None, fwd, inv, None, fused=f) for f in (True, False))
    # (the torch expression sums 2 x 561 float32 terms: n 2^-24 = 6.7e-5 relative at worst)
    assert a.shape == b.shape == (1,) and a.dtype == b.dtype and abs(float(a) - float(b)) <= 1e-4 * abs(float(b))
    # no silent fallback
    cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}
    with pytest.raises(ValueError):
        losses.compute_optimization_loss(opts, i["tgt"].cpu(), None, None, cpu(fwd), cpu(inv), None, fused=True)
    with pytest.raises(ValueError):
        losses.compute_optimization_loss(opts, i["tgt"], None, None, {k: v.detach().double() for k, v in fwd.items()}, inv, None, fused=True)
    with pytest.raises(ValueError):
        losses.compute_optimization_loss(dict(opts, num_source_imgs=5), i["tgt"], None, None, fwd, inv, None, fused=True)
