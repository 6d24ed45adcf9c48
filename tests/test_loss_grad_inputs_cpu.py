"""The inputs, the float64 reference and the judge of the loss-gradient tests (tests/loss_grad_inputs.py), checked without a GPU: the
SSIM mask stays under the cap, the smooth-loss inputs have no sign disagreement and no near-tie (a bad input is reported as a bad
input), the numpy statements of the three closed forms -- the l_n identity and the reflect multiplicity included -- are the float64
autograd gradients, the end-to-end inputs keep every SSIM pixel off the clamp and their masks are not empty, and the judge rejects
four planted faults (the fifth, an open-interval clamp, is shown to change nothing but rounding noise)."""
import numpy as np
import pytest

import loss_grad_inputs as LG

torch = pytest.importorskip("torch")
PG = LG.PG


@pytest.mark.parametrize("case", LG.CASES, ids=LG.IDS)
def test_inputs_are_fit_for_the_purpose(case):
    H, W, N = case
    ties, flips = LG.ssim_mask(case)
    per_item = (ties | flips).any(1).reshape(N, -1).sum(1)
    print(case, "ssim ties", ties.sum(), "float32 gates otherwise", flips.sum(), "masked pixels per item", per_item.tolist(), "cap", LG.mask_cap(H * W))
    assert (per_item <= LG.mask_cap(H * W)).all(), (case, per_item, LG.mask_cap(H * W))
    g = LG.ssim_cotangent(case)
    assert not g[ties | flips].any() and (g != 0).sum() >= g.size - SSIM_MASKED_MAX(case)
    x, y = LG.make_ssim(case)
    v = PG.ssim_raw(torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)).numpy()
    r0, r1, c0, c1 = LG.same_region(H, W)
    assert np.array_equal(x[0, :, r0:r1, c0:c1], y[0, :, r0:r1, c0:c1])
    if H >= 5:
        assert (np.abs(v[0, :, r0 + 1:r1 - 1, c0 + 1:c1 - 1]) < LG.TIE).all()          # y = x: the value sits at the clamp's lower edge
    off = np.ones(v.shape, bool); off[0, :, r0:r1, c0:c1] = False
    assert (v[off] > 1e-3).all() and (v[off] < 1 - 1e-3).all(), (v[off].min(), v[off].max())
    disp = LG.make_disp(case)
    bad_sign, near = LG.smooth_input_report(disp)
    assert bad_sign == 0 and near == 0, (case, "bad smooth-loss input", bad_sign, near)
    p0, p1, q0, q1 = LG.patch(H, W)
    assert (disp[:, :, p0:p1, q0:q1] == disp[:, :, p0:p0 + 1, q0:q0 + 1]).all() and (p1 - p0) * (q1 - q0) >= 2
    assert all(not np.array_equal(disp[i], disp[j]) for i in range(N) for j in range(i))
    assert np.array_equal(np.round(disp.astype(np.float64) * 4096), disp.astype(np.float64) * 4096)


def SSIM_MASKED_MAX(case):
    H, W, N = case
    return N * LG.SSIM_C * LG.mask_cap(H * W)


@pytest.mark.parametrize("case", LG.F64_CASES, ids=LG.IDS[:-1])
def test_closed_forms_are_the_autograd_gradients(case):
    H, W, N = case
    disp, img, cot = LG.make_disp(case), LG.make_img(case), LG.d2d_cotangents(case)
    for subset in LG.D2D_SUBSETS:
        l2, _ = LG.errors(LG.d2d_closed_form(disp, {k: cot[k] for k in subset}), LG.twin_d2d(case, subset)["g_disp"])
        assert l2 < 1e-13, (case, subset, l2)
    x, y = LG.make_ssim(case)
    ref = LG.twin_ssim(case)
    for side in LG.SSIM_OUTS:
        got = LG.ssim_closed_form(x, y, LG.ssim_cotangent(case), side)
        for n in range(N):
            l2, _ = LG.errors(got[n], ref[side][n])
            assert l2 < 1e-10, (case, side, n, l2)
    if H > 2:
        assert not np.allclose(LG.ssim_closed_form(x, y, LG.ssim_cotangent(case), "g_y", multiplicity=False), ref["g_y"], rtol=1e-6, atol=0)
    got, ln, coupling = LG.smooth_closed_form(disp, img)
    ref = LG.twin_smooth(case)["g_disp"]
    for n in range(N):
        l2, mx = LG.errors(got[n], ref[n])
        print(case, n, "smooth closed form vs autograd: rel_l2", l2, "max/rms", mx)
        assert l2 < 1e-12, (case, n, l2)
    assert np.allclose(coupling, ln, rtol=1e-12, atol=0), (coupling, ln)          # sum_j g_n[j] n_j = l_n: no second reduction
    assert abs(ln.sum() - LG.smooth_gradient(disp, img)[1]) < 1e-14


def test_reflect_multiplicity_counts():
    """m(q, p) along one axis: 1 inside, 2 next to a border, and at a length of 2 each pixel is hit twice by the other's window"""
    def mult(q, p, n):
        return sum(int(LG._refl(np.array(q + d), n)) == p for d in (-1, 0, 1))
    assert [mult(q, p, 5) for q, p in ((2, 2), (2, 1), (0, 1), (1, 0), (0, 0), (4, 3), (3, 4))] == [1, 1, 2, 1, 1, 2, 1]
    assert [mult(q, p, 2) for q, p in ((0, 0), (0, 1), (1, 0), (1, 1))] == [1, 2, 2, 1]


def test_float32_twin_passes_the_judge_and_float64_is_exact():
    case = (17, 33, 3)
    for ref, t32, tensors in ((LG.twin_d2d(case), LG.twin_d2d(case, LG.D2D_COTS, "f32"), ("g_disp",)),
                              (LG.twin_ssim(case), LG.twin_ssim(case, "f32"), LG.SSIM_OUTS),
                              (LG.twin_smooth(case), LG.twin_smooth(case, "f32"), ("g_disp",))):
        fails, worst = LG.judge(t32, ref, t32, "f32", tensors)
        assert not fails and all(v[0] <= 1.0 for v in worst.values()), (fails, worst)
        assert not LG.judge(ref, ref, t32, "f64", tensors)[0]


FAULT_CASES = [(5, 9, 3), (17, 33, 3), (37, 53, 3)]


@pytest.mark.parametrize("case", FAULT_CASES, ids=[LG.IDS[LG.CASES.index(c)] for c in FAULT_CASES])
def test_judge_rejects_planted_faults(case):
    """each fault, planted at numpy level into the closed forms, fails the judge: the mean term dropped, the multiplicity taken as 1,
    sgn(0) = 1, g_depth / s instead of / s^2.  The fifth, an open-interval clamp, is planted and shown to be invisible (see below)."""
    disp, img = LG.make_disp(case), LG.make_img(case)
    ref, t32 = LG.twin_smooth(case), LG.twin_smooth(case, "f32")
    for name, kw in (("mean_term_dropped", dict(mean_term=False)), ("sgn0_is_1", dict(sgn0=1.0))):
        assert LG.judge(dict(g_disp=LG.smooth_closed_form(disp, img, **kw)[0]), ref, t32, name, ("g_disp",))[0], (case, name)
    x, y = LG.make_ssim(case)
    ref, t32 = LG.twin_ssim(case), LG.twin_ssim(case, "f32")
    f = {s: LG.ssim_closed_form(x, y, LG.ssim_cotangent(case), s, multiplicity=False) for s in LG.SSIM_OUTS}
    assert {e[1] for e in LG.judge(f, ref, t32, "multiplicity_one", LG.SSIM_OUTS)[0]} == set(LG.SSIM_OUTS), case
    # The open-interval clamp is planted too, but it cannot be told from the closed one on SSIM by ANY judge: the value (1 - s) / 2
    # reaches 0 only where x = y on the whole window (s = 1 is the maximum of SSIM), a stationary point whose gradient is zero, and
    # never reaches 1 (s > -1 while C1 > 0).  What is asserted: windows at exactly 0 do occur under a non-zero cotangent (item 0's
    # y = x region), the fault changes those pixels, and the change is rounding noise of the cancelling terms -- so the judge, rightly,
    # lets both pass.  The closed interval is what the kernel implements (torch's convention).
    g = LG.ssim_cotangent(case)
    v = PG.ssim_raw(torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)).numpy()
    closed, opened = (LG.ssim_closed_form(x, y, g, "g_y", closed=c) for c in (True, False))
    if ((v == 0) & (g != 0)).any():
        assert np.abs(closed - opened).max() <= 1e-12 * np.abs(closed).max()
    assert not LG.judge(dict(g_x=LG.ssim_closed_form(x, y, g, "g_x", closed=False), g_y=opened), ref, t32, "open_interval_clamp", LG.SSIM_OUTS)[0]
    cot = LG.d2d_cotangents(case)
    ref, t32 = LG.twin_d2d(case), LG.twin_d2d(case, LG.D2D_COTS, "f32")
    assert LG.judge(LG.d2d_gradient(disp, cot, "f64", power=1), ref, t32, "g_depth_over_s", ("g_disp",))[0], case


def test_end_to_end_inputs():
    """the initial disparity differs enough from the leaf that no SSIM pixel sits within TIE of the clamp; the twin's own masks are not
    empty in either direction; the float32 twin passes the judge on the end-to-end gradient"""
    i = LG.e2e_inputs()
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    v = PG.ssim_raw(T(i["disp_t"]), T(i["disp_init"])).numpy()
    assert (v > LG.TIE).all() and (v < 1 - LG.TIE).all(), (v.min(), v.max())
    assert LG.smooth_input_report(i["disp_t"])[0] == 0
    m = LG.e2e_twin_masks()
    print({k: float(a.sum()) for k, a in m.items()})
    assert m["fwd_valid"].sum() > 0 and m["inv_valid"].sum() > 0
    ref, L = LG.e2e_twin(m)
    t32, L32 = LG.e2e_twin(m, "f32")
    assert np.isfinite(L) and abs(L - L32) < 1e-5 * abs(L)
    assert all(np.abs(ref[k]).max() > 0 for k in LG.E2E_TENSORS)
    assert not LG.judge(t32, ref, t32, "e2e f32", LG.E2E_TENSORS, rel_l2_max=None)[0]
