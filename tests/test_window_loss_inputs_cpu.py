"""The window loss's test inputs and closed forms, without a GPU: the closed forms of include/tcsfm.h (tests/window_loss_inputs.closed_forms)
are the float64 autograd gradients of losses.compute_optimization_loss, the min's ties go to source 0 on the CPU, and the inputs carry what
the GPU test relies on (planted stretches, non-zero denominators)."""
import numpy as np
import pytest

import window_loss_inputs as WL


def _tie_mask(case):
    H, W, B, S = case
    m = np.zeros((S, B, H * W), dtype=bool)
    if WL.planted(case):
        m[:, :, WL.PATCH["tie"]] = True
    return m.reshape(S * B, 1, H, W)


@pytest.mark.parametrize("case", WL.CASES, ids=lambda c: "x".join(map(str, c)))
def test_closed_forms_are_float64_autograd(case):
    H, W, B, S = case
    tie = _tie_mask(case)
    for combo in WL.COMBOS:
        loss64, g64 = WL.reference64(case, combo)
        loss, stats, g, arg, valid_min = WL.closed_forms(case, combo)
        assert loss64.shape == ((1,) if combo[0] else ())
        assert stats[1] > 0 and (stats[3] > 0 or not combo[2]), (case, combo, stats)
        assert abs(loss - float(loss64.reshape(-1)[0])) <= 1e-12 * abs(loss), (case, combo)
        for k in WL.GRADS:
            off = ~tie if k == "f_diff" else np.ones_like(tie)
            # 1e-12 of the terms' size: a weight gradient is a difference q - w / n of two float64 terms that nearly cancel at a few of
            # the 245 760 pixels of the real grid, so the bound is relative to |q| + w / n <= |g| + 2 w / n, not to |g| alone
            scale = np.abs(g64[k]) + (2 * combo[3] / stats[6] if k.endswith("weight") else 0.0)
            assert np.all((np.abs(g[k] - g64[k]) <= 1e-12 * scale)[off]), (case, combo, k)
        if combo[0] and WL.planted(case) and S > 1:
            # ties: torch.min(dim) on the CPU sends the gradient to the lowest source index, and so does the contract
            gd = g64["f_diff"].reshape(S, B, H * W)[:, :, WL.PATCH["tie"]]
            assert np.all(gd[0] > 0) and np.all(gd[1:] == 0)
            assert np.array_equal(g["f_diff"].reshape(S, B, H * W)[:, :, WL.PATCH["tie"]], gd) or np.allclose(
                g["f_diff"].reshape(S, B, H * W)[:, :, WL.PATCH["tie"]], gd, rtol=1e-12, atol=0)
            assert np.all(arg.reshape(B, H * W)[:, WL.PATCH["tie"]] == 0)


@pytest.mark.parametrize("case", WL.CASES, ids=lambda c: "x".join(map(str, c)))
def test_planted_patches_exist(case):
    H, W, B, S = case
    x = {k: v.reshape(S, B, H * W) for k, v in WL.inputs(case).items()}
    assert all(v.dtype == np.float32 for v in x.values())
    if not WL.planted(case):
        assert H * W < 64
        return
    p = WL.PATCH["invalid"]
    assert np.all(x["f_valid"][:, :, p] == 0) and np.all(x["i_valid"][:, :, p] == 0)
    p = WL.PATCH["tie"]
    assert np.all(x["f_diff"][:, :, p] == x["f_diff"][0:1, :, p]) and np.all(x["f_valid"][:, :, p] == 1)
    for automask in (True, False):
        _, _, _, _, valid_min = WL.closed_forms(case, (True, automask, True, 0.0))
        assert np.all(valid_min.reshape(B, H * W)[:, p] == 1)
        assert np.all(valid_min.reshape(B, H * W)[:, WL.PATCH["invalid"]] == 0)
    p = WL.PATCH["zero_weight"]
    assert np.all(x["f_weight"][:, :, p] == 0) and np.all(x["i_weight"][:, :, p] == 0)
    assert max(s.stop for s in WL.PATCH.values()) <= H * W
    # the stretches straddle the kernel's four-pixel units
    assert all(s.start % 4 and s.stop % 4 for s in WL.PATCH.values())
