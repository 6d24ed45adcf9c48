"""The inputs and the judges of the composed weight-tuning chain (tests/tuning_chain_inputs.py), checked without a GPU: the conditions
the GPU tests rely on hold at the float32 twin network's disparities (and the boundary headroom at the accuracy shape; the larger
shape's is reported, see the inputs module on why it cannot hold there), the depth-init SSIM stays off its clamp, the unfaulted
float64 gradient rounded to float32 passes both judges, and each of six planted faults of the composition is rejected by both."""
import numpy as np
import pytest

import tuning_chain_inputs as TC

torch = pytest.importorskip("torch")
LG = TC.LG


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.IDS)
def test_inputs_are_fit_for_the_purpose(shape):
    """every disparity strictly inside (0, 1); each of the four directed pairs keeps at least half of the frame; float32 and float64
    geometry take the same cell and validity at every pixel; no depth near the clamp; no sign disagreement in the smooth loss; at
    ACCURACY_SHAPE no valid sample closer to a cell or frame boundary than 8 x the float32 / float64 coordinate difference"""
    c = TC.conditions(shape, TC.twin_disparity(shape))
    print(shape, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in c.items()})
    bad = TC.conditions_hold(c, headroom=shape == TC.ACCURACY_SHAPE)
    assert not bad, (shape, bad, c)
    p = TC.poses(shape)
    assert p.shape == (2, 6) and not np.array_equal(p[0], p[1])
    im = TC.images(shape)
    assert all(not np.array_equal(im[i], im[j]) for i in range(3) for j in range(i))


def test_accuracy_inputs_keep_the_depth_init_term_off_its_clamp():
    """the perturbed initial disparity differs enough from the target's that no SSIM pixel sits within TIE of the clamp (as
    loss_grad_inputs' end-to-end inputs), the twin's own masks are not empty, and every tensor of the gradient is non-zero"""
    inp, masks, ref, t32 = TC.twin_chain(TC.ACCURACY_SHAPE)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    v = LG.PG.ssim_raw(T(inp["disp_t"]), T(inp["disp_init"])).numpy()
    assert (v > LG.TIE).all() and (v < 1 - LG.TIE).all(), (v.min(), v.max())
    assert masks["fwd_valid"].sum() > 0 and masks["inv_valid"].sum() > 0
    assert all(np.abs(ref[k][n]).max() > 0 for k in TC.TENSORS for n in range(ref[k].shape[0]))


def test_clean_baseline_passes_both_judges():
    """the float64 gradient, rounded to float32, against itself; and the float32 twin passes the loss-side judge at ratio 1"""
    shape = TC.ACCURACY_SHAPE
    _, _, ref, t32 = TC.twin_chain(shape)
    rounded = {k: v.astype(np.float32) for k, v in ref.items()}
    fails, _ = TC.loss_judge(rounded, ref, t32, "rounded")
    assert not fails, fails
    # (the float32 twin may leave a rounding residue of 1 / cd - cd / cd^2, analytically zero, at an out-of-frame pixel where float64
    # happens to cancel exactly: its exact-zero entries are not held against the yardstick)
    fails, worst = TC.loss_judge(t32, ref, t32, "f32")
    fails = [f for f in fails if f[3] != "exact zero"]
    assert not fails and all(w[0] <= 1.0 for w in worst.values()), (fails, worst)
    true = TC.twin_param_gradients(shape, TC.join(ref))
    bad, worst = TC.param_judge({k: g.float() for k, g in true.items()}, true)
    print("rounded parameter gradients:", worst)
    assert not bad, bad
    assert len([k for k in true if k.startswith(TC.dt.ENC)]) == 60 and all(bool(g.any()) for g in true.values())


def test_judges_reject_planted_faults():
    """each fault of the composition fails the loss-side judge on the tensor it touches (and on no other), and, handed to the
    network as its cotangent, fails the parameter judge"""
    shape = TC.ACCURACY_SHAPE
    _, _, ref, t32 = TC.twin_chain(shape)
    true = TC.twin_param_gradients(shape, TC.join(ref))
    touches = dict(sources_detached="d_disp_s", repeat_counted_once="d_disp_t", depth_init_dropped="d_disp_t", smoothness_dropped="d_disp_t",
                   inverse_ref_depth_dropped="d_disp_t", image1_cotangent_to_image2="d_disp_s")
    faults = TC.planted_faults(shape)
    assert sorted(faults) == sorted(touches)
    for name, faulty in faults.items():
        fails, worst = TC.loss_judge(faulty, ref, t32, name)
        assert {f[1] for f in fails} == {touches[name]}, (name, fails)
        bad, w = TC.param_judge(TC.twin_param_gradients(shape, TC.join(faulty)), true)
        print(name, "loss side: worst ratio | relative L2", worst[touches[name]], "parameters over their bound:", len(bad), "of", len(true), w)
        assert bad, name
