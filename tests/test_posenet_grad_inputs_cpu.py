"""The references of the PoseNet input-gradient tests, checked without a GPU (tests/posenet_grad_inputs.py):
  * forward_pinned with the twin's own ReLU decisions reproduces plain float64 autograd of standins.PoseNetTwin, and so does
    backward_manual, the torch-level restatement of the backward's formulas the planted faults are made from;
  * the float32 yardstick passes its own judge;
  * every planted fault fails the judge at every case shape, under the fp32-exact dense cotangent.
"""
import functools

import pytest

torch = pytest.importorskip("torch")

import posenet_grad_inputs as GI      # noqa: E402
import posenet_layers as PL           # noqa: E402


@functools.lru_cache(maxsize=None)
def _case(i, pset="base"):
    """shared per case: inputs, own masks, float64 reference, float32 yardstick (computed once, never modified)"""
    H, W, N, _ = GI.CASES[i]
    sd = PL.PARAM_SETS[pset](0)
    x = PL.images(H, W, N, seed=3)
    d = GI.cotangent_dense(N, i)
    with torch.no_grad():
        masks = GI.forward_pinned(sd, x)[1]
    ref = GI.grad_pinned(sd, x, masks, d)
    yard = GI.grad_pinned(sd, x, masks, d, torch.float32)
    return sd, x, d, masks, ref, yard


@pytest.mark.parametrize("i", range(len(GI.CASES)), ids=GI.CASE_IDS)
def test_pinned_reference_is_autograd(i):
    sd, x, d, masks, ref, _ = _case(i)
    plain = GI.grad_plain64(sd, x, d)
    assert PL.rel_l2(ref, plain) < 1e-12, PL.rel_l2(ref, plain)
    manual = GI.backward_manual(sd, x, masks, d)
    assert PL.rel_l2(manual, ref) < 1e-11 and PL.max_over_rms(manual, ref) < 1e-10, GI.figures(manual, ref)


@pytest.mark.parametrize("pset", ["base", "gamma"])
def test_yardstick_passes_its_own_judge(pset):
    for i in (0, 1, 3):
        _, _, _, _, ref, yard = _case(i, pset)
        ok, fig = GI.judge(yard, ref, yard)
        assert ok and fig["rel_l2"] < 1e-4, fig


@pytest.mark.parametrize("fault", GI.FAULTS)
@pytest.mark.parametrize("i", range(len(GI.CASES)), ids=GI.CASE_IDS)
def test_planted_fault_fails_the_judge(i, fault):
    sd, x, d, masks, ref, yard = _case(i)
    ok, fig = GI.judge(GI.backward_manual(sd, x, masks, d, fault), ref, yard)
    assert not ok, (fault, fig)


def test_constant_frame_has_zero_variance_groups():
    x = GI.constant_frames(17, 33, 2)
    assert float(PL.operand64(1, x).abs().max()) == 0.0
    sd = PL.PARAM_SETS["base"](0)
    c = PL.chained64(sd, x)
    sc = c["scsh"][0][:, :, 0] / torch.as_tensor(sd["conv1.1.weight"]).double()
    assert torch.allclose(sc, torch.full_like(sc, 1e-5 ** -0.5), rtol=1e-12)
