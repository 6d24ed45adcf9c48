"""The yardsticks of the PoseNet parameter-gradient tests, without a GPU (tests/posenet_param_grad_inputs.py): the float64
restatement of the backward's parameter formulas reproduces autograd of the pinned twin, the float32 twin passes the judge it
defines (conv1.0.bias inside its derived bound), and every planted fault fails that judge, at every small shape of the GPU test, on
the tensors FAULT_TENSORS names."""
import pytest

torch = pytest.importorskip("torch")

import posenet_grad_inputs as GI          # noqa: E402
import posenet_layers as PL               # noqa: E402
import posenet_param_grad_inputs as PG    # noqa: E402

_CACHE = {}


def _case(H, W, N):
    """references of one shape, computed once: (sd, x, d, masks, ref64, yard32, bound)"""
    key = (H, W, N)
    if key not in _CACHE:
        sd = PL.PARAM_SETS["base"](3)
        x = PL.images(H, W, N, seed=5)
        d = GI.cotangent_dense(N, H + N)
        ref, masks = PG.param_grads_pinned(sd, x, None, d)
        yard, _ = PG.param_grads_pinned(sd, x, masks, d, torch.float32)
        _CACHE[key] = (sd, x, d, masks, ref, yard, PG.conv1_bias_bound(sd, x, masks, d))
    return _CACHE[key]


@pytest.mark.parametrize("H,W,N", PG.CPU_SHAPES)
def test_restatement_reproduces_autograd_and_yardstick_passes(H, W, N):
    sd, x, d, masks, ref, yard, bound = _case(H, W, N)
    man = PG.param_backward_manual(sd, x, masks, d)
    for k in PG.NAMES:
        if k == PG.DEGENERATE:
            assert float(man[k].abs().max()) < 1e-12 and float(ref[k].abs().max()) < 1e-12
        else:
            assert PL.rel_l2(man[k], ref[k]) < 1e-10, k
    bad, figs = PG.judge_all(yard, ref, yard, bound)
    assert not bad, (bad, figs)
    assert figs[PG.DEGENERATE]["worst_over_bound"] < 0.5


@pytest.mark.parametrize("fault", PG.FAULTS)
@pytest.mark.parametrize("H,W,N", PG.CPU_SHAPES)
def test_planted_fault_fails_the_judge(H, W, N, fault):
    sd, x, d, masks, ref, yard, bound = _case(H, W, N)
    man = PG.param_backward_manual(sd, x, masks, d, fault)
    bad, figs = PG.judge_all(man, ref, yard, bound)
    missed = [k for k in PG.FAULT_TENSORS[fault] if k not in bad]
    assert not missed, (fault, missed, {k: figs[k] for k in missed})
    # a fault touches nothing but its own family of tensors
    family = PG.FAULT_TENSORS[fault][0].split(".", 1)[1] if fault != "unmasked_affine" else "1."
    assert all(family in k or k.startswith("pose_pred") for k in bad), bad
