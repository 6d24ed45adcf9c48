"""The inputs of the coupled pose loop's gradient test, checked without a GPU (tests/pose_loop_grad_inputs.py): the committed
candidates hold the search's conditions with room, and the twin loop's gradient is a gradient."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pose_loop_grad_inputs as LI      # noqa: E402


@pytest.mark.parametrize("config", list(LI.CONFIGS))
def test_committed_candidate_holds(config):
    """the candidate the GPU test uses holds every condition, with room: its margin is 13.8 x (many) and 21 x (few) against the
    HEADROOM of 8, and the float32 twin's rounding on another host (thread count, convolution algorithm) moved margins by about a
    tenth where it was observed.  Candidates near the threshold may change
    sides from host to host: HOLDING records the search as it came out where it was run, and only its first entry is relied upon."""
    seed = LI.chosen(config)
    assert seed is not None and seed == LI.HOLDING[config][0]
    c = LI.conditions(config, seed)
    assert not LI.conditions_hold(c) and c["margin_ratio"] >= LI.HEADROOM, c
    assert seed in LI.search(config)
    inp = LI.inputs(config, seed)
    B, S = LI.CONFIGS[config]
    assert inp["srcs"].shape == (S, B, 3, LI.H, LI.W) and 0 < inp["disp_t"].min() and inp["disp_s"].max() < 1
    assert np.array_equal(inp["R"] * 8, np.round(inp["R"] * 8))


def test_search_rejects_a_candidate_without_headroom():
    c = LI.conditions("few", 4)            # a sample 7e-6 px off a cell border: 1.3 x the coordinate difference
    assert c["margin_ratio"] < 0.5 * LI.HEADROOM and LI.conditions_hold(c) and 4 not in LI.search("few")


def test_twin_gradient_against_a_finite_difference():
    """the float64 twin loop's gradient predicts the scalar's change under a small disparity step (the step keeps every cell: the
    chosen inputs have 1e-4 px of room)"""
    inp = dict(LI.inputs("few", LI.chosen("few")))
    a = LI.twin_loop(inp, torch.float64, grad=True)
    assert np.abs(a["d_disp_t"]).max() > 0 and np.abs(a["d_disp_s"]).max() > 0
    rng = np.random.default_rng(5)
    scalar = lambda r: float((r["stacked"] * inp["R"].astype(np.float64)).sum())
    vt, vs = rng.standard_normal(inp["disp_t"].shape), rng.standard_normal(inp["disp_s"].shape)
    eps = 1e-7
    vals = []
    for sgn in (1.0, -1.0):
        q = dict(inp, disp_t=inp["disp_t"].astype(np.float64) + sgn * eps * vt, disp_s=inp["disp_s"].astype(np.float64) + sgn * eps * vs)
        vals.append(scalar(LI.twin_loop(q, torch.float64, masks=a["masks"])))
    fd = (vals[0] - vals[1]) / (2 * eps)
    an = float((a["d_disp_t"] * vt).sum() + (a["d_disp_s"] * vs).sum())
    assert abs(fd - an) < 1e-5 * abs(an), (fd, an)


def test_yardstick_passes_its_own_judge():
    inp = LI.inputs("few", LI.chosen("few"))
    a = LI.twin_loop(inp, torch.float64, grad=True)
    b = LI.twin_loop(inp, torch.float32, masks=a["masks"], grad=True)
    fails, figs = LI.judge(b, a, b)
    assert not fails and all(f["rel_l2"] < 1e-3 for f in figs.values()), figs
    wrong = dict(d_disp_t=-a["d_disp_t"], d_disp_s=a["d_disp_s"])
    assert LI.judge(wrong, a, b)[0]
