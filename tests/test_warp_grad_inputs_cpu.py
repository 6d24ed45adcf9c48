"""The inputs, the float64 reference and the judge of the warp-gradient tests (tests/warp_grad_inputs.py), checked without a GPU:
the tie mask keeps its conditions on every case, every item of a batch differs, the twin's autograd gradients agree with central
finite differences of the float64 twin (independent of autograd), the judge rejects six planted faults each by the criterion
that should catch it, and the new entry point is declared in the header and in the binding."""
import os
import re

import numpy as np
import pytest

import warp_grad_inputs as WG

torch = pytest.importorskip("torch")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", WG.CASES, ids=WG.IDS)
def test_tie_mask_conditions(case):
    """the masked share of an item's frame is at most max(2 pixels, 1.5 %), the float32 twin takes the float64 cell at every unmasked
    valid pixel, the cotangents vanish on the mask and differ in scale between items and maps"""
    H, W, N, s = case
    near, g = WG.tie_mask(case)
    share = (near & g["valid"]).sum(1)
    print(case, "masked valid pixels per item", share.tolist(), "cap", WG.mask_cap(H * W), "clamped", int((g["p2"] < 1e-3).sum()))
    assert (share <= WG.mask_cap(H * W)).all(), (case, share, WG.mask_cap(H * W))
    assert WG.cell_flips32(case) == 0, case
    cot = WG.cotangents(case)
    for k in WG.COTS:
        assert not cot[k][np.broadcast_to(near.reshape(N, 1, H, W), cot[k].shape)].any()
    lg = np.log10([[np.sqrt((cot[k][n].astype(np.float64) ** 2).mean()) for n in range(N)] for k in WG.COTS])
    for n in range(N):                # half a decade or more between the maps of an item and between neighbouring items of a map
        assert min(abs(lg[a, n] - lg[b, n]) for a in range(3) for b in range(a)) > 0.4, lg
        assert n == 0 or (np.abs(lg[:, n] - lg[:, n - 1]) > 0.4).all(), lg


@pytest.mark.parametrize("case", WG.CASES, ids=WG.IDS)
def test_items_differ(case):
    assert WG.OI.items_differ(WG.make_case(*case))


def test_scale_30_reaches_the_clamp_and_leaves_the_frame():
    for case in [c for c in WG.CASES if c[3] == 30.0]:
        g = WG.tie_mask(case)[1]
        assert (g["p2"] < 1e-3).sum() > 0 and (~g["valid"]).mean() > 0.5, case


FD_CASES = [(5, 9, 3, 1.0), (17, 33, 3, 1.0), (17, 33, 3, 30.0), (37, 53, 3, 1.0)]


def _functional(case, pose, depth_t):
    c, cot = WG.make_case(*case), WG.cotangents(case)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    rec, _, pd, cd = WG.tw.warp(T(c["src"]), T(depth_t), T(c["depth_s"]), -T(pose), T(c["K"]))
    return float((rec * T(cot["g_rec"])).sum() + (pd * T(cot["g_pd"])).sum() + (cd * T(cot["g_cd"])).sum())


@pytest.mark.parametrize("case", FD_CASES, ids=[WG.IDS[WG.CASES.index(c)] for c in FD_CASES])
def test_twin_gradient_vs_finite_differences(case):
    """central differences of the float64 functional: d_pose (all 6 N entries) and d_depth_t at a handful of unmasked pixels.  The
    functional is piecewise smooth; a step of 1e-7 moves a sample by less than the 1e-3 px the mask keeps clear of every kink, so
    the difference quotient is exact up to h^2 and to the rounding eps |L| / h ~ 1e-9 |L|: bound 1e-6 of the gradient's largest
    entry of that kind (translations, rotations, depth separately)"""
    H, W, N, s = case
    c = WG.make_case(*case)
    ref = WG.twin(case)
    pose0, d0 = c["pose"].astype(np.float64), c["depth_t"].astype(np.float64)
    h = 1e-7
    fd = np.zeros((N, 6))
    for n in range(N):
        for j in range(6):
            p = pose0.copy(); p[n, j] += h
            m = pose0.copy(); m[n, j] -= h
            fd[n, j] = (_functional(case, p, d0) - _functional(case, m, d0)) / (2 * h)
    for sl in (slice(0, 3), slice(3, 6)):
        err, scale = np.abs(fd[:, sl] - ref["d_pose"][:, sl]).max(), np.abs(ref["d_pose"][:, sl]).max()
        print(case, "d_pose", sl, "fd error", err, "scale", scale)
        assert err <= 1e-6 * scale, (case, sl, err, scale)
    near = WG.tie_mask(case)[0]
    rng = np.random.default_rng(3)
    gd = ref["d_depth_t"].reshape(N, -1)
    picks = [(n, int(i)) for n in range(N) for i in rng.choice(np.flatnonzero(~near[n]), 4, replace=False)]
    scale = np.abs(gd).max()
    for n, i in picks:
        p = d0.copy().reshape(N, -1); p[n, i] += h
        m = d0.copy().reshape(N, -1); m[n, i] -= h
        q = (_functional(case, pose0, p.reshape(d0.shape)) - _functional(case, pose0, m.reshape(d0.shape))) / (2 * h)
        assert abs(q - gd[n, i]) <= 1e-6 * scale, (case, n, i, q, gd[n, i], scale)


def test_float32_twin_passes_the_judge_and_float64_is_exact():
    case = (37, 53, 3, 30.0)
    ref, t32 = WG.twin(case), WG.twin(case, WG.COTS, "f32")
    fails, worst = WG.judge(t32, ref, t32, "f32")
    assert not fails and all(v <= 1.0 for v in worst.values()), (fails, worst)
    fails, _ = WG.judge(ref, ref, t32, "f64")
    assert not fails


FAULT_CASES = [(17, 33, 3, 30.0), (37, 53, 3, 30.0), (100, 333, 2, 30.0)]


@pytest.mark.parametrize("case", FAULT_CASES, ids=[WG.IDS[WG.CASES.index(c)] for c in FAULT_CASES])
def test_judge_rejects_planted_faults(case):
    """each fault, planted at numpy level into the true float64 gradient, fails the judge on the tensors it touches, by the criterion
    that should catch it, and on no other tensor"""
    ref, t32 = WG.twin(case), WG.twin(case, WG.COTS, "f32")
    expect = dict(w_factor_dropped="rel_l2", tap_weight_swapped="rel_l2", g_cd_dropped_out_of_frame="rel_l2", d_pose_sign="rel_l2",
                  item0_for_all="rel_l2", clamp_ignored="exact zero")
    for name, (faulty, tensors) in WG.planted_faults(case).items():
        fails, _ = WG.judge(faulty, ref, t32, name)
        hit = {f[1] for f in fails}
        assert hit == set(tensors), (case, name, hit, tensors)
        for k in tensors:
            assert any(f[1] == k and f[3].startswith(expect[name]) for f in fails), (case, name, k, fails)


def test_entry_point_is_declared():
    """tcsfm_warp_backward is in the header and in the binding's export list (fails before the feature exists)"""
    from tightly_coupled_sfm_amd import _lib
    assert "tcsfm_warp_backward" in _lib.EXPORTS
    header = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    assert re.search(r"\bint\s+tcsfm_warp_backward\s*\(", header)
    res, args = _lib._SIGNATURES["tcsfm_warp_backward"]
    assert len(args) == 14          # handle, opts, N, five inputs, three cotangents, three outputs
