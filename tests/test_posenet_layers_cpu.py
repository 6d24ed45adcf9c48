"""CPU: the float64 references, the rounding bound and the case table of tests/posenet_layers.py, which the GPU tests of the
PoseNet's layers (tests/test_gpu_posenet_layers.py) judge the HIP kernels with.

MEASURED here: the chained float64 twin against golden_posenet.npz (written by the reference's fp32 module, so the distance is
the fixture's own fp32 error) -- poses 1.9e-6 / 3.3e-6 of the largest pose (fixture a / b), feat7 7.3e-6 / 1.1e-5 absolute, per-layer
statistics 5.2e-8 / 4.6e-8 relative; the bounds below are twice the larger figure, rounded (the fp32 check of
tests/test_posenet_cpu.py allows 1e-5, 1e-4 and 1e-5).  torch's fp32 convolution uses at most 0.02 of the rounding bound."""
import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")

import posenet_layers as PL      # noqa: E402
import standins                  # noqa: E402


def test_chained_float64_twin_vs_reference_golden():
    from tightly_coupled_sfm_amd import synth
    g = load_golden("posenet")
    sd = standins.posenet_params(int(g["seed"]))
    for tag, (H, W, N) in (("a", (48, 160, 4)), ("b", (192, 640, 2))):
        b = synth.make_batch(N, H, W, seed0=40, both_directions=True)
        x = torch.tensor(np.concatenate([b["tgt"], b["src"]], 1))
        c = PL.chained64(sd, x)
        ref = g[f"{tag}_pose"]
        e_pose = np.max(np.abs(c["pose"].numpy() - ref)) / np.abs(ref).max()
        e_feat = np.max(np.abs(c["act"][6].numpy() - g[f"{tag}_feat7"]))
        e_stat = max(np.max(np.abs(np.array([float(f.mean()), float(f.abs().mean())]) / g[f"{tag}_feat{i + 1}_stats"] - 1)) for i, f in enumerate(c["act"]))
        print(f"{tag}: pose {e_pose:.2e} feat7 {e_feat:.2e} stats {e_stat:.2e}")
        assert e_pose < 7e-6 and e_feat < 2.5e-5 and e_stat < 1e-7


@pytest.mark.parametrize("pset", sorted(PL.PARAM_SETS))
def test_isolated_reference_equals_chained(pset):
    """layer l alone on the chained twin's own (raw, scale/shift) of layer l - 1 is the chained twin's layer l: two routes to the
    same float64 numbers (nn.GroupNorm and the twin's convolution / the helper's statistics and convolution)"""
    sd = PL.PARAM_SETS[pset](3)
    x = PL.images(37, 53, 3, seed=1)
    c = PL.chained64(sd, x)
    for l in range(1, 8):
        a = PL.operand64(l, imgs=x) if l == 1 else PL.operand64(l, raw=c["raw"][l - 2], scsh=c["scsh"][l - 2])
        if l > 1:
            assert float((a - c["act"][l - 2]).abs().max()) <= 1e-12 * max(1.0, float(c["act"][l - 2].abs().max()))
        y, bound = PL.isolated64(sd, l, a)
        assert float((y - c["raw"][l - 1]).abs().max()) <= 1e-12 * float(c["raw"][l - 1].abs().max()), l
        assert float(bound.min()) > 0


@pytest.mark.parametrize("H,W,N", [(17, 33, 5), (100, 333, 1), (192, 640, 2)])
def test_fp32_twin_inside_the_bound_and_a_one_tap_mutant_outside(H, W, N):
    """the bound is neither too tight for a correct fp32 convolution (torch's, on its own fp32 operand) nor vacuous: with one tap of
    one input channel zeroed, the outputs whose operand is not a ReLU zero there leave it"""
    sd = standins.posenet_params(3)
    x = PL.images(H, W, N, seed=2)
    c32 = PL.chained(sd, x, torch.float32)
    for l in range(1, 8):
        if l == 1:
            a = PL.operand64(1, imgs=x)
        else:    # the fp32 twin's operand: its own GroupNorm + ReLU output, taken as given
            a = c32["act"][l - 2].double()
        y, bound = PL.isolated64(sd, l, a)
        ratio = float(((c32["raw"][l - 1].double() - y).abs() / bound).max())
        wm = PL.ws64(sd[f"conv{l}.0.weight"])
        k = wm.shape[-1]
        wm[:, 0, k // 2, k // 2] = 0
        ym, _ = PL.isolated64(sd, l, a, w64=wm)
        touched = (a[:, 0:1, ::2, ::2] != 0)[:, :, :y.shape[2], :y.shape[3]].expand_as(y)      # centre tap of output (oy, ox) reads (2 oy, 2 ox)
        out = ((ym - y).abs() > bound)
        share = float(out[touched].double().mean()) if bool(touched.any()) else float("nan")
        print(f"{H}x{W} layer {l}: fp32 err / bound {ratio:.4f}; mutant outside the bound on {share:.2f} of the outputs it touches")
        assert ratio < 0.25, (l, ratio)              # a correct kernel has room: the bound is a worst case over K roundings
        assert not bool(out[~touched].any())
        assert share > 0.5, (l, share)                 # (0.81 .. 1.00 measured; a tap whose activation is small beside K others stays inside)


def test_selection_table_and_cases_cover_the_missing_splits():
    """every (layer, nb, ks, pb) a case names is what the selection rule gives at that size and N, and together the cases launch
    every split the suite never ran"""
    seen_few, seen_many = set(), set()
    sizes_few, sizes_many = set(), set()
    for H, W, N, M, combos in PL.CASES:
        assert 1 <= N <= M
        tab = PL.selection_table(H, W)
        for (l, nb, ks, pb) in combos:
            assert tab[l - 1]["few" if N <= 4 else "many"] == (nb, ks, pb), (H, W, N, l, tab[l - 1])
        (seen_few if N <= 4 else seen_many).update(combos)
        (sizes_few if N <= 4 else sizes_many).add((H, W))
    assert PL.NEEDED_FEW <= seen_few, PL.NEEDED_FEW - seen_few
    assert PL.NEEDED_MANY <= seen_many, PL.NEEDED_MANY - seen_many
    need = {(5, 9), (17, 33), (37, 53), (64, 64), (100, 333), (128, 416), (192, 640), (240, 320), (256, 448), (320, 1024), (375, 1242), (33, 2050)}
    assert sizes_few == need and sizes_many == need
    assert any(M > N for _, _, N, M, _ in PL.CASES)
    # the sizes the suite ran before reach none of them
    for (H, W), regime in [((48, 160), "few"), ((64, 96), "few"), ((100, 333), "few"), ((192, 640), "few"), ((192, 640), "many"), ((48, 160), "many")]:
        got = {(l + 1,) + r[regime] for l, r in enumerate(PL.selection_table(H, W))}
        assert not got & (PL.NEEDED_FEW if regime == "few" else PL.NEEDED_MANY)
    # geometry at the edges the sizes were chosen for
    assert PL.selection_table(100, 333)[0]["ow"] == 167 and PL.selection_table(375, 1242)[0]["ow"] == 621
    assert (PL.selection_table(33, 2050)[0]["oh"], PL.selection_table(33, 2050)[0]["ow"]) == (17, 1025)


def test_parameter_sets():
    """the offset set puts every group's mean at 3..10 standard deviations, the gamma set has near-zero and negative gammas, and
    neither touches the seeded stream of standins.posenet_params"""
    base = standins.posenet_params(3)
    again = standins.posenet_params(3)
    assert all(np.array_equal(base[k], again[k]) for k in base)
    off, gam = PL.posenet_params_offset(3), PL.posenet_params_gamma(3)
    assert all(np.array_equal(off[k], base[k]) for k in base if not k.endswith(".0.bias"))
    assert all(np.array_equal(gam[k], base[k]) for k in base if not k.endswith(".1.weight"))
    x = PL.images(64, 96, 2, seed=3)
    c = PL.chained64(off, x)
    for l in range(7):
        _, mean, var = PL.gn_scsh64(c["raw"][l], off[f"conv{l + 1}.1.weight"], off[f"conv{l + 1}.1.bias"])
        r = (mean.abs() / var.sqrt())
        print(f"layer {l + 1}: |mean| / std {float(r.min()):.1f} .. {float(r.max()):.1f}")
        assert float(r.min()) > 2.0 and float(r.max()) < 25.0
    g1 = gam["conv3.1.weight"]
    assert np.abs(g1[1::4]).max() < 1e-2 and (g1[2::4] < 0).mean() > 0.9


def test_scsh_tolerance_admits_fp32_group_norm_and_rejects_a_dropped_tile():
    """the derived scale/shift tolerance: torch's fp32 GroupNorm statistics pass; statistics that miss one 64-pixel tile do not"""
    sd = PL.posenet_params_offset(3)
    x = PL.images(100, 333, 2, seed=4)
    c = PL.chained(sd, x, torch.float32)
    for l in (1, 2, 4):
        raw = c["raw"][l - 1]
        gamma, beta = sd[f"conv{l}.1.weight"], sd[f"conv{l}.1.bias"]
        ref, tol = PL.scsh_tolerance(raw, gamma, beta, 64)
        N, Cn = raw.shape[:2]
        g = raw.reshape(N, 16, Cn // 16, -1)
        mean32, var32 = g.mean((2, 3)), g.var((2, 3), unbiased=False)           # fp32 statistics
        sc = (1.0 / torch.sqrt(var32 + 1e-5)).repeat_interleave(Cn // 16, 1) * torch.as_tensor(gamma)
        sh = torch.as_tensor(beta) - mean32.repeat_interleave(Cn // 16, 1) * sc
        got = torch.stack([sc, sh], 2).double()
        assert bool(((got - ref).abs() <= tol).all()), l
        cut = raw.clone().flatten(2)[:, :, 64:].double()                        # the first 64 pixels never reached the sums
        bad = PL.gn_scsh64(cut.unsqueeze(3), gamma, beta)[0]
        assert float(((bad - ref).abs() > tol).double().mean()) > 0.5, l
