"""The inputs, the float64 reference and the judge of the photometric-gradient tests (tests/photo_grad_inputs.py), checked without a
GPU: the masks stay under the warp tests' cap and the float32 twin takes the float64 decisions off them, the restated assembly is
torch_twin.photometric's, the numpy statement of the kernel's formulas (reflect multiplicity included) is the float64 autograd
gradient, and the judge rejects six planted faults on the tensors they touch."""
import numpy as np
import pytest

import photo_grad_inputs as PG

torch = pytest.importorskip("torch")
WG = PG.WG


@pytest.mark.parametrize("mode", ("maps", "chain"))
@pytest.mark.parametrize("case", PG.CASES, ids=PG.IDS)
def test_masks_under_the_cap_and_float32_decides_alike(case, mode):
    """per item the union of the masks (photo ties, float32 disagreements, and for the chain the warp's tie mask on valid pixels) is at
    most mask_cap(H W); the float32 twin decides otherwise than float64 at a handful of pixels at the most, all of them masked; the
    cotangents vanish on the mask and differ in scale between items and maps"""
    H, W, N, s = case
    ties, flips, cell = PG.photo_tie_mask(case, mode)
    union = ties | flips | cell
    if mode == "chain":
        near, g = WG.tie_mask(case)
        union = union | (near & g["valid"])
    print(case, mode, "photo ties", ties.sum(1).tolist(), "float32 decides otherwise", flips.sum(1).tolist(), "cell flips", cell.sum(1).tolist(),
          "union", union.sum(1).tolist(), "cap", PG.mask_cap(H * W))
    assert (union.sum(1) <= PG.mask_cap(H * W)).all(), (case, mode, union.sum(1), PG.mask_cap(H * W))
    assert (flips.sum(1) <= max(2, PG.mask_cap(H * W) // 8)).all(), (case, mode, flips.sum(1))
    zero, cot = PG.mask(case, mode), PG.cotangents(case, mode)
    for k, g in cot.items():
        assert not g[np.broadcast_to(zero[k].reshape(N, 1, H, W), g.shape)].any()
        assert (ties | flips)[~zero[k]].sum() == 0
    lg = np.log10([[np.sqrt((cot[k][n].astype(np.float64) ** 2).mean()) for n in range(N)] for k in cot])
    for n in range(N):
        assert min(abs(lg[a, n] - lg[b, n]) for a in range(len(cot)) for b in range(a)) > 0.4, lg
        assert n == 0 or (np.abs(lg[:, n] - lg[:, n - 1]) > 0.4).all(), lg


def test_kinks_occur_in_the_inputs():
    """the conventions are exercised: pixels at |rec - tgt| = 1 exactly and at |r| = 1 exactly (pd = 0 out of frame) carry cotangents"""
    for case in [c for c in PG.CASES if c[3] == 30.0]:
        H, W, N, _ = case
        l, cot = PG.leaves(case), PG.cotangents(case, "maps")
        one = (np.abs(l["rec"].astype(np.float64) - l["tgt"]) == 1).any(1, keepdims=True)
        assert (one & (cot["g_diff"] != 0)).sum() > 0, case
        assert ((l["pd"] == 0) & (cot["g_weight"] != 0)).sum() > 0.5 * N * H * W, case


def test_assembly_is_the_twins():
    case = (17, 33, 3, 1.0)
    c = PG.make_case(*case)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    r = PG.tw.photometric(T(c["tgt"]), T(c["src"]), T(c["depth_t"]), T(c["depth_s"]), T(c["pose"]), T(c["K"]))
    diff, weight = PG.assembly(T(c["tgt"]), r["rec"], r["proj_depth"], r["comp_depth"])
    assert torch.equal(diff, r["diff"]) and torch.equal(weight, r["weight"])
    assert torch.equal(PG.ssim_raw(T(c["tgt"]), r["rec"]).clamp(0, 1), PG.tw.ssim(T(c["tgt"]), r["rec"]))


FORMULA_CASES = [(5, 9, 3, 1.0), (5, 9, 3, 30.0), (17, 33, 3, 30.0), (37, 53, 3, 1.0)]


@pytest.mark.parametrize("case", FORMULA_CASES, ids=[PG.IDS[PG.CASES.index(c)] for c in FORMULA_CASES])
def test_formulas_are_the_autograd_gradient(case):
    """L1 part + SSIM part (scatter over the reflected taps) == float64 autograd's g_rec to rounding; with the multiplicity taken as 1
    the border pixels differ"""
    ref, cot = PG.twin_maps(case), PG.cotangents(case, "maps")
    got = PG.l1_part(case, cot["g_diff"]) + PG.ssim_part(case, cot["g_diff"])
    for n in range(case[2]):
        l2, _ = WG.errors(got[n], ref["g_rec"][n])
        print(case, n, "formula vs autograd rel_l2", l2)
        assert l2 < 1e-11, (case, n, l2)
    assert not np.allclose(PG.ssim_part(case, cot["g_diff"], multiplicity=False), PG.ssim_part(case, cot["g_diff"]), rtol=1e-6, atol=0)


def test_float32_twin_passes_the_judge_and_float64_is_exact():
    """(g_cd is left out of the float32 twin's own pass: where pd = 0 float64 autograd's 1 / cd - cd / cd^2 rounds to an exact zero that
    float32 autograd misses by an ulp of 1 / cd -- at poses x30 that residue is most of its g_cd error.  The closed form -k pd is exactly
    zero there.)"""
    case = (37, 53, 3, 30.0)
    ref, t32 = PG.twin_maps(case), PG.twin_maps(case, PG.MAP_COTS, "f32")
    fails, worst = PG.judge(t32, ref, t32, "f32", ("g_rec", "g_pd"))
    assert not fails and all(v[0] <= 1.0 for v in worst.values()), (fails, worst)
    assert not PG.judge(ref, ref, t32, "f64", PG.MAP_TENSORS)[0]
    ref, t32 = PG.twin_chain(case), PG.twin_chain(case, PG.CHAIN_COTS, "f32")
    fails, worst = PG.judge(t32, ref, t32, "f32", PG.CHAIN_TENSORS, rel_l2_max=None)
    assert all(f[1] == "d_depth_t" and f[3] == "exact zero" for f in fails), fails        # the same residue, passed on through comp_depth


FAULT_CASES = [(5, 9, 3, 30.0), (17, 33, 3, 30.0), (37, 53, 3, 30.0)]


@pytest.mark.parametrize("case", FAULT_CASES, ids=[PG.IDS[PG.CASES.index(c)] for c in FAULT_CASES])
def test_judge_rejects_planted_faults(case):
    """each fault, planted at numpy level into the true float64 gradient of the maps, fails the judge on the tensors it touches and
    on no other tensor"""
    ref, t32 = PG.twin_maps(case), PG.twin_maps(case, PG.MAP_COTS, "f32")
    faults = PG.planted_faults(case)
    assert set(faults) == {"multiplicity_one", "weights_swapped", "channel_mean_dropped", "g_pd_sign", "no_gradient_at_one", "item0_cotangents_for_all"}
    for name, (faulty, tensors) in faults.items():
        fails, _ = PG.judge(faulty, ref, t32, name, PG.MAP_TENSORS)
        hit = {f[1] for f in fails}
        assert hit == set(tensors), (case, name, hit, tensors)
