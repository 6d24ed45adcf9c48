"""CPU: the cases, the bound and the judge of tests/dense_linearize_exact_inputs.py, before a GPU is asked anything.

  * the module's constants are the kernels' (read from the sources), the additions follow from them, and the export path really never
    splits k_solve_joint's record sum;
  * the oracle's new outputs: every |gradient entry| <= its sum of |contributions|, the replay under the oracle's own decisions returns the
    free-running results, and the decisions it sums under are the ones decisions() states;
  * every case meets its conditions on the float64 oracle alone: mask floors, near-ties, the out-of-bounds share, the out-of-window tap
    share, the depth-consistency share of W_DC_BIG (and W_DC_BIG / 2 misses it), the pairwise coverage of the option set;
  * the float32 oracle under the decisions IT takes passes the judge against float64 under the same decisions, with no hard flip;
  * the judge rejects six planted faults, the float32 twin's outputs standing in for the engine's.  Today's bar (2e-4 of the largest entry
    of g_pose, g_rho, g_rho_src) ACCEPTS two of them, asserted below: the SSIM tap dropped at a sliver-tile pixel and the depth-consistency
    part of one pixel scaled by 1 + 2^-10 -- the single-pixel faults.  It rejects the other four (the out-of-window scatter dropped, the
    prior's gradient taken at depth_t, two pose rows swapped, a source map in the wrong slot): each moves many entries by far more than
    2e-4 of the largest.
"""
import functools
import itertools
import os
import re

import numpy as np
import pytest

import dense_linearize_exact_inputs as DX
import linearize_exact_inputs as LX
import parity_util as PU

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tightly_coupled_sfm_amd", "csrc")
SMALL_IDS = [i for i in DX.IDS if DX.BY_ID[i].H < 100]
BIG_IDS = [i for i in DX.IDS if DX.BY_ID[i].H >= 100]


def test_constants_are_the_kernels():
    api, ker, joint, dref = (open(os.path.join(CSRC, f)).read() for f in ("tcsfm_api.hip", "kernels.h", "joint_kernel.h", "dense_ref_kernel.h"))
    api += open(os.path.join(CSRC, "dense_host.h")).read()          # the dense drivers: part of the API file's translation unit
    lay = open(os.path.join(CSRC, "layout.h")).read()               # the layout constants host arithmetic and kernels share: the joint tile lives there
    assert re.search(r"constexpr int FM = (\d+), WW = TW \+ 2 \* FM, WH = TH \+ 2 \* FM", ker).group(1) == str(DX.FM)
    assert re.search(r"constexpr double DREF_FIX = (\d+)\.0;", ker).group(1) == str(2 ** DX.DREF_FIX_BITS)
    assert "llrint((double)(f_dc * w4[k]) * DREF_FIX)" in ker and "llrint((double)(coef * w4[k]) * DREF_FIX)" in dref
    tw, th = re.search(r"kJointTileW = (\d+)", lay), re.search(r"kJointTileH = (\w+)", lay)
    assert tw and int(tw.group(1)) == DX.JTILE_W and th
    assert re.search(r"#define TC_JOINT_TILE_H (\d+)", lay).group(1) == str(DX.JTILE_H)
    assert "s += (r0 + k * PARTS < r_hi) ? (double)w[k] : 0.0;" in joint                     # k_solve_joint adds the records in double
    assert "for (int w = 0; w < NT / 64; w++) s += red[w * 32 + tid];" in joint              # joint_reduce_add: the wave partials in order
    assert "g_rho -= o_depth * o_depth * (r_dc * Edc - r_eph * Eph);" in joint
    # the export returns before the split of the record sum is configured: nsplit stays 0 (memset) on that path
    assert re.search(r"if \(ex\) return export_once\(\);\n\s+params_solve\(\);", api) and api.count("params_solve()") == 2
    assert re.search(r"void params_solve\(\) \{\n\s+auto split_of = \[\]\(int recs, int ns\)", api) and api.count("nsplit =") == 2
    assert "memset(&Sj, 0, sizeof(Sj));" in api and "const int G = P.nsplit > 1 ? P.nsplit : 1;" in joint
    assert [DX.additions_rho(S) for S in (1, 2, 3, 4)] == [21, 23, 25, 27]
    assert [DX.additions_xi(S) for S in (1, 2, 3, 4)] == [26, 27, 28, 29]
    assert [DX.additions_fwd(S) for S in (1, 2, 3, 4)] == [13, 15, 17, 19]
    A = DX.allowances(DX.CROSSING_CASES[0])
    assert A["xi_inv"] == 28 * 2.0 ** -24 and DX.allowances(DX.SHAPE_CASES[-1])["xi_inv"] == 13 * 2.0 ** -24
    assert LX.n_tiles(208, 640) == 260 > LX.DIRECT_MAX_TILES
    assert len(set(DX.IDS)) == len(DX.CASES)


def test_option_rows_cover_every_pair_of_values():
    rows = DX.option_rows()
    names = list(DX.OPTION_VALUES)
    for a, b in itertools.combinations(names, 2):
        for va in DX.OPTION_VALUES[a]:
            for vb in DX.OPTION_VALUES[b]:
                assert any(r[a] == va and r[b] == vb for r in rows), (a, va, b, vb)
    for H, W in DX.OPTION_SHAPES:        # ... and every row is a case at both ragged shapes (the all-default row is the shape case itself)
        have = {(c.argmin, c.automask, (c.w_l1, c.w_ssim), c.w_dc, c.prior, c.w_smooth, c.w_pc) for c in DX.CASES
                if (c.H, c.W, c.B, c.S, c.kind) == (H, W, 2, 2, "plain")}
        assert {tuple(r[n] for n in names) for r in rows} <= have
    ids = set(DX.IDS)
    assert {"5x9-B1-S2-argmin0-am0-l1_0.15-ssim0.85-dc0.15-prior0.1-smooth0-pc0", "9x40-B1-S1-argmin1-am1-l1_0.15-ssim0.85-dc0.15-prior0.1-smooth2-pc0",
            "16x48-B2-S2-default", "12x36-B1-S3-argmin0-am1-l1_0.15-ssim0.85-dc0.15-prior0.1-smooth0-pc0", "20x36-B2-S4-default", "17x33-B2-S2-default",
            "37x53-B2-S2-default", "208x640-B1-S2-default", "37x53-B1-S2-oob", "37x53-B1-S2-fallback"} <= ids
    d = DX.inputs(DX.BY_ID["37x53-B2-S2-default"])
    assert not np.array_equal(d["depth0"], d["depth_t"]) and not np.array_equal(d["tgt"][0], d["tgt"][1]) and not np.array_equal(d["srcs"][0], d["srcs"][1])


@functools.lru_cache(maxsize=None)
def _refs(c):
    """the float64 oracle's own bits of the case, and both oracles' linearisations under them"""
    bits = DX.own_bits(c)
    return bits, DX.reference(c, "f64", bits), DX.reference(c, "f32", bits)


def _check_case(cid):
    c = DX.BY_ID[cid]
    bits, r64, _ = _refs(c)
    px, SB = c.H * c.W, c.S * c.B
    mask, tie, valid = DX.decisions(c)
    # the oracle's new outputs
    free = DX.reference(c, "f64")
    for k in ("g_rho", "g_xi", "g_rho_s", "loss", "K_f", "K_i"):           # replaying its own decisions changes nothing
        assert np.allclose(r64[k], free[k], rtol=1e-12, atol=0), (cid, k)
    assert np.array_equal(r64["mask"] > 0.5, mask) and np.array_equal((bits & 1) > 0, mask)
    assert r64["K_f"] == mask[:SB].sum() and r64["K_i"] == mask[SB:].sum()
    for g, a in (("g_rho", "g_rho_abs"), ("g_xi", "g_xi_abs"), ("g_rho_s", "g_rho_s_abs")):
        assert np.all(np.abs(r64[g]) <= r64[a] * (1 + 1e-12)), (cid, g)
    assert np.all(r64["g_xi_abs"] > 0) and (r64["g_rho_abs"] > 0).mean() > 0.9
    # mask floor: every judged pair keeps MIN_MASK_FRAC of the frame.  Under the min over the sources the forward pairs of a target SHARE
    # its selection (a pixel goes to one source): the floor then holds for the selection, and every one of the S pairs keeps its S-th part
    frac = mask.reshape(2 * SB, -1).mean(1)
    assert np.all(frac[SB:] >= DX.MIN_MASK_FRAC), (cid, frac)
    if c.argmin and c.S > 1:
        for b in range(c.B):
            idx = [s * c.B + b for s in range(c.S)]
            assert mask[idx].any(0).mean() >= DX.MIN_MASK_FRAC and np.all(frac[idx] >= DX.MIN_MASK_FRAC / c.S), (cid, frac)
    else:
        assert np.all(frac[:SB] >= DX.MIN_MASK_FRAC), (cid, frac)
    assert DX.near_tie_fraction(c) <= DX.MAX_TIE_FRAC, (cid, DX.near_tie_fraction(c))
    if c.w_dc == DX.W_DC_BIG:
        share = DX.dc_share(c, bits)
        assert min(share) >= DX.MIN_DC_PIXELS, (cid, share)
    # the float32 oracle under the decisions it takes itself, judged as the engine is
    b32 = DX.own_bits(c, "f32")
    eng = DX.engine_like(DX.reference(c, "f32", b32), c)
    fails, summ = DX.judge_case(c, eng, b32)
    assert not fails, (cid, fails)
    assert all(ratio in (0.0, 1.0) or abs(ratio - 1) < 1e-9 for ratio, _ in summ.values()), summ
    if c.H < 100:       # (208 x 640: the float32 ORACLE takes 2 of its 532 480 decisions differently from float64 by more than a near-tie -- its SSIM is
        PU.check_flips_every_linearisation(DX.oracle("f64"), 1, 2 * SB * px, cid)      # cancellation-limited; the engine is held to none at every size)


@pytest.mark.parametrize("cid", SMALL_IDS)
def test_case_conditions_and_float32_twin(cid):
    _check_case(cid)


@pytest.mark.parametrize("cid", BIG_IDS)
def test_crossing_case_conditions_and_float32_twin(cid):
    _check_case(cid)


def test_w_dc_big_is_the_smallest_power_of_two():
    """over the option rows that carry it: W_DC_BIG supplies 30 % of g_rho_abs64 on a quarter of the masked pixels of every target of every
    row (asserted per case above), half of it misses that on at least one row"""
    assert np.log2(DX.W_DC_BIG) == int(np.log2(DX.W_DC_BIG))
    big = [c for c in DX.OPTION_CASES if c.w_dc == DX.W_DC_BIG]
    assert len(big) >= 4 and {(c.H, c.W) for c in big} == set(DX.OPTION_SHAPES)
    half = [min(DX.dc_share(c._replace(w_dc=DX.W_DC_BIG / 2), _refs(c)[0])) for c in big]
    assert min(half) < DX.MIN_DC_PIXELS, half


def test_out_of_bounds_and_fallback_conditions():
    c = DX.OOB_CASE
    valid = DX.decisions(c)[2]
    assert np.all(valid.reshape(len(valid), -1).mean(1) <= 1 - DX.OOB_MIN_FRAC), valid.reshape(len(valid), -1).mean(1)
    r64 = _refs(c)[1]
    assert (r64["n_taps"] == 0).any() and (r64["n_taps"] > 0).any()            # pixels no inverse sample reaches, beside pixels some do
    c = DX.FALLBACK_CASE
    share, n = DX.window_share(c)
    mask = DX.decisions(c)[0]
    assert share >= DX.FALLBACK_MIN_SHARE and n > 0, share
    assert np.all(mask.reshape(len(mask), -1).mean(1) >= DX.FALLBACK_MIN_MASK)
    # (the floor is a few centimetres below the camera: the scaled motion of two other cases sends taps past the window too -- 16x48 default
    # 11.6 %, the out-of-bounds case 20.8 % -- the remaining shape cases none: the case made for it does not stand alone)
    assert DX.window_share(DX.case(17, 33, 2, 2))[1] == 0 and DX.window_share(DX.case(16, 48, 2, 2))[1] > 0


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
# (under the min over the sources source 0's weight map multiplies every selected pixel, and it is zero where source 0 -- moving forward --
# samples outside its frame: the border pixels of an argmin case carry no photometric gradient at all.  The sliver fault needs a row without it.)
SLIVER = [c for c in DX.OPTION_CASES if (c.H, c.W) == (17, 33) and not c.argmin and c.w_ssim > 0][0]
BIG_DC = [c for c in DX.OPTION_CASES if (c.H, c.W) == (37, 53) and c.w_dc == DX.W_DC_BIG and c.prior > 0][0]
PRIOR = DX.case(37, 53, 2, 2)


def _verdict(c, eng):
    bits, r64, r32 = _refs(c)
    fails = DX.judge(c, eng, r64, r32, bits)[0]
    return {f.split(":")[0] for f in fails}, DX.todays_bar(eng, r64)


def _twin(c):
    return DX.engine_like(_refs(c)[2], c)


def test_honest_twin_passes_both():
    for c in (SLIVER, BIG_DC, PRIOR, DX.FALLBACK_CASE, DX.OOB_CASE):
        assert _verdict(c, _twin(c)) == (set(), True)


def test_fault_1_ssim_tap_dropped_at_a_sliver_tile_pixel():
    """column 32 of 17 x 33 is a one-pixel sliver of both tile grids: what pixel (0, 32) receives from the SSIM window centred on (0, 31) --
    a pixel of ANOTHER tile -- comes through the tile halo.  That one tap dropped (forward pair (1, 0), all three channels)."""
    c = SLIVER
    bits = _refs(c)[0]
    m, (cy, cx), dst = 2, (0, 31), (0, 32)
    assert bits[m, cy, cx] & 1 and cx // DX.JTILE_W != dst[1] // DX.JTILE_W and cx // DX.FTILE_W != dst[1] // DX.FTILE_W and c.W - 1 == dst[1]
    eng = DX.engine_like(DX.reference(c, "f32", bits, fault_tap=(m, cy * c.W + cx, (dst[0] - cy + 1) * 3 + (dst[1] - cx + 1))), c)
    moved = np.argwhere(eng["g_rho"] != _twin(c)["g_rho"])
    assert moved.tolist() == [[m % c.B, dst[0], dst[1]]]                      # that one pixel of one target, nothing else in the map
    got, bar = _verdict(c, eng)
    assert "rho" in got and bar, (got, bar)                                   # today's bar accepts it


def test_fault_2_scatter_dropped_outside_the_lds_window():
    c = DX.FALLBACK_CASE
    bits = _refs(c)[0]
    eng = DX.engine_like(DX.reference(c, "f32", bits, fault_scatter=DX.outside_window_taps(c)), c)
    got, bar = _verdict(c, eng)
    assert "rho" in got, got
    assert not bar                                                            # (a tenth of the scattered adjoint: today's bar sees that one)


def test_fault_3_depth_consistency_part_of_one_pixel_scaled():
    """the pixel on which the depth-consistency part is the largest share of g_rho_abs64, among those small enough for today's bar"""
    c = BIG_DC
    bits, r64, r32 = _refs(c)
    part = r32["g_rho"] - DX.reference(c, "f32", bits, opts=DX.oracle_opts(c, w_dc=0.0))["g_rho"]      # (w_dc is part of no decision)
    share = np.abs(part) / r64["g_rho_abs"]
    share[np.abs(part) * 2.0 ** -10 >= 1e-4 * np.abs(r64["g_rho"]).max()] = 0
    p = np.unravel_index(np.argmax(share), share.shape)
    assert share[p] > 0.5
    eng = _twin(c)
    eng["g_rho"][p] += 2.0 ** -10 * part[p]
    got, bar = _verdict(c, eng)
    assert got == {"rho"} and bar, (got, bar, share[p])


def test_fault_4_prior_taken_at_depth_t():
    c = PRIOR
    bits = _refs(c)[0]
    eng = DX.engine_like(DX.reference(c, "f32", bits, depth0=DX.inputs(c)["depth_t"]), c)
    got, bar = _verdict(c, eng)
    assert {"rho", "fwd"} <= got and not bar, (got, bar)


def test_fault_5_pose_rows_swapped():
    c = PRIOR
    eng = _twin(c)
    SB = c.S * c.B
    eng["g_pose"][[1, SB + 1]] = eng["g_pose"][[SB + 1, 1]]
    got, bar = _verdict(c, eng)
    assert got == {"xi_fwd", "xi_inv"} and not bar, (got, bar)


def test_fault_6_source_map_written_to_the_wrong_slot():
    c = PRIOR
    eng = _twin(c)
    eng["g_rho_src"][0] = eng["g_rho_src"][1]
    got, bar = _verdict(c, eng)
    assert got == {"rho_s"} and not bar, (got, bar)


def test_zero_rule_and_counts():
    c = DX.OOB_CASE
    bits, r64, r32 = _refs(c)
    dead = np.argwhere(r64["g_rho_s_abs"] == 0)
    assert len(dead) > 0                                                      # source pixels nothing reaches
    eng = _twin(c)
    eng["g_rho_src"][tuple(dead[0])] = 1e-12
    assert any(f.startswith("rho_s: 1 pixels") for f in DX.judge(c, eng, r64, r32, bits)[0])
    eng = _twin(c)
    eng["K_i"] += 1
    assert _verdict(c, eng)[0] == {"K_i"}


def test_report_line(tmp_path, monkeypatch):
    f = tmp_path / "report.tsv"
    monkeypatch.setenv("TCSFM_TEST_DENSE_LIN_EXACT_REPORT", str(f))
    c = PRIOR
    bits = _refs(c)[0]
    fails, summ = DX.judge_case(c, _twin(c), bits)
    assert not fails and set(summ) == set(DX.MEASURES)
    line = f.read_text().strip().split("\t")
    assert line[0] == DX.case_id(c) and len(line) == 1 + 2 * len(DX.MEASURES) + 2
