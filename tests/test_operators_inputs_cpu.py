"""The inputs of tests/test_gpu_operators.py, checked without a GPU (tests/operator_inputs.py builds them for both modules):

  * the oracle's fp32 build against its float64 build stays inside the decision-pixel cap on every case -- an input on which fp32
    arithmetic alone breaks the cap is a bad input, whatever the kernels do with it;
  * every item of a batch differs from every other in images, both depth maps, intrinsics and pose;
  * every crafted median case has the count, parity, tie and byte structure its name claims (on the fp32 oracle's heights);
  * the numpy lower median agrees with torch.median on those arrays, the padded ones included.
"""
import numpy as np
import pytest

import operator_inputs as OI

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", OI.PAIR_CASES, ids=OI.PAIR_IDS)
def test_pair_inputs_keep_fp32_inside_the_decision_cap(case, oracle32, oracle64):
    H, W, N, s = case
    c = OI.make_case(H, W, N, s)
    assert OI.items_differ(c)
    shares = []
    for n in range(N):
        tag = (OI.PAIR_IDS[OI.PAIR_CASES.index(case)], n)
        OI.judge_warp(OI.oracle_warp(oracle32, c, n), OI.oracle_warp(oracle64, c, n), tag)
        for wl, ws in OI.PHOTO_WEIGHTS:
            OI.judge_photometric(OI.oracle_photometric(oracle32, c, n, wl, ws), OI.oracle_photometric(oracle64, c, n, wl, ws), tag)
        shares.append(float(OI.oracle_warp(oracle64, c, n)["valid"].mean()))
    # the scaled poses are there to push most samples out of the frame, the true ones to keep most inside
    print("valid share", shares)
    assert (max(shares) < 0.5) if s > 1 else (min(shares) > 0.4), shares


@pytest.mark.parametrize("H,W,N", OI.SHAPES + [OI.MANY], ids=lambda v: str(v))
def test_ground_inputs_keep_fp32_inside_the_decision_cap(H, W, N, oracle32, oracle64):
    depth, K = OI.make_ground(H, W, N)
    assert all(not np.array_equal(depth[i], depth[j]) and not np.array_equal(K[i], K[j]) for i in range(N) for j in range(i))
    ground = 0
    for n in range(N):
        h32, m32 = oracle32.ground_height(depth[n, 0], K[n])
        h64, m64 = oracle64.ground_height(depth[n, 0], K[n])
        OI.judge_ground(h32, m32, h64, m64, (H, W, n))
        ground += int(m64.sum())
    assert ground > 0, "a case without any ground tests no height"


def test_median_cases_have_the_structure_their_names_claim(oracle32, oracle64):
    cases = OI.median_cases(oracle32, oracle64)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    counts, parities, pads = set(), set(), set()
    for name, depth, K, pad, expect in cases:
        N = depth.shape[0]
        hm = [oracle32.ground_height(depth[n, 0], K[n]) for n in range(N)]
        heights, masks = np.stack([h for h, _ in hm]), np.stack([m for _, m in hm])
        med, count = OI.check_median_structure(name, heights, masks, pad, expect)
        # the numpy lower median is torch.median, on the padded array too
        _, _, v = OI.lower_median(heights, masks, pad)
        if count:
            assert np.float32(torch.median(torch.tensor(v))).tobytes() == np.float32(med).tobytes(), name
            assert count == v.size
        else:
            assert np.isnan(med), name
        counts.add(count); parities.add(count % 2)
        pads.add(0 if pad == 0 else (pad - N, N))
    assert {0, 1, 2} <= counts and parities == {0, 1}
    assert {(1, 3), (6, 3)} <= pads, pads              # pad_to_batch = N + 1 and 3 N


def test_smooth_inputs_have_a_different_mean_per_item():
    for H, W, N in OI.SHAPES + [OI.MANY]:
        disp, _ = OI.make_smooth(H, W, N)
        means = disp.reshape(N, -1).mean(1)
        assert np.all(np.diff(means) > 0.1 * means[0]), means


def test_ssim_planes_and_disparities_hold_the_edge_values():
    for H, W in OI.SSIM_SHAPES:
        x, y = OI.make_ssim_planes(H, W)
        assert np.ptp(x[1, 1]) == 0 and np.ptp(y[1, 1]) == 0 and np.ptp(x[1, 2]) == 0
        assert set(np.unique(x[2, 0])) == {0.0, 1.0} and set(np.unique(y[2, 0])) == {0.0, 1.0}
    d = OI.make_disp()
    assert d.size > 65535 * 256 and (d == 0).any() and (d == 1).any() and d[-1] == 1.0
