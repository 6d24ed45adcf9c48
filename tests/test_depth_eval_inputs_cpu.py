"""The float64 twin of the depth evaluation (tests/depth_eval_inputs.py) against the reference's own lines.

golden_depth_eval.npz holds what paper_plots_and_data/evaluate_depth_eigen.py:143-166 and its compute_errors return on already-resized
inputs (tests/golden/make_golden_depth_eval.py).  The twin's evaluate_masked must reproduce
  * a1, a2, a3, ratio and the two counts EXACTLY: counts over correctly rounded comparisons, and np.median itself;
  * abs_rel, sq_rel, rmse within n_valid * 2^-50 relative: both sides are double sums of non-negative terms in different orders (the
    reference sums float64 terms too: float32 gt against float64 predictions promotes);
  * rmse_log within 1e-6 absolute: the reference's log(gt) is a float32 log, off by at most about 2 ulp of a float32 in [4, 8)
    (2 * 2^-21 = 9.5e-7) per term, and perturbing every term of an RMS by at most e moves the RMS by at most e.
These bounds are derived, not measured."""
import numpy as np
import pytest

import depth_eval_inputs as D

SIZES = [(375, 1242), (370, 1226), (376, 1241), (11, 37), (33, 70), (5, 9), (6, 20), (1, 37), (11, 1), (9, 9)]


@pytest.mark.parametrize("k", range(4))
def test_twin_matches_the_reference(k):
    g = D.golden()
    assert int(g["n_cases"]) == 4
    gt, pred, bench = g[f"gt{k}"], g[f"pred{k}"], int(g[f"bench{k}"])
    assert gt.dtype == np.float32 and pred.dtype == np.float64
    m = D.mask_of(gt, bench, 1e-3, 80.0)
    got = D.evaluate_masked(gt[m], pred[m])
    want = g[f"errors{k}"]
    n_valid = int(g[f"n_valid{k}"])
    assert got[D.N_VALID] == n_valid and got[D.N_MEDIAN] == int(g[f"n_median{k}"])
    assert got[D.RATIO] == float(g[f"ratio{k}"])
    for j in (D.A1, D.A2, D.A3):
        assert got[j] == want[j], (j, got[j], want[j])
    for j in (D.ABS_REL, D.SQ_REL, D.RMSE):
        assert abs(got[j] - want[j]) <= D.summed_bound(n_valid) * abs(want[j]), (j, got[j], want[j])
    assert abs(got[D.RMSE_LOG] - want[D.RMSE_LOG]) <= 1e-6, (got[D.RMSE_LOG], want[D.RMSE_LOG])
    # the golden cases exercise what they are there for: thresholds in order, and a clipped prediction
    assert 0 < got[D.A1] < got[D.A2] < got[D.A3] < 1
    assert (pred[m] * got[D.RATIO] > 80.0).any()
    # the whole frame through evaluate_frame without its resize: the same numbers
    disp = 30 / pred
    assert np.array_equal(30 / disp, pred)
    assert D.same_bits(D.evaluate_frame(disp, gt, bench, do_resize=False), got)
    if bench == D.EIGEN_BENCHMARK:
        assert got[D.N_MEDIAN] <= got[D.N_VALID]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crop_integers(size):
    gt_h, gt_w = size
    want = np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)
    got = D.crop(D.EIGEN, gt_h, gt_w)
    assert list(got) == [int(v) for v in want]
    assert 0 <= got[0] <= got[1] <= gt_h and 0 <= got[2] <= got[3] <= gt_w
    assert D.crop(D.EIGEN_BENCHMARK, gt_h, gt_w) == (0, gt_h, 0, gt_w)
    if size == (375, 1242):
        assert got == (153, 371, 44, 1197)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 101, 102])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_median_is_np_median(n, dtype):
    rng = np.random.default_rng(n)
    a = rng.uniform(1e-3, 80.0, size=n).astype(dtype)
    if n >= 4:
        a[1] = a[0]                                              # a tie
    got, want = D.median(a), np.median(a)
    assert got.dtype == want.dtype == dtype
    assert got == want
    if n == 2:
        assert got == (a[0] + a[1]) / dtype(2)


def test_resize_identity_and_clamps():
    P = D.disparity(6, 20, seed=1)
    assert D.same_bits(D.resize(P, 6, 20), P)
    # one row, one column: every tap is clamped onto it
    row = D.disparity(1, 20, seed=2)
    out = D.resize(row, 5, 20)
    assert all(D.same_bits(out[y:y + 1], row) for y in range(5))
    col = D.disparity(6, 1, seed=3)
    out = D.resize(col, 6, 4)
    assert all(D.same_bits(out[:, x:x + 1], col) for x in range(4))
    # an enlargement stays inside the plane's range (a convex combination up to rounding) and keeps a constant plane constant
    up = D.resize(P, 11, 37)
    assert up.shape == (11, 37) and up.min() >= P.min() * (1 - 1e-15) and up.max() <= P.max() * (1 + 1e-15)
    s, s1, w0, w1 = D.axis_coeffs(20, 37)
    assert w0.dtype == np.float32 and w1.dtype == np.float32 and s.min() == 0 and s1.max() == 19
    assert s[0] == 0 and w1[0] == 0 and s[-1] == 19 and w1[-1] == 0       # both edges clamp


def test_special_rows():
    P, gt = D.base_case(True)
    empty = np.zeros_like(gt)
    r = D.evaluate_frame(P, empty)
    assert np.isnan(r[:8]).all() and r[D.N_VALID] == 0 and r[D.N_MEDIAN] == 0
    r = D.evaluate_frame(P, empty, median_scaling=False)
    assert np.isnan(r[:7]).all() and r[D.RATIO] == 1.0 and r[D.N_VALID] == 0
    far = np.full_like(gt, 90.0)                                 # benchmark: every pixel valid, none below max_depth
    r = D.evaluate_frame(P, far, D.EIGEN_BENCHMARK)
    assert np.isnan(r[:8]).all() and r[D.N_VALID] == gt.size and r[D.N_MEDIAN] == 0
    r = D.evaluate_frame(P, far, D.EIGEN_BENCHMARK, median_scaling=False)
    assert np.isfinite(r).all() and r[D.RATIO] == 1.0


def test_base_cases_are_what_they_claim():
    for odd in (True, False):
        P, gt = D.base_case(odd)
        r = D.evaluate_frame(P, gt)
        assert (int(r[D.N_MEDIAN]) % 2 == 1) == odd and r[D.N_VALID] >= 20
        assert 0 < r[D.A1] < r[D.A2] < r[D.A3] < 1
        assert D.clip_census(P, gt)[1] > 0
        assert (gt == 0).any()
