"""Shared by the depth evaluation tests: a NumPy float64 restatement of the reference's per-frame Eigen evaluation
(paper_plots_and_data/evaluate_depth_eigen.py:133-168) and the test cases.  It is the contract k_depth_eval is held to.

evaluate_frame follows the reference line by line: resize the disparity plane to the ground truth's size, depth_unit / disp, mask and
crop, median scaling, clip, compute_errors.  Two things are stated here rather than taken from the reference:
  * the resize.  The reference calls cv2.resize (bilinear); OpenCV is not available where the golden vectors are made, so `resize` below
    restates INTER_LINEAR's generic path -- half-pixel centres, float32 coefficients, edges clamped, horizontal pass first -- in float64
    with every operation rounded on its own.  Bit-equality with cv2.resize is NOT claimed; the exact-2x shrink, where OpenCV switches to
    area averaging, is not special-cased.
  * log(gt) is a float64 log (the reference's gt is float32 and np.log(gt) a float32 log): the one deliberate deviation.
Everything from the mask to compute_errors is pinned to the reference's own lines by tests/test_depth_eval_inputs_cpu.py
(golden/golden_depth_eval.npz).  A float32 plane is promoted to float64 first (exact); from there on there is one arithmetic path."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EIGEN, EIGEN_BENCHMARK = 0, 1
NEVAL = 10
ABS_REL, SQ_REL, RMSE, RMSE_LOG, A1, A2, A3, RATIO, N_VALID, N_MEDIAN = range(NEVAL)
EXACT = (A1, A2, A3, RATIO, N_VALID, N_MEDIAN)
SUMMED = (ABS_REL, SQ_REL, RMSE, RMSE_LOG)
MIN_DISP, MAX_DISP = 1 / 2.67, 1 / 0.06          # disp_to_depth's scaled_disp at the reference's depth bounds (make_golden_disp_post.py)


def axis_coeffs(n_src, n_dst):
    """one axis of the bilinear resize -> (s, s1 int tap indices [n_dst], w0, w1 float32 weights [n_dst])"""
    scale = 1.0 / (n_dst / n_src)
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)         # computed in double, rounded once
    s = np.floor(f)
    f = (f - s.astype(np.float32)).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= n_src - 1
    s = np.where(low, 0, np.where(high, n_src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    w0 = (np.float32(1) - f).astype(np.float32)
    return s, np.minimum(s + 1, n_src - 1), w0, f


def resize(plane, gt_h, gt_w):
    """plane [H,W] float64 -> [gt_h,gt_w] float64: two multiplications and one addition per pass, each rounded on its own"""
    P = np.asarray(plane, dtype=np.float64)
    sx, sx1, w0, w1 = axis_coeffs(P.shape[1], gt_w)
    sy, sy1, b0, b1 = axis_coeffs(P.shape[0], gt_h)
    R = P[:, sx] * w0.astype(np.float64) + P[:, sx1] * w1.astype(np.float64)
    return R[sy] * b0.astype(np.float64)[:, None] + R[sy1] * b1.astype(np.float64)[:, None]


def crop(protocol, gt_h, gt_w):
    """(y0, y1, x0, x1) of the pixels the protocol looks at: the Eigen crop, or the whole plane"""
    if protocol == EIGEN_BENCHMARK:
        return 0, gt_h, 0, gt_w
    c = np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)
    return tuple(int(v) for v in c)


def median(a):
    """np.median of a 1-D array by selection: the middle element, or the mean of the two middle ones in the array's own dtype"""
    a = np.sort(np.asarray(a))
    n = a.size
    if n == 0:
        return a.dtype.type(np.nan)
    if n % 2:
        return a[n // 2]
    return (a[n // 2 - 1] + a[n // 2]) / a.dtype.type(2)


def mask_of(gt, protocol, min_depth, max_depth):
    gt = np.asarray(gt)
    assert gt.dtype == np.float32
    if protocol == EIGEN_BENCHMARK:
        return gt > np.float32(0)
    y0, y1, x0, x1 = crop(protocol, *gt.shape)
    m = np.zeros(gt.shape, bool)
    m[y0:y1, x0:x1] = True
    return m & (gt > np.float32(min_depth)) & (gt < np.float32(max_depth))


def compute_errors(g, pred):
    """the reference's compute_errors on float64 vectors (g = float64(gt))"""
    thresh = np.maximum(g / pred, pred / g)
    a1, a2, a3 = (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(), (thresh < 1.25 ** 3).mean()
    d = g - pred
    rmse = np.sqrt((d ** 2).mean())
    rmse_log = np.sqrt(((np.log(g) - np.log(pred)) ** 2).mean())
    return np.mean(np.abs(d) / g), np.mean((d ** 2) / g), rmse, rmse_log, a1, a2, a3


def evaluate_masked(gt_m, pred_m, median_scaling=True, min_depth=1e-3, max_depth=80.0):
    """reference lines 158-168 on the masked vectors gt_m float32, pred_m float64 -> the NEVAL doubles"""
    out = np.full(NEVAL, np.nan)
    out[N_VALID] = gt_m.size
    sub = gt_m < np.float32(max_depth)
    out[N_MEDIAN] = int(sub.sum())
    out[RATIO] = 1.0
    if median_scaling:
        out[RATIO] = np.float64(median(gt_m[sub])) / median(pred_m[sub]) if sub.any() else np.nan
    if gt_m.size == 0 or np.isnan(out[RATIO]):
        return out
    lo, hi = np.float64(np.float32(min_depth)), np.float64(np.float32(max_depth))
    pred = pred_m * out[RATIO] if median_scaling else pred_m.copy()
    pred = np.minimum(np.maximum(pred, 0.0), hi)
    pred[pred < lo] = lo
    pred[pred > hi] = hi
    out[:7] = compute_errors(gt_m.astype(np.float64), pred)
    return out


def evaluate_frame(plane, gt, protocol=EIGEN, median_scaling=True, min_depth=1e-3, max_depth=80.0, depth_unit=30.0, do_resize=True):
    """plane [H,W] float32 or float64, gt [gt_h,gt_w] float32 -> float64 [NEVAL].  do_resize=False: the plane is taken as it is (it
    must have the ground truth's size)"""
    gt = np.asarray(gt)
    P = np.asarray(plane).astype(np.float64)
    out = resize(P, *gt.shape) if do_resize else P
    assert out.shape == gt.shape
    pred = np.float64(depth_unit) / out
    m = mask_of(gt, protocol, min_depth, max_depth)
    return evaluate_masked(gt[m], pred[m], median_scaling, min_depth, max_depth)


def evaluate(planes, gts, **kw):
    return np.stack([evaluate_frame(p, g, **kw) for p, g in zip(planes, gts)])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def summed_bound(n_valid):
    """relative bound on a summed metric: two double sums of n_valid non-negative terms in different orders"""
    return max(float(n_valid), 1.0) * 2.0 ** -50


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  Disparities are uniform in [MIN_DISP, MAX_DISP], so a prediction lies in depth_unit * [0.06, 2.67]: a spread of 44.5.  With
# the default bounds (1e-3, 80: a spread of 80 000) a median-scaled frame can therefore clip at ONE end only; the default-bound cases
# draw the ground truth around 10 x the predictions so that the upper clip fires, and the case with its own bounds (0.8, 4) clips at both.
def disparity(h, w, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return rng.uniform(MIN_DISP, MAX_DISP, size=(h, w)).astype(dtype)


def ground_truth(plane, gt_h, gt_w, seed, valid=0.3, gain=10.0, spread=4.0, far=0.0, depth_unit=30.0):
    """float32 [gt_h,gt_w]: gain * prediction * log-uniform noise in [1/spread, spread] on a fraction `valid` of the pixels, 0 (a hole)
    elsewhere; a fraction `far` of the valid ones is moved to [80, 120) (beyond max_depth)"""
    rng = np.random.default_rng(seed)
    pred = depth_unit / resize(np.asarray(plane, np.float64), gt_h, gt_w)
    g = gain * pred * np.exp(rng.uniform(-np.log(spread), np.log(spread), size=pred.shape))
    g = np.where(rng.uniform(size=pred.shape) < far, rng.uniform(80.0, 120.0, size=pred.shape), g)
    g = np.where(rng.uniform(size=pred.shape) < valid, g, 0.0)
    return g.astype(np.float32)


def clip_census(plane, gt, protocol=EIGEN, median_scaling=True, min_depth=1e-3, max_depth=80.0, depth_unit=30.0):
    """(predictions clipped at min_depth, at max_depth) of one frame"""
    r = evaluate_frame(plane, gt, protocol, median_scaling, min_depth, max_depth, depth_unit)
    m = mask_of(gt, protocol, min_depth, max_depth)
    pred = (depth_unit / resize(np.asarray(plane).astype(np.float64), *gt.shape))[m] * (r[RATIO] if median_scaling else 1.0)
    return int((pred < np.float64(np.float32(min_depth))).sum()), int((pred > np.float64(np.float32(max_depth))).sum())


def toggle_one(gt, protocol=EIGEN, min_depth=1e-3, max_depth=80.0):
    """gt with its first masked pixel turned into a hole: the masked count changes parity"""
    g = gt.copy()
    m = mask_of(g, protocol, min_depth, max_depth)
    y, x = np.argwhere(m)[0]
    g[y, x] = 0
    return g


@functools.lru_cache(maxsize=None)
def base_case(odd=True):
    """disparity 6 x 20 -> ground truth 11 x 37, about 30 % valid with holes; the median subset's count is odd (or, one pixel
    toggled, even)"""
    P = disparity(6, 20, seed=3)
    gt = ground_truth(P, 11, 37, seed=4, valid=0.45)
    n = int(mask_of(gt, EIGEN, 1e-3, 80.0).sum())
    if (n % 2 == 1) != odd:
        gt = toggle_one(gt)
    return P, gt


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(HERE, "golden", "golden_depth_eval.npz"))
    return {k: g[k] for k in g.files}
