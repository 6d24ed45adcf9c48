"""tcsfm_depth_eval / tcsfm_sequence_depth_eval on the GPU against the float64 twin of tests/depth_eval_inputs.py (pinned to the
reference's own lines by tests/test_depth_eval_inputs_cpu.py).

Pass criteria: ratio, a1, a2, a3 and the two counts EXACTLY equal to the twin -- every operation up to the comparisons is a correctly
rounded IEEE operation in a prescribed order --; abs_rel, sq_rel, rmse, rmse_log within n_valid * 2^-50 relative: two double sums of
non-negative terms in different orders, plus a double log of a few ulp.  "Bit for bit" comparisons are int64 views.

Shapes are the smallest at which the kernel can still go wrong.  Two notes on the cases:
  * the disparities lie in [1/2.67, 1/0.06], so the predictions of a frame span a factor 44.5; between the default bounds (1e-3, 80:
    a factor 80 000) a median-scaled frame can clip at one end only.  The default-bound cases are drawn so that the upper clip fires
    (asserted with the twin), the case with its own bounds (0.8, 4) clips at both ends (asserted).
  * a handle's planes have at least four rows and columns (tcsfm_create), so a one-row or one-column DISPARITY plane does not exist at
    this interface: the one-row and one-column case runs on such GROUND TRUTH, and on the narrowest planes a handle takes (4 rows, 4
    columns).  Both clamps of the resize (s < 0, s >= n_src - 1) fire at the edges of every enlargement below."""
import ctypes as C

import numpy as np
import pytest

import depth_eval_inputs as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG = -1
SENTINEL = -7.5
_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(h, w):
    from tightly_coupled_sfm_amd.engine import Engine
    if (h, w) not in _ENGINES:
        _ENGINES[(h, w)] = Engine(h, w, 1)
    return _ENGINES[(h, w)]


def _run(planes, gts, **kw):
    """Engine.depth_eval on NumPy planes [N,H,W] and ground truth [N,gt_h,gt_w] -> NumPy [N,10]"""
    planes, gts = np.ascontiguousarray(planes), np.ascontiguousarray(gts)
    e = _engine(*planes.shape[1:])
    return e.depth_eval(torch.from_numpy(planes).cuda(), torch.from_numpy(gts).cuda(), **kw).cpu().numpy()


def _twin_kw(kw):
    t = {k: v for k, v in kw.items() if k != "lds_pairs"}
    if "protocol" in t:
        t["protocol"] = {"eigen": D.EIGEN, "eigen_benchmark": D.EIGEN_BENCHMARK}[t["protocol"]]
    return t


def _check(got, want):
    """one frame's row against the twin's"""
    assert got.shape == want.shape == (D.NEVAL,)
    print("got ", got.tolist(), "\nwant", want.tolist())
    for j in D.EXACT:
        assert got[j] == want[j] or (np.isnan(got[j]) and np.isnan(want[j])), (j, got[j], want[j])
    for j in D.SUMMED:
        if np.isnan(want[j]):
            assert np.isnan(got[j]), j
        else:
            assert abs(got[j] - want[j]) <= D.summed_bound(want[D.N_VALID]) * abs(want[j]), (j, got[j], want[j])


def _against_twin(plane, gt, **kw):
    got = _run(plane[None], gt[None], **kw)[0]
    _check(got, D.evaluate_frame(plane, gt, **_twin_kw(kw)))
    return got


def _in_order(r):
    return 0 < r[D.A1] < r[D.A2] < r[D.A3] < 1


@pytest.mark.parametrize("odd", [True, False], ids=["odd_count", "even_count"])
def test_eigen_float64(odd):
    """cases 1, 2 and 12: 6 x 20 -> 11 x 37, holes, an odd and an even median subset; two runs are bit-identical"""
    P, gt = D.base_case(odd)
    r = _against_twin(P, gt)
    assert (int(r[D.N_MEDIAN]) % 2 == 1) == odd and _in_order(r) and D.clip_census(P, gt)[1] > 0
    assert r[D.N_VALID] >= 20 and (gt == 0).any()
    assert D.same_bits(_run(P[None], gt[None]), r[None])


def test_benchmark_protocol_with_far_ground_truth():
    """case 3: gt > 0 over the whole plane, values >= 80 present: the median subset is smaller than the mask"""
    P = D.disparity(6, 20, seed=5)
    gt = D.ground_truth(P, 11, 37, seed=6, valid=0.5, far=0.2)
    r = _against_twin(P, gt, protocol="eigen_benchmark")
    assert 0 < r[D.N_MEDIAN] < r[D.N_VALID] and _in_order(r)
    assert D.clip_census(P, gt, D.EIGEN_BENCHMARK)[1] > 0


def test_dense_ground_truth_with_and_without_the_list():
    """case 4: every pixel valid, 12 x 24 -> 33 x 70; the list too short for the frame (every pass scans the crop), and the default"""
    P = D.disparity(12, 24, seed=7)
    gt = np.minimum(D.ground_truth(P, 33, 70, seed=8, valid=1.0), np.float32(79.5))
    n_mask = int(D.mask_of(gt, D.EIGEN, 1e-3, 80.0).sum())
    y0, y1, x0, x1 = D.crop(D.EIGEN, 33, 70)
    assert n_mask == (y1 - y0) * (x1 - x0) > 1024 and D.clip_census(P, gt)[1] > 0      # more than one trip of the workgroup
    short = _against_twin(P, gt, lds_pairs=50)
    full = _against_twin(P, gt)
    assert D.same_bits(short, full) and _in_order(full)
    for cap in (0, 1, n_mask - 1, n_mask):
        assert D.same_bits(_run(P[None], gt[None], lds_pairs=cap)[0], full), cap


def test_three_frames_in_one_call():
    """case 5: the middle frame has no valid pixel: NaN with counts 0; the neighbours are their single-frame calls bit for bit"""
    P0, g0 = D.base_case(True)
    P2 = D.disparity(6, 20, seed=9)
    g2 = D.ground_truth(P2, 11, 37, seed=10, valid=0.6)
    got = _run(np.stack([P0, P0, P2]), np.stack([g0, np.zeros_like(g0), g2]))
    assert np.isnan(got[1, :8]).all() and got[1, D.N_VALID] == 0 and got[1, D.N_MEDIAN] == 0
    _check(got[1], D.evaluate_frame(P0, np.zeros_like(g0)))
    assert D.same_bits(got[0], _run(P0[None], g0[None])[0]) and D.same_bits(got[2], _run(P2[None], g2[None])[0])
    _check(got[2], D.evaluate_frame(P2, g2))
    off = _run(P0[None], np.zeros_like(g0)[None], median_scaling=False)[0]
    assert np.isnan(off[:7]).all() and off[D.RATIO] == 1.0 and off[D.N_VALID] == 0


def test_ground_truth_of_the_planes_size():
    """case 6: the resize is the identity: the metrics are the twin's without its resize"""
    P = D.disparity(6, 20, seed=11)
    gt = D.ground_truth(P, 6, 20, seed=12, valid=0.8)
    got = _against_twin(P, gt)
    _check(got, D.evaluate_frame(P, gt, do_resize=False))
    assert got[D.N_VALID] >= 10
    got = _against_twin(P, gt, protocol="eigen_benchmark")
    _check(got, D.evaluate_frame(P, gt, D.EIGEN_BENCHMARK, do_resize=False))


def test_shrink():
    """case 7: 6 x 20 -> 5 x 9"""
    P = D.disparity(6, 20, seed=13)
    gt = D.ground_truth(P, 5, 9, seed=14, valid=0.9)
    assert _against_twin(P, gt)[D.N_VALID] >= 4
    assert _against_twin(P, gt, protocol="eigen_benchmark")[D.N_VALID] >= 20


@pytest.mark.parametrize("shape", [(6, 20, 1, 37), (6, 20, 11, 1), (4, 20, 9, 37), (6, 4, 11, 9)], ids=["gt_one_row", "gt_one_column", "four_rows", "four_columns"])
def test_narrow_planes(shape):
    """case 8 (see the module's note)"""
    h, w, gh, gw = shape
    P = D.disparity(h, w, seed=15)
    gt = D.ground_truth(P, gh, gw, seed=16, valid=0.8)
    r = _against_twin(P, gt, protocol="eigen_benchmark")
    assert r[D.N_VALID] >= 5
    _against_twin(P, gt)                                                         # the Eigen crop of such a plane may be empty: NaN rows agree too


def test_float32_planes_are_their_promotion():
    """case 9"""
    P, gt = D.base_case(True)
    P32 = P.astype(np.float32)
    got = _against_twin(P32, gt)
    assert D.same_bits(got, _run(P32.astype(np.float64)[None], gt[None])[0])
    assert not D.same_bits(got, _run(P[None], gt[None])[0])                       # (the rounding to float32 shows)


def test_without_median_scaling():
    """case 10: ratio == 1.0; ground truth near the predictions, so that the thresholds separate"""
    P = D.disparity(6, 20, seed=17)
    gt = D.ground_truth(P, 11, 37, seed=18, valid=0.5, gain=1.0, spread=3.0)
    r = _against_twin(P, gt, median_scaling=False)
    assert r[D.RATIO] == 1.0 and _in_order(r)
    r = _against_twin(P, gt, median_scaling=False, protocol="eigen_benchmark")
    assert r[D.RATIO] == 1.0


def test_other_depth_unit_and_bounds():
    """case 11: depth_unit 5.4, bounds (0.8, 4): predictions clip at both ends"""
    P = D.disparity(6, 20, seed=19)
    kw = dict(depth_unit=5.4, min_depth=0.8, max_depth=4.0)
    for protocol, code, gain in (("eigen", D.EIGEN, 1.0), ("eigen_benchmark", D.EIGEN_BENCHMARK, 1.5)):
        gt = D.ground_truth(P, 11, 37, seed=20, valid=0.6, gain=gain, spread=3.0, depth_unit=5.4)
        lo, hi = D.clip_census(P, gt, code, **kw)
        assert lo > 0 and hi > 0, (protocol, lo, hi)
        r = _against_twin(P, gt, protocol=protocol, **kw)
        assert _in_order(r) and r[D.N_VALID] >= 20
        assert (r[D.N_MEDIAN] < r[D.N_VALID]) == (protocol == "eigen_benchmark")


def test_refusals_leave_the_output_untouched():
    """case 13"""
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import default_opts
    P, gt = D.base_case(True)
    e = _engine(6, 20)
    d = torch.from_numpy(np.stack([P, P])).cuda()
    g = torch.from_numpy(np.stack([gt, gt])).cuda()
    out = torch.full((2, D.NEVAL), SENTINEL, dtype=torch.float64, device="cuda")
    wide = torch.full((2 * 11 * 37,), 0.5, dtype=torch.float32, device="cuda")
    o = default_opts()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    e._bind()

    def call(opts=o, ev=None, n=2, f64=1, dp=p(d), gh=11, gw=37, gp=p(g), op=p(out), **fields):
        ev = _lib.depth_eval_opts() if ev is None else ev
        for k, v in fields.items():
            setattr(ev, k, v)
        return e.lib.tcsfm_depth_eval(e._h, None if opts is None else C.byref(opts), None if ev is False else C.byref(ev), n, f64, dp, gh, gw, gp, op)

    err = e.last_error
    assert call(dp=None) == E_ARG and "NULL" in err()
    assert call(gp=None) == E_ARG and call(op=None) == E_ARG and call(opts=None) == E_ARG and call(ev=False) == E_ARG and "NULL" in err()
    assert call(n=0) == E_ARG and "N must be at least 1" in err()
    assert call(n=-2) == E_ARG
    assert call(gh=0) == E_ARG and "gt_h and gt_w" in err()
    assert call(gw=-1) == E_ARG and "gt_h and gt_w" in err()
    assert call(protocol=2) == E_ARG and "protocol" in err()
    assert call(protocol=-1) == E_ARG
    for lo, hi in ((0.0, 80.0), (-1.0, 80.0), (80.0, 80.0), (5.0, 2.0), (float("nan"), 80.0), (1e-3, float("nan")), (1e-3, float("inf"))):
        assert call(min_depth=lo, max_depth=hi) == E_ARG and "min_depth" in err(), (lo, hi)
    for unit in (0.0, -30.0, float("nan"), float("inf")):
        assert call(depth_unit=unit) == E_ARG and "depth_unit" in err(), unit
    assert call(opts=default_opts(host_ptrs=1)) == E_ARG and "host_ptrs" in err()
    assert call(op=p(out, 4)) == E_ARG and "aligned" in err()
    # metrics_out on top of an input
    assert call(f64=0, dp=p(wide), op=p(wide)) == E_ARG and err() == "tcsfm_depth_eval: metrics_out overlaps disp"
    assert call(gp=p(wide), op=p(wide, 16)) == E_ARG and err() == "tcsfm_depth_eval: metrics_out overlaps gt"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wide == 0.5).all())
    assert call() == 0                                                            # the handle stays usable
    torch.cuda.synchronize()
    assert D.same_bits(out.cpu().numpy(), _run(np.stack([P, P]), np.stack([gt, gt])))
    # the wrapper's own checks
    with pytest.raises(ValueError):
        e.depth_eval(d, g, protocol="scannet")
    with pytest.raises(TypeError):
        e.depth_eval(d.to(torch.float16), g)
    with pytest.raises(RuntimeError, match="nothing kept"):
        e.sequence_depth_eval(gt[None])


# ---------------------------------------------------------------------------------------------------------------------------------
# the sequence form: 32 x 64 frames, T = 7, single-frame chunks -- the smallest frames-only call of tests/test_gpu_sequence_disp.py
H, W, T = 32, 64, 7
GT_H, GT_W = 45, 97


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("mode", ["plain", "post"])
def test_sequence_form_is_the_operator_on_the_fetched_planes(mode):
    import depthnet_twin
    import standins
    from tightly_coupled_sfm_amd import _lib, synth
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.evaluate_depth_eigen import evaluate
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    e = Engine(H, W, 8)
    dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
    e.attach_depthnet(dn)
    pn = PoseNetHIP(e, 8, standins.posenet_params(5))
    seq = synth.make_sequence(T, H, W, seed=4)
    frames = torch.as_tensor(np.ascontiguousarray(seq["frames"], dtype=np.float32)).pin_memory()
    K = seq["K"].astype(np.float32)
    o = default_opts(n_iters=3, argmin=1)
    kw = dict(sources=1, iterations=2, ring=3, windows_per_call=1, target_pos=0, cam_height=1.65 / 30.0)
    on = pn.odometry_sequence(frames, None, K, o, disparity=mode, **kw)
    planes = e.sequence_disparities()
    scales = e.sequence_scales()
    assert planes.dtype == (np.float64 if mode == "post" else np.float32) and planes.shape == (T, H, W)
    gts = np.stack([D.ground_truth(planes[t], GT_H, GT_W, seed=30 + t, valid=0.4) for t in range(T)])
    gts[2] = 0                                                                    # a frame without ground truth
    got = e.sequence_depth_eval(gts)
    want = e.depth_eval(torch.from_numpy(planes).cuda(), torch.from_numpy(gts).cuda()).cpu().numpy()
    assert got.shape == (T, D.NEVAL) and D.same_bits(got, want)
    assert np.isnan(got[2, :8]).all() and np.isfinite(np.delete(got, 2, axis=0)).all()
    for t in (0, T - 1):
        _check(got[t], D.evaluate_frame(planes[t], gts[t]))
    # a sub-range, other options, the benchmark protocol; a second run returns the same bits
    assert D.same_bits(e.sequence_depth_eval(gts[3:6], first=3), want[3:6])
    assert D.same_bits(e.sequence_depth_eval(gts[T - 1:], first=T - 1), want[T - 1:])
    okw = dict(protocol="eigen_benchmark", median_scaling=False, min_depth=0.5, max_depth=60.0, depth_unit=25.0, lds_pairs=16)
    assert D.same_bits(e.sequence_depth_eval(gts[1:4], first=1, **okw),
                       e.depth_eval(torch.from_numpy(planes[1:4]).cuda(), torch.from_numpy(gts[1:4]).cuda(), **okw).cpu().numpy())
    assert D.same_bits(e.sequence_depth_eval(gts), want)
    # the drop-in groups by size: frames 0, 1 at one size, 2 .. 6 at another
    mixed = [gts[0], gts[1]] + [np.ascontiguousarray(g[:40, :90]) for g in gts[2:]]
    res = evaluate(None, mixed, e)
    assert D.same_bits(res["metrics"][:2], want[:2])
    assert D.same_bits(res["metrics"][2:], e.sequence_depth_eval(np.stack(mixed[2:]), first=2))
    res2 = evaluate(planes, mixed, e)
    assert D.same_bits(res2["metrics"], res["metrics"]) and res["errors"].shape == (T, 7) and res["ratios"].shape == (T,)
    # the evaluation changed nothing of the call: planes, scales and poses are those of the same call without it
    assert D.same_bits(e.sequence_disparities().astype(np.float64), planes.astype(np.float64))
    again = pn.odometry_sequence(frames, None, K, o, disparity=mode, **kw)
    assert torch.equal(_bits(again[0]), _bits(on[0])) and torch.equal(_bits(again[1]), _bits(on[1]))
    assert D.same_bits(e.sequence_disparities().astype(np.float64), planes.astype(np.float64))
    s2 = e.sequence_scales()
    for k in ("scale", "median", "count"):
        assert torch.equal(_bits(s2[k]), _bits(scales[k])), k
    # refusals of the sequence form: the output keeps its contents
    ev = _lib.depth_eval_opts()
    out = np.full((T, D.NEVAL), SENTINEL)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda t=T, first=0, count=T, gh=GT_H, gw=GT_W, g=hp(gts), op=hp(out), opts=ev: e.lib.tcsfm_sequence_depth_eval(
        e._h, None if opts is None else C.byref(opts), t, first, count, gh, gw, g, op)
    err = e.last_error
    assert call(t=T - 1) == E_ARG and "T differs" in err()
    assert call(first=1) == E_ARG and "first + count <= T" in err()
    assert call(first=-1, count=1) == E_ARG and call(count=0) == E_ARG and call(first=T, count=1) == E_ARG and call(count=2**31 - 1) == E_ARG
    assert call(g=None) == E_ARG and "NULL" in err()
    assert call(op=None) == E_ARG and call(opts=None) == E_ARG
    assert call(gh=0) == E_ARG and "gt_h and gt_w" in err()
    bad = _lib.depth_eval_opts()
    bad.protocol = 5
    assert call(opts=bad) == E_ARG and "protocol" in err()
    assert call(op=hp(gts)) == E_ARG and err() == "tcsfm_sequence_depth_eval: metrics_out overlaps gt"
    assert bool((out == SENTINEL).all())
    assert call() == 0 and D.same_bits(out, want)
    # a later call with the stage off leaves nothing to evaluate
    pn.odometry_sequence(frames, None, K, o, **kw)
    with pytest.raises(RuntimeError, match="nothing kept"):
        e.sequence_depth_eval(gts)
    e.close()
