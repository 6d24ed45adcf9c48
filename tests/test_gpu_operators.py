"""The drop-in operators behind stn / helpers / losses / learning_helpers / plot_loss_surface / dnet_layers -- tcsfm_warp,
tcsfm_warp_posenet_input, tcsfm_photometric, tcsfm_ssim, tcsfm_smooth_loss, tcsfm_disp_to_depth, tcsfm_loss_surface,
tcsfm_scale_recovery -- against the float64 oracle beyond the golden sizes: batches in which every item differs in images, both
depth maps, intrinsics and pose; frames of less than one block (5x9, 17x33), with a ragged last block (37x53, 100x333), the two
production sizes (192x640, 256x448) and one call of 19 items on an Engine made for 24; poses that keep most samples inside the
frame and poses that push most of them out.  tests/operator_inputs.py builds the inputs and holds the judging rules (decision
pixels and their cap; bound = max(existing bound, MARGIN * |oracle32 - oracle64|), MARGIN = 4); tests/test_operators_inputs_cpu.py
checks the inputs themselves.  The median of the scale recovery is checked bit for bit against numpy on the call's own fp32
heights and masks: no tolerance, no oracle.

MEASURED on an MI355X (TCSFM_TEST_OPERATOR_REPORT=<file> appends one line per map and case), worst over all cases of a map:
r = |hip - f64| / |oracle32 - f64| against the fixed MARGIN of 4, and u = |hip - f64| / bound, the share of the bound in use.

    map                      r       u        map                      r       u
    warp rec                 1.97    0.27     ssim first / last row    0.02    0.006
    warp projected depth     1.70    0.18     ssim first / last column 0.00    0.001
    warp computed depth      0.77    0.009    ssim interior            0.01    0.001
    photometric diff         1.26    0.22     smoothness, kernel       (31)    0.023
    photometric weight       2.63    0.21     smoothness, drop-in      1.00    0.024
    photometric auto error   0.13    0.005    disparity -> scaled      0.51    0.042
    photometric rec          1.97    0.27     disparity -> depth       0.57    0.057
    ground height            1.28    0.32     loss surface median      0.07    0.018
                                              loss surface maximum     (5.5)   0.10

Every map fits inside MARGIN = 4 wherever the margin is what sets the bound.  The two ratios in brackets are cases in which the
existing absolute bound is the larger one by far and the ratio divides by an fp32 error that happens to be tiny: the smoothness
loss (fp32 torch happens to land within 2.5e-10 of float64 at 100x333, the kernel is at 7.7e-9 there, the bound is 2e-6) and the
largest relative error of a loss-surface sweep (2.0e-4 against the existing 2e-3).  SSIM is the other way round: the kernel centres
the window on the pixel before it squares and is 300 times closer to float64 than the oracle's fp32 build, which subtracts squared
means (up to 3e-4 on planes of zeros and ones).  No validity, auto-mask or ground-mask decision differed from float64 at more than
the cap allows; the median and the scale were bit-exact on every case.
"""
import ctypes as C
import os

import numpy as np
import pytest

import operator_inputs as OI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TCSFM_E_ARG = -1          # include/tcsfm.h


def _eng(H, W, n):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(H, W, n)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _report(test, tag, name, err, e32, bnd):
    """print every figure before it is asserted; TCSFM_TEST_OPERATOR_REPORT=<file> keeps them"""
    line = f"{test}\t{tag}\t{name}\thip-f64={err:.3e}\tf32-f64={e32:.3e}\tratio={err / e32 if e32 > 0 else float('nan'):.2f}\tbound={bnd:.3e}"
    print(line)
    f = os.environ.get("TCSFM_TEST_OPERATOR_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _hold(test, tag, errs, e32s, floors):
    """every map of one case: report, then assert  error <= max(floor, MARGIN * fp32 oracle's error)"""
    fails = []
    for k, err in errs.items():
        bnd = OI.bound(floors[k], e32s[k])
        _report(test, tag, k, err, e32s[k], bnd)
        if not err <= bnd:
            fails.append((k, err, bnd))
    assert not fails, (test, tag, fails)


def _case_dev(c):
    return {k: _t(v) for k, v in c.items()}


def _engine_for(H, W, N):
    return _eng(H, W, OI.MANY_MAX_PAIRS if (H, W, N) == OI.MANY else N)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OI.PAIR_CASES, ids=OI.PAIR_IDS)
def test_warp_and_posenet_input_vs_oracle(case, oracle64, oracle32):
    """inverse_warp2 (stn.py:234-273): rec, validity, projected and computed depth per item; the PoseNet input (train_mono.py:73-77):
    channels 0-2 = tgt * valid, 3-5 = rec, the latter bit-identical to inverse_warp2's (one kernel writes both)"""
    H, W, N, s = case
    tag = OI.PAIR_IDS[OI.PAIR_CASES.index(case)]
    c = OI.make_case(H, W, N, s)
    d = _case_dev(c)
    e = _engine_for(H, W, N)
    rec, valid, pd, cd = (_np(x) for x in e.inverse_warp2(d["src"], d["depth_t"], d["depth_s"], -d["pose"], d["K"]))
    pin = _np(e.posenet_input(d["tgt"], d["src"], d["depth_t"], d["depth_s"], d["pose"], d["K"]))
    assert np.array_equal(pin[:, 3:6].view(np.uint32), rec.view(np.uint32)), tag
    assert np.array_equal(pin[:, 0:3], c["tgt"] * valid), tag         # a product with 0 or 1 is exact
    assert set(np.unique(valid)) <= {0.0, 1.0}
    for n in range(N):
        ref = OI.oracle_warp(oracle64, c, n)
        got = dict(rec=rec[n], valid=valid[n, 0], proj_depth=pd[n, 0], comp_depth=cd[n, 0])
        err, e32 = OI.judge_warp(got, ref, (tag, n, "hip")), OI.judge_warp(OI.oracle_warp(oracle32, c, n), ref, (tag, n, "f32"))
        _hold("warp", f"{tag}/{n}", err, e32, OI.FLOOR)
    e.close()


@pytest.mark.parametrize("weights", OI.PHOTO_WEIGHTS, ids=lambda w: f"l1={w[0]},ssim={w[1]}")
@pytest.mark.parametrize("case", OI.PAIR_CASES, ids=OI.PAIR_IDS)
def test_photometric_maps_vs_oracle(case, weights, oracle64, oracle32):
    """compute_photometric_error (helpers.py:8-23): diff, validity, weight, auto-mask error, auto-mask, rec per item"""
    from tightly_coupled_sfm_amd.engine import default_opts
    H, W, N, s = case
    wl, ws = weights
    tag = f"{OI.PAIR_IDS[OI.PAIR_CASES.index(case)]}-l1={wl}"
    c = OI.make_case(H, W, N, s)
    d = _case_dev(c)
    e = _engine_for(H, W, N)
    r = e.compute_photometric_error(d["tgt"], d["src"], d["depth_t"], d["depth_s"], d["pose"], d["K"], default_opts(w_l1=wl, w_ssim=ws))
    keys = dict(diff="diff_img", valid="warp_valid", weight="weight_mask", auto_err="auto_mask_error", auto_mask="auto_mask", rec="img_rec")
    maps = {k: _np(r[v]) for k, v in keys.items()}
    assert np.array_equal(_np(r["valid_mask"]), maps["auto_mask"] * maps["valid"]), tag
    for n in range(N):
        ref = OI.oracle_photometric(oracle64, c, n, wl, ws)
        got = {k: (v[n] if k == "rec" else v[n, 0]) for k, v in maps.items()}
        err = OI.judge_photometric(got, ref, (tag, n, "hip"))
        e32 = OI.judge_photometric(OI.oracle_photometric(oracle32, c, n, wl, ws), ref, (tag, n, "f32"))
        _hold("photometric", f"{tag}/{n}", err, e32, OI.FLOOR)
    e.close()


@pytest.mark.parametrize("H,W", OI.SSIM_SHAPES)
def test_ssim_vs_oracle(H, W, oracle64, oracle32):
    """SSIM_Loss.forward (losses.py:27-41) on N * C planes, constant planes and planes of zeros and ones among them; the first and
    last rows and columns are judged on their own, each against the fp32 oracle's error in that region"""
    x, y = OI.make_ssim_planes(H, W)
    e = _eng(H, W, x.shape[0])
    got = _np(e.ssim_loss(_t(x), _t(y)))
    ref, r32 = OI.oracle_ssim(oracle64, x, y), OI.oracle_ssim(oracle32, x, y)
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert np.all(got[1, 1] == 0.0), "two equal constant planes: SSIM loss exactly 0"
    for name, sel in OI.ssim_regions(H, W).items():
        _hold("ssim", f"{H}x{W}", {name: OI._maxabs(got, ref, sel)}, {name: OI._maxabs(r32, ref, sel)}, {name: OI.FLOOR["ssim"]})
    e.close()


@pytest.mark.parametrize("H,W,N", OI.SHAPES + [OI.MANY], ids=lambda v: str(v))
def test_smooth_loss_vs_reference_expression(H, W, N):
    """get_smooth_loss (losses.py:43-61), the kernel and the losses.get_smooth_loss drop-in, against the reference expression in
    float64 torch; every item has a different mean disparity (2e-6 relative is the bound of the existing 24x40 test)"""
    from tightly_coupled_sfm_amd import losses
    disp, img = OI.make_smooth(H, W, N)
    ref, r32 = OI.smooth_reference(disp, img, torch.float64), OI.smooth_reference(disp, img, torch.float32)
    e = _engine_for(H, W, N)
    got = e.smooth_loss(_t(disp), _t(img))
    drop = float(losses.get_smooth_loss(_t(disp), _t(img)))
    errs = dict(kernel=abs(got - ref) / ref, drop_in=abs(drop - ref) / ref)
    e32 = abs(r32 - ref) / ref
    # the drop-in returns its result in the dtype of the disparity (fp32): half an ulp on top
    _hold("smooth", f"{H}x{W}-N{N}", errs, dict(kernel=e32, drop_in=e32), dict(kernel=2e-6, drop_in=2e-6))
    e.close()


def test_disp_to_depth_large_map_vs_oracle(oracle64, oracle32):
    """disp_to_depth (learning_helpers.py:77-86) on a map of more blocks than one grid row holds, values exactly 0 and 1 included
    (2e-6 relative is the bound of the existing 8x8 test)"""
    disp = OI.make_disp()
    e = _eng(8, 8, 1)
    s, z = (_np(v) for v in e.disp_to_depth(_t(disp), OI.MIN_DEPTH, OI.MAX_DEPTH))
    s64, z64 = oracle64.disp_to_depth(disp, OI.MIN_DEPTH, OI.MAX_DEPTH)
    s32, z32 = oracle32.disp_to_depth(disp, OI.MIN_DEPTH, OI.MAX_DEPTH)
    rel = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b) / b))
    _hold("disp_to_depth", str(disp.size), dict(scaled=rel(s, s64), depth=rel(z, z64)), dict(scaled=rel(s32, s64), depth=rel(z32, z64)),
          dict(scaled=2e-6, depth=2e-6))
    for i in (0, 1, disp.size - 2, disp.size - 1):       # the ends of the range, at both ends of the map
        want = OI.MAX_DEPTH if disp[i] == 0 else OI.MIN_DEPTH
        assert abs(z[i] / want - 1) < 2e-6, (i, z[i], want)
    e.close()


@pytest.mark.parametrize("H,W", OI.SURFACE_SHAPES)
def test_loss_surface_vs_oracle(H, W, oracle64, oracle32):
    """generate_loss_surface's cost sweeps (plot_loss_surface.py:31-47) along z and in yaw, one launch each, in the form of the
    existing golden test: median and maximum relative error (floors 2e-5 and 2e-3), argmin within one step"""
    one, sweeps = OI.make_surface(H, W)
    e = _eng(H, W, 32)
    args = tuple(_t(one[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K"))
    for i, poses in enumerate(sweeps):
        mine = e.loss_surface(*args, _t(poses))
        ref, r32 = OI.oracle_surface(oracle64, one, poses), OI.oracle_surface(oracle32, one, poses)
        rel, rel32 = np.abs(mine - ref) / ref, np.abs(r32 - ref) / ref
        _hold("loss_surface", f"{H}x{W}-sweep{i}", dict(median=float(np.median(rel)), max=float(rel.max())),
              dict(median=float(np.median(rel32)), max=float(rel32.max())), dict(median=2e-5, max=2e-3))
        assert abs(int(np.argmin(mine)) - int(np.argmin(ref))) <= 1
        assert 0 < int(np.argmin(ref)) < len(poses) - 1, "the sweep must bracket its minimum"
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", OI.SHAPES + [OI.MANY], ids=lambda v: str(v))
def test_ground_heights_and_masks_vs_oracle(H, W, N, oracle64, oracle32):
    """DNet ScaleRecovery's height map and ground mask (dnet_layers.py:259-304,319-322) per item, with per-item intrinsics"""
    depth, K = OI.make_ground(H, W, N)
    e = _engine_for(H, W, N)
    _, _, hm, mm = e.scale_recovery(_t(depth), _t(K), OI.CAM_HEIGHT, maps=True)
    hm, mm = _np(hm)[:, 0], _np(mm)[:, 0]
    for n in range(N):
        h64, m64 = oracle64.ground_height(depth[n, 0], K[n])
        h32, m32 = oracle32.ground_height(depth[n, 0], K[n])
        err, e32 = OI.judge_ground(hm[n], mm[n], h64, m64, (H, W, n, "hip")), OI.judge_ground(h32, m32, h64, m64, (H, W, n, "f32"))
        _hold("ground", f"{H}x{W}-N{N}/{n}", dict(height=err), dict(height=e32), OI.FLOOR)
    e.close()


def test_scale_recovery_median_is_the_exact_lower_median(oracle64, oracle32):
    """the radix select (k_sel_hist / k_sel_pick) against numpy ON THE CALL'S OWN fp32 heights and masks: the median is, bit for
    bit, sorted[(count - 1) // 2] of the masked heights -- image 0's repeated for pad_to_batch -- and the scale is
    real_cam_height / median in fp32.  Counts of 0, 1, 2, odd and even, exact ties, heights that differ only in the lowest or only
    in the highest byte, pad_to_batch of 0, N + 1 and 3 N, frames of less than one block, N = 1."""
    seen = set()
    for name, depth, K, pad, expect in OI.median_cases(oracle32, oracle64):
        N, _, H, W = depth.shape
        e = _eng(H, W, N)
        scale, med, hm, mm = e.scale_recovery(_t(depth), _t(K), OI.CAM_HEIGHT, pad_to_batch=pad, maps=True)
        scale, med, hm, mm = _np(scale), _np(med), _np(hm)[:, 0], _np(mm)[:, 0]
        want, count = OI.check_median_structure(name, hm, mm, pad, expect)     # the case is what its name claims, on the GPU's own maps
        plain = _np(e.scale_recovery(_t(depth), _t(K), OI.CAM_HEIGHT, pad_to_batch=pad))
        print(f"median\t{name}\tcount={count}\tgot={med[0]!r}\twant={want!r}")
        if count == 0:
            assert np.isnan(med[0]) and np.isnan(scale[0]) and np.isnan(plain[0]), name
        else:
            assert med.view(np.uint32)[0] == np.float32(want).view(np.uint32), (name, count, med[0], want)
            assert scale.view(np.uint32)[0] == (np.float32(OI.CAM_HEIGHT) / np.float32(want)).view(np.uint32), (name, scale[0], want)
            assert plain.view(np.uint32)[0] == scale.view(np.uint32)[0], name                  # with and without the map outputs
        seen.add((min(count, 3), count % 2))
        e.close()
    assert {(0, 0), (1, 1), (2, 0), (3, 1), (3, 0)} <= seen


@pytest.mark.parametrize("H,W", [(4, 9), (9, 4)])
def test_scale_recovery_refuses_frames_below_five(H, W):
    """k_ground's reflected neighbour index (H - 3, W - 3 and their neighbours) would leave an image of fewer than 5 rows or
    columns: the call returns TCSFM_E_ARG with a message and launches nothing (the outputs keep their contents)"""
    e = _eng(H, W, 1)
    depth, K = _t(np.ones((1, 1, H, W))), _t(OI.pinhole(H, W)[None])
    out = torch.full((2 + 2 * H * W,), -7.0, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)
    from tightly_coupled_sfm_amd.engine import default_opts
    rc = e.lib.tcsfm_scale_recovery(e._h, C.byref(default_opts()), 1, P(depth), P(K), C.c_float(OI.CAM_HEIGHT), 0, P(out), P(out, 1), P(out, 2),
                                    P(out, 2 + H * W))
    assert rc == TCSFM_E_ARG and "image too small" in e.last_error(), (rc, e.last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(Exception, match="image too small"):
        e.scale_recovery(depth, K, OI.CAM_HEIGHT)
    e.close()
