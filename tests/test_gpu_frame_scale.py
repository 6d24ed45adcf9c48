"""Per-frame metric scales: tcsfm_scale_recovery_frames (k_ground + k_median_frames, csrc/frame_scale_kernel.h) and the scale stage
of the three sequence calls (tcsfm_sequence_scale / tcsfm_sequence_scales).

The yardstick is the existing chain, tcsfm_scale_recovery on one item at a time (k_ground, then eight select launches): both are
exact selects on integer counts, so every comparison is bitwise -- int32 views, NaN by isnan -- and no tolerance is involved.  The
sequence tests use frames whose ground-pixel counts are all different (tests/test_sequence_scale_abi_cpu.py checks that on the CPU),
so a scale taken from a stale, shifted or not yet written ring slot changes a count."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import operator_inputs as OI  # noqa: E402

E_ARG = -1
H, W = 32, 64
CAM = np.float32(1.65 / 30.0)          # the reference's camera_height / depth unit

#        id                     S  T   ring wpc target_pos   (tests/test_gpu_sequence_depthnet.py)
SHAPES = [("single_frame_chunks", 1, 7, 3, 1, 0),
          ("chunks_of_four", 1, 11, 0, 2, 0),
          ("middle_target", 2, 8, 0, 2, -1)]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _same(a, b):
    """the same bits; NaN matches NaN"""
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def _engine(h, w, max_pairs, lanes=0):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(h, w, max_pairs, lanes=lanes) if lanes else Engine(h, w, max_pairs)


def _chain(e, depth, K):
    """the yardstick, item by item -> (scale [N], median [N], count [N], numpy's own lower median of the call's masked heights [N])"""
    sc, md, ct, srt = [], [], [], []
    for n in range(depth.shape[0]):
        s, m, hm, mm = e.scale_recovery(depth[n:n + 1], K[n:n + 1], float(CAM), maps=True)
        hm, mm = hm.cpu().numpy().ravel(), mm.cpu().numpy().ravel()
        v = np.sort(hm[mm > 0])
        sc.append(s.cpu()); md.append(m.cpu()); ct.append(int(mm.sum()))
        srt.append(v[(v.size - 1) // 2] if v.size else np.float32(np.nan))
    return torch.cat(sc), torch.cat(md), torch.tensor(ct, dtype=torch.int32), torch.as_tensor(np.asarray(srt, dtype=np.float32))


def _check_against_chain(e, depth, K, tag):
    scale, med, count = e.scale_recovery_frames(depth, K, float(CAM))
    want = _chain(e, depth, K)
    print(f"frames\t{tag}\tcount={count.cpu().tolist()}\tmedian={med.cpu().tolist()}")
    assert _same(count, want[2]), (tag, count.cpu().tolist(), want[2].tolist())
    assert _same(med, want[1]) and _same(scale, want[0]), (tag, med.cpu(), want[1], scale.cpu(), want[0])
    assert _same(med, want[3]), (tag, "numpy's lower median of the call's own masked heights", med.cpu(), want[3])
    assert bool((torch.isnan(scale.cpu()) == (count.cpu() == 0)).all()), tag
    return count.cpu().tolist()


def test_operator_equals_the_chain_and_numpy_item_by_item(oracle32, oracle64):
    """every batch of operator_inputs.median_cases (its pad ignored) and 11 frames of one sequence as ONE batch: scale and median are the
    bits of tcsfm_scale_recovery on the item alone, count the sum of that call's mask, median numpy's sorted[(count - 1) // 2]"""
    from tightly_coupled_sfm_amd import synth
    seen, engines = set(), {}
    for name, depth, K, _pad, _expect in OI.median_cases(oracle32, oracle64):
        N, _, h, w = depth.shape
        if (h, w) not in engines:
            engines[(h, w)] = _engine(h, w, 4)
        for c in _check_against_chain(engines[(h, w)], _t(depth), _t(K), name):
            seen.add((min(c, 3), c % 2))
    for e in engines.values():
        e.close()
    assert {(0, 0), (1, 1), (2, 0), (3, 1), (3, 0)} <= seen, seen
    seq = synth.make_sequence(11, 37, 53, seed=4)
    e = _engine(37, 53, 11)
    counts = _check_against_chain(e, _t(seq["depths"]), _t(np.repeat(seq["K"][None], 11, 0)), "sequence-37x53-N11")
    assert len(set(counts)) == 11 and {c % 2 for c in counts} == {0, 1}, counts      # a result written to the wrong item would show
    e.close()


def test_full_and_single_batches_optional_outputs_and_broadcast_K():
    """N = max_pairs and N = 1; median_out / count_out NULL; a [3,3] K for all items"""
    from tightly_coupled_sfm_amd import synth
    from tightly_coupled_sfm_amd.engine import default_opts
    h, w, M = 17, 33, 6
    seq = synth.make_sequence(M, h, w, seed=4)
    e = _engine(h, w, M)
    depth, K1 = _t(seq["depths"]), _t(seq["K"])
    KN = K1[None].expand(M, 3, 3).contiguous()
    full = e.scale_recovery_frames(depth, KN, float(CAM))
    want = _chain(e, depth, KN)
    assert _same(full[0], want[0]) and _same(full[1], want[1]) and _same(full[2], want[2])
    assert int((full[2] > 0).sum()) >= M // 2
    bc = e.scale_recovery_frames(depth, K1, float(CAM))                       # [3,3]: one camera
    assert all(_same(a, b) for a, b in zip(bc, full))
    one = e.scale_recovery_frames(depth[2:3], K1, float(CAM))
    assert all(_same(a, b[2:3]) for a, b in zip(one, full))
    P = lambda t: C.c_void_p(t.data_ptr())
    for n in (M, 1):
        out = torch.full((n,), -7.0, device="cuda")
        rc = e.lib.tcsfm_scale_recovery_frames(e._h, C.byref(default_opts()), n, P(depth), P(KN), C.c_float(float(CAM)), P(out), None, None)
        assert rc == 0, e.last_error()
        assert _same(out, full[0][:n])
    e.close()


@pytest.mark.parametrize("h,w", [(37, 53), (32, 64)], ids=["key-by-key", "vector-loads"])
def test_the_list_of_masked_keys_at_its_capacity(h, w, monkeypatch):
    """k_median_frames keeps a frame's masked keys in LDS after its first pass when they fit, and reads the plane again in every round
    when they do not: the same bits either way.  TCSFM_MEDIAN_LDS_KEYS moves the capacity onto a frame's own count: count - 1 (does
    not fit), count and count + 1 (fits), 0 (nothing fits), in a batch whose other frames lie on either side of it."""
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(4, h, w, seed=4)
    e = _engine(h, w, 4)
    depth, K = _t(seq["depths"]), _t(seq["K"])
    monkeypatch.delenv("TCSFM_MEDIAN_LDS_KEYS", raising=False)
    want = e.scale_recovery_frames(depth, K, float(CAM))
    counts = want[2].cpu().tolist()
    assert len(set(counts)) == 4 and min(counts) > 2, counts
    chain = _chain(e, depth, K[None].expand(4, 3, 3).contiguous())
    assert _same(want[0], chain[0]) and _same(want[1], chain[1]) and _same(want[2], chain[2])
    mid = sorted(counts)[1]
    for cap in (mid - 1, mid, mid + 1, 0, 1):
        monkeypatch.setenv("TCSFM_MEDIAN_LDS_KEYS", str(cap))
        got = e.scale_recovery_frames(depth, K, float(CAM))
        assert all(_same(a, b) for a, b in zip(got, want)), (cap, counts, got, want)
    e.close()


def test_a_frame_with_more_ground_than_the_list_holds():
    """192 x 640 planes under the camera: about half of each frame is ground, more keys than fit in LDS -- the rounds re-read the plane
    (vector loads), beside a noisy frame of the same batch that fits"""
    h, w = 192, 640
    K1 = OI.pinhole(h, w)
    noisy = OI.make_ground(h, w, 1)
    depth = np.stack([OI.plane(h, w, K1, OI.CAM_HEIGHT), noisy[0][0, 0], OI.plane(h, w, K1, 0.7)])[:, None]
    K = np.stack([K1, noisy[1][0], K1])
    e = _engine(h, w, 3)
    counts = _check_against_chain(e, _t(depth), _t(K), "planes-192x640")
    assert counts[0] > 36864 and counts[2] > 36864 and 0 < counts[1] <= 36864, counts      # kMedianLdsKeys, csrc/frame_scale_kernel.h
    e.close()


def test_refusals_launch_nothing():
    from tightly_coupled_sfm_amd.engine import default_opts
    h, w, M = 17, 33, 3
    e = _engine(h, w, M)
    hw = h * w
    depth = torch.ones((M, 1, h, w), device="cuda")
    K = _t(np.repeat(OI.pinhole(h, w)[None], M, 0))
    out = torch.full((3 * M,), -7.0, device="cuda")
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + 4 * off)
    o, oh = default_opts(), default_opts(host_ptrs=1)
    call = lambda o_, n, d, k, s, m, c: e.lib.tcsfm_scale_recovery_frames(e._h, C.byref(o_), n, d, k, C.c_float(float(CAM)), s, m, c)
    good = (P(depth), P(K), P(out), P(out, M), P(out, 2 * M))
    cases = [("NULL", (o, M, None) + good[1:]), ("NULL", (o, M, good[0], None) + good[2:]),
             ("NULL", (o, M, good[0], good[1], None, good[3], good[4])),
             ("N out of range", (o, 0) + good), ("N out of range", (o, M + 1) + good),
             ("host_ptrs", (oh, M) + good)]
    for text, args in cases:
        rc = call(*args)
        assert rc == E_ARG and text in e.last_error(), (text, rc, e.last_error())
    # an output on an input, and on another output
    keep_d, keep_K = depth.clone(), K.clone()
    for text, args in [("scale_out overlaps depth", (P(depth), P(K), P(depth, hw), P(out, M), P(out, 2 * M))),
                       ("median_out overlaps K", (P(depth), P(K), P(out), P(K, 9), P(out, 2 * M))),
                       ("count_out overlaps depth", (P(depth), P(K), P(out), P(out, M), P(depth, 2 * hw - 1))),
                       ("scale_out overlaps median_out", (P(depth), P(K), P(out), P(out, M - 1), P(out, 2 * M))),
                       ("scale_out overlaps count_out", (P(depth), P(K), P(out), P(out, M), P(out)))]:
        assert call(o, M, *args) == E_ARG and text in e.last_error(), (text, e.last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and torch.equal(depth, keep_d) and torch.equal(K, keep_K)
    # not pinhole: refused as tcsfm_scale_recovery refuses it
    Kbad = K.clone(); Kbad[1, 0, 1] = 0.5
    assert call(o, M, P(depth), P(Kbad), P(out), P(out, M), P(out, 2 * M)) != 0 and "pinhole" in e.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(o, M, *good) == 0                                    # the handle still runs a valid call
    e.synchronize()
    assert not bool((out == -7.0).any())
    e.close()
    for (h5, w5) in ((4, 9), (9, 4)):
        e = _engine(h5, w5, 1)
        d5, K5 = torch.ones((1, 1, h5, w5), device="cuda"), _t(OI.pinhole(h5, w5)[None])
        o5 = torch.full((3,), -7.0, device="cuda")
        rc = e.lib.tcsfm_scale_recovery_frames(e._h, C.byref(o), 1, P(d5), P(K5), C.c_float(float(CAM)), P(o5), P(o5, 1), P(o5, 2))
        assert rc == E_ARG and "image too small" in e.last_error(), e.last_error()
        torch.cuda.synchronize()
        assert bool((o5 == -7.0).all())
        e.close()


# ---- the sequence stage ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sequence(T):
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(T, H, W, seed=4)
    pin = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).pin_memory()
    return pin(seq["frames"]), pin(seq["depths"]), seq["K"].astype(np.float32)


def _init_poses(T, S):
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.normal(scale=[1e-3, 1e-3, 2e-3, 3e-4, 3e-4, 3e-4], size=(T - S, 2 * S, 6)).astype(np.float32))


def _operator_per_frame(e, depths, K):
    """tcsfm_scale_recovery_frames over the host depths [T,1,H,W], in batches the handle takes -> dict like Engine.sequence_scales()"""
    Kd = _t(K)
    parts = [e.scale_recovery_frames(depths[i:i + 8].cuda(), Kd, float(CAM)) for i in range(0, depths.shape[0], 8)]
    return dict(scale=torch.cat([p[0] for p in parts]).cpu(), median=torch.cat([p[1] for p in parts]).cpu(),
                count=torch.cat([p[2] for p in parts]).cpu())


def _scales_equal(got, want):
    return all(_same(got[k], want[k]) for k in ("scale", "median", "count"))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_refine_sequence_with_depths_given(shape, lanes):
    from tightly_coupled_sfm_amd.engine import default_opts
    _, S, T, ring, wpc, tpos = shape
    e = _engine(H, W, 8, lanes=lanes)
    frames, depths, K = _sequence(T)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3)
    kw = dict(sources=S, ring=ring, windows_per_call=wpc, target_pos=tpos)
    want = _operator_per_frame(e, depths, K)
    assert len(set(want["count"].tolist())) == T and int(want["count"].min()) > 0, want["count"].tolist()
    off = e.refine_sequence(frames, depths, K, p0, o, **kw)
    with pytest.raises(RuntimeError, match="tcsfm_sequence_scales"):
        e.sequence_scales(T)                                         # the stage was off: nothing kept
    on = e.refine_sequence(frames, depths, K, p0, o, cam_height=float(CAM), **kw)
    got = e.sequence_scales()
    assert _scales_equal(got, want), (got, want)
    assert _same(on, off) and not _same(on, p0)                      # the poses are the bits of the call with the stage off
    again = e.refine_sequence(frames, depths, K, p0, o, cam_height=float(CAM), **kw)
    assert _same(again, on) and _scales_equal(e.sequence_scales(), got)
    # the camera's bytes: another producer in front of the stage on the pack stream, the same depths -> the same scales
    u8 = (frames * 255.0).round().to(torch.uint8).pin_memory()
    on_u8 = e.refine_sequence(u8, depths, K, p0, o, cam_height=float(CAM), **kw)
    assert _scales_equal(e.sequence_scales(), want)
    assert _same(on_u8, e.refine_sequence(u8, depths, K, p0, o, **kw))
    e.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_dense_sequence_with_float_frames_runs_the_stage_alone_on_the_pack_stream(lanes):
    from tightly_coupled_sfm_amd.engine import default_opts
    _, S, T, ring, wpc, tpos = SHAPES[1]
    e = _engine(H, W, 8, lanes=lanes)
    frames, depths, K = _sequence(T)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=2)
    kw = dict(sources=S, ring=ring, windows_per_call=wpc, target_pos=tpos)
    want = _operator_per_frame(e, depths, K)
    off_pose, off_maps = e.refine_dense_sequence(frames, depths, K, p0, o, **kw)
    on_pose, on_maps = e.refine_dense_sequence(frames, depths, K, p0, o, cam_height=float(CAM), **kw)
    assert _scales_equal(e.sequence_scales(), want)
    assert _same(on_pose, off_pose) and _same(on_maps, off_maps)
    pose2, maps2 = e.refine_dense_sequence(frames, depths, K, p0, o, cam_height=float(CAM), **kw)
    assert _same(pose2, on_pose) and _same(maps2, on_maps) and _scales_equal(e.sequence_scales(), want)
    e.close()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=[s[0] for s in SHAPES[:2]])
def test_frames_only_odometry_scales_the_networks_depths(shape):
    """a depth network attached, depths == NULL: the stage follows the chunk's depth stage; its scales are the operator's on the
    two-step depths (DepthNetHIP.forward per frame, Engine.disp_to_depth), NaN pattern included"""
    import depthnet_twin
    import standins
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import default_opts
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    _, S, T, ring, wpc, tpos = shape
    e = _engine(H, W, 8, lanes=2)
    dn, pn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0)), PoseNetHIP(e, 8, standins.posenet_params(5))
    frames, _, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    two_step = torch.cat([e.disp_to_depth(dn.forward(f[None].cuda()), o.min_depth, o.max_depth)[1].cpu() for f in frames])
    want = _operator_per_frame(e, two_step, K)
    print("frames-only counts", want["count"].tolist())
    assert int((want["count"] > 0).sum()) * 2 >= T, want["count"].tolist()      # not a comparison of NaNs alone
    e.attach_depthnet(dn)
    kw = dict(sources=S, iterations=2, ring=ring, windows_per_call=wpc, target_pos=tpos)
    off = pn.odometry_sequence(frames, None, K, o, **kw)
    on = pn.odometry_sequence(frames, None, K, o, cam_height=float(CAM), **kw)
    got = e.sequence_scales()
    assert _scales_equal(got, want), (got, want)
    assert _same(on[0], off[0]) and _same(on[1], off[1])
    e.close()


def test_state_of_the_setting_and_of_the_kept_results():
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T = 1, 7
    e = _engine(H, W, 8, lanes=1)
    frames, depths, K = _sequence(T)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=2)
    out = np.full(3 * T, -7.0, np.float32)
    cnt = np.full(T, -7, np.int32)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    fetch = lambda t: e.lib.tcsfm_sequence_scales(e._h, t, P(out), P(out, T), P(cnt))
    untouched = lambda: bool((out == -7.0).all() and (cnt == -7).all())
    assert fetch(T) == E_ARG and "nothing kept" in e.last_error() and untouched()           # before any call
    e.refine_sequence(frames, depths, K, p0, o, sources=S)
    assert fetch(T) == E_ARG and "nothing kept" in e.last_error() and untouched()           # after a call with the stage off
    e.refine_sequence(frames, depths, K, p0, o, sources=S, cam_height=float(CAM))
    assert fetch(T - 1) == E_ARG and "T differs" in e.last_error() and untouched()          # a wrong T
    assert fetch(T + 1) == E_ARG and untouched()
    assert fetch(T) == 0 and not np.isnan(out[:2 * T]).any() and (cnt > 0).all()
    kept = e.sequence_scales()
    assert _same(kept["scale"], torch.from_numpy(out[:T].copy())) and _same(kept["count"], torch.from_numpy(cnt.copy()))
    # after cam_height= on a Python method the handle's setting is off again: the next plain call keeps nothing
    e.refine_sequence(frames, depths, K, p0, o, sources=S)
    with pytest.raises(RuntimeError, match="nothing kept"):
        e.sequence_scales(T)
    # the setting itself: refusals leave it unchanged
    lib = e.lib
    assert lib.tcsfm_sequence_scale(e._h, C.c_float(float(CAM))) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.tcsfm_sequence_scale(e._h, C.c_float(bad)) == E_ARG and "tcsfm_sequence_scale" in e.last_error()
    e.refine_sequence(frames, depths, K, p0, o, sources=S)          # (still on: set through the C entry, no keyword)
    assert _same(e.sequence_scales(T)["scale"], kept["scale"])
    # the stage needs depths: disparities are refused, and a refused call leaves nothing
    od = default_opts(n_iters=2, depth_is_disp=1)
    with pytest.raises(RuntimeError, match="depth_is_disp"):
        e.refine_sequence(frames, depths, K, p0, od, sources=S)
    assert fetch(T) == E_ARG and "nothing kept" in e.last_error()
    assert lib.tcsfm_sequence_scale(e._h, C.c_float(0.0)) == 0
    e.refine_sequence(frames, (1.0 / depths).pin_memory(), K, p0, od, sources=S)             # off: disparities are fine again
    e.close()
