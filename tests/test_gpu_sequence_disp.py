"""tcsfm_sequence_disparity: the sequence calls keep every frame's disparity on the device -- "plain" (disp_to_depth's scaled_disp of
the network's output, float32) or "post" (helpers.get_disp_for_eigen: a second, mirrored pass and the blend, float64).  Every
comparison is bitwise.  The yardsticks are per-frame calls on the same handle: DepthNetHIP.disp_for_eigen on each frame alone (pinned
to the reference's blend by tests/test_gpu_disp_post.py) and Engine.disp_to_depth(DepthNetHIP.forward(frame))[0]; equality with them
for every frame shows that a frame's plane does not depend on chunking, ring, groups or lanes.  Poses, depth maps and scales must be
the bits of the same call with the stage off.

32 x 64 frames and the three shapes of tests/test_gpu_sequence_depthnet.py: single-frame chunks with every ring slot recycled twice;
chunks of four with a short last chunk; S = 2 with the target in the middle.  One and two lanes."""
import ctypes as C
import functools

import numpy as np
import pytest

import disp_post_inputs as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

H, W = 32, 64
E_ARG = -1
OFF, PLAIN, POST = 0, 1, 2
CAM = np.float32(1.65 / 30.0)

#        id                S  T   ring wpc target_pos
SHAPES = [("single_frame_chunks", 1, 7, 3, 1, 0),
          ("chunks_of_four", 1, 11, 0, 2, 0),
          ("middle_target", 2, 8, 0, 2, -1)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _depth_params():
    import depthnet_twin
    return depthnet_twin.depthnet_params(0)


@functools.lru_cache(maxsize=None)
def _pose_params():
    import standins
    return standins.posenet_params(5)


@functools.lru_cache(maxsize=None)
def _sequence(T):
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(T, H, W, seed=4)
    pin = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).pin_memory()
    return pin(seq["frames"]), seq["K"].astype(np.float32)


def _world(lanes, max_pairs=8, dn_images=8, attach=True):
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    e = Engine(H, W, max_pairs, lanes=lanes)
    dn = DepthNetHIP(e, dn_images, _depth_params())
    if attach:
        e.attach_depthnet(dn)
    return e, dn, PoseNetHIP(e, max_pairs, _pose_params())


_REF = {}


def _per_frame(e, dn, frames_dev, o, key):
    """the yardsticks, one frame per call -> (post float64 [T,H,W], plain float32 [T,H,W]); computed once per `key` and left unchanged
    (they are bits of per-frame calls: any handle of this size returns the same)"""
    if key not in _REF:
        post = np.concatenate([dn.disp_for_eigen(f[None], o.min_depth, o.max_depth).cpu().numpy() for f in frames_dev])
        plain = np.concatenate([e.disp_to_depth(dn.forward(f[None]), o.min_depth, o.max_depth)[0].cpu().numpy().reshape(1, H, W) for f in frames_dev])
        assert post.dtype == np.float64 and plain.dtype == np.float32 and np.isfinite(post).all() and float(post.std()) > 0
        assert float(np.abs(post - plain).max()) > 1e-6          # the two modes are different planes
        post.setflags(write=False); plain.setflags(write=False)
        _REF[key] = (post, plain)
    return _REF[key]


def _init_poses(T, S):
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.normal(scale=[1e-3, 1e-3, 2e-3, 3e-4, 3e-4, 3e-4], size=(T - S, 2 * S, 6)).astype(np.float32))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_odometry_keeps_every_frames_disparity(shape, lanes):
    from tightly_coupled_sfm_amd.engine import default_opts
    _, S, T, ring, wpc, tpos = shape
    e, dn, pn = _world(lanes)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    want_post, want_plain = _per_frame(e, dn, frames.cuda(), o, ("seq", T))
    kw = dict(sources=S, iterations=2, ring=ring, windows_per_call=wpc, target_pos=tpos)
    off = pn.odometry_sequence(frames, None, K, o, **kw)
    assert not _same(off[0], off[1])
    with pytest.raises(RuntimeError, match="nothing kept"):
        e.sequence_disparities()
    # post: the poses of the call with the stage off; every frame's plane is the per-frame call's
    post = pn.odometry_sequence(frames, None, K, o, disparity="post", **kw)
    assert _same(post[0], off[0]) and _same(post[1], off[1])
    got = e.sequence_disparities()
    assert got.shape == (T, H, W) and D.same_bits(got, want_post)
    for first, count in ((0, 1), (T - 1, 1), (2, 3), (1, T - 1)):
        assert D.same_bits(e.sequence_disparities(first, count), want_post[first:first + count]), (first, count)
    assert D.same_bits(e.sequence_disparities(3), want_post[3:])
    # plain: float32, the two-step path's scaled disparity; the poses again
    plain = pn.odometry_sequence(frames, None, K, o, disparity="plain", **kw)
    assert _same(plain[0], off[0]) and _same(plain[1], off[1])
    got = e.sequence_disparities()
    assert got.dtype == np.float32 and D.same_bits(got, want_plain)
    assert D.same_bits(e.sequence_disparities(T - 2, 2), want_plain[T - 2:])
    # the same run again: the same bits
    again = pn.odometry_sequence(frames, None, K, o, disparity="post", **kw)
    assert _same(again[1], off[1]) and D.same_bits(e.sequence_disparities(), want_post)
    e.close()


def test_groups_smaller_than_a_chunk():
    """a depth network of max_images = 2 under chunks of four frames: both passes and the blend run in groups of two"""
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T, wpc = 1, 11, 2
    e, dn, pn = _world(2, dn_images=2)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    want_post, want_plain = _per_frame(e, dn, frames.cuda(), o, ("seq", T))
    off = pn.odometry_sequence(frames, None, K, o, sources=S, iterations=2, windows_per_call=wpc)
    on = pn.odometry_sequence(frames, None, K, o, sources=S, iterations=2, windows_per_call=wpc, disparity="post")
    assert _same(on[0], off[0]) and _same(on[1], off[1]) and D.same_bits(e.sequence_disparities(), want_post)
    on = pn.odometry_sequence(frames, None, K, o, sources=S, iterations=2, windows_per_call=wpc, disparity="plain")
    assert _same(on[1], off[1]) and D.same_bits(e.sequence_disparities(), want_plain)
    e.close()


def test_refine_and_dense_sequences_keep_them_too():
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import default_opts
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    S, T, wpc = 1, 11, 2
    e, dn, _ = _world(2)
    frames, K = _sequence(T)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3, refine=_lib.REFINE_POSE_SCALE)
    od = default_opts(n_iters=2)
    want_post, _ = _per_frame(e, dn, frames.cuda(), o, ("seq", T))
    ref_pose, ref_ls = e.refine_sequence(frames, None, K, p0, o, sources=S, log_scale=True, windows_per_call=wpc)
    pose, ls = e.refine_sequence(frames, None, K, p0, o, sources=S, log_scale=True, windows_per_call=wpc, disparity="post")
    assert _same(pose, ref_pose) and _same(ls, ref_ls) and not _same(pose, p0)
    assert D.same_bits(e.sequence_disparities(), want_post)
    ref_dpose, ref_maps = e.refine_dense_sequence(frames, None, K, p0, od, sources=S, windows_per_call=wpc)
    with pytest.raises(RuntimeError, match="nothing kept"):                    # a later call with the stage off leaves nothing
        e.sequence_disparities()
    dpose, maps = e.refine_dense_sequence(frames, None, K, p0, od, sources=S, windows_per_call=wpc, disparity="post")
    assert _same(dpose, ref_dpose) and _same(maps, ref_maps) and float(maps.std()) > 0
    assert D.same_bits(e.sequence_disparities(), want_post)
    # SequenceRefiner.run_native passes the keyword through
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, default_opts(n_iters=3), S
    assert _same(sr.run_native(frames, None, K, p0, disparity="post"), sr.run_native(frames, None, K, p0))
    with pytest.raises(RuntimeError, match="nothing kept"):
        e.sequence_disparities()
    sr.run_native(frames, None, K, p0, disparity="post")
    assert D.same_bits(e.sequence_disparities(), want_post)
    e.close()


def test_scales_are_unchanged_beside_the_disparity_stage():
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T, wpc = 1, 11, 2
    e, dn, pn = _world(2)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    want_post, _ = _per_frame(e, dn, frames.cuda(), o, ("seq", T))
    kw = dict(sources=S, iterations=2, windows_per_call=wpc)
    ref = pn.odometry_sequence(frames, None, K, o, cam_height=float(CAM), **kw)
    want = e.sequence_scales()
    assert int((want["count"] > 0).sum()) > 0
    got_pose = pn.odometry_sequence(frames, None, K, o, cam_height=float(CAM), disparity="post", **kw)
    got = e.sequence_scales()
    assert _same(got_pose[0], ref[0]) and _same(got_pose[1], ref[1])
    for k in ("scale", "median", "count"):
        assert _same(got[k], want[k]), k
    assert D.same_bits(e.sequence_disparities(), want_post)
    e.close()


def test_camera_size_bytes():
    """u8 frames at twice the size, resized on the device: the disparities are those of the float frames Engine.resize_u8 makes"""
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T = 1, 7
    e, dn, pn = _world(2)
    frames, K = _sequence(T)
    small = (frames.numpy() * 255.0 + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)                  # [T,H,W,3]
    cam = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(small, 2, axis=1), 2, axis=2)))   # [T,2H,2W,3]
    o = default_opts(n_iters=3, argmin=1)
    resized = e.resize_u8(cam.cuda(), "hwc", "f32")
    assert resized.shape == (T, 3, H, W)
    want_post, _ = _per_frame(e, dn, resized, o, ("cam", T))
    kw = dict(sources=S, iterations=2, ring=5, windows_per_call=1, source_size=(2 * H, 2 * W))
    off = pn.odometry_sequence(cam, None, K, o, **kw)
    on = pn.odometry_sequence(cam, None, K, o, disparity="post", **kw)
    assert _same(on[0], off[0]) and _same(on[1], off[1]) and not _same(on[0], on[1])
    assert D.same_bits(e.sequence_disparities(), want_post)
    e.close()


def _c_odometry(e, pn, o, frames, depths, K, S=1, ring=0, wpc=1, tpos=0):
    """tcsfm_odometry_sequence itself -> (return code, PoseNet poses, refined poses)"""
    T = frames.shape[0]
    init = torch.zeros((T - S, 2 * S, 6)); out = torch.zeros_like(init)
    Kc = torch.as_tensor(np.ascontiguousarray(K, dtype=np.float32))
    hp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    e._bind()
    rc = e.lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kc), hp(init), hp(out), None, ring, wpc, tpos)
    return rc, init, out


def test_refusals_and_the_state_of_the_kept_planes():
    from tightly_coupled_sfm_amd.engine import default_opts
    T = 7
    e, dn, pn = _world(1, attach=False)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    want_post, want_plain = _per_frame(e, dn, frames.cuda(), o, ("seq", T))
    depths = torch.cat([e.disp_to_depth(dn.forward(f[None].cuda()), o.min_depth, o.max_depth)[1].cpu() for f in frames]).pin_memory()
    lib = e.lib
    err = e.last_error
    out = np.full((T, H, W), -7.0, np.float64)
    mode = C.c_int(-5)
    fetch = lambda t, first=0, count=None: lib.tcsfm_sequence_disparities(e._h, t, first, t - first if count is None else count,
                                                                          out.ctypes.data_as(C.c_void_p), C.byref(mode))
    untouched = lambda: bool((out == -7.0).all()) and mode.value == -5
    assert fetch(T) == E_ARG and "nothing kept" in err() and untouched()                    # before any call
    base = _c_odometry(e, pn, o, frames, depths, K)
    assert base[0] == 0
    assert fetch(T) == E_ARG and "nothing kept" in err() and untouched()                    # after a call with the stage off
    # stage on, nothing attached: refused whether depths are given or not; the texts name the reason
    assert lib.tcsfm_sequence_disparity(e._h, POST) == 0
    assert _c_odometry(e, pn, o, frames, depths, K)[0] == E_ARG and "tcsfm_sequence_disparity" in err() and "depths == NULL" in err()
    assert _c_odometry(e, pn, o, frames, None, K)[0] == E_ARG and "tcsfm_sequence_disparity" in err() and "attached depth network" in err()
    with pytest.raises(ValueError, match="attach_depthnet"):
        pn.odometry_sequence(frames, None, K, o, disparity="post")
    # attached: depths given are still refused; depth bounds out of order too
    e.attach_depthnet(dn)
    assert _c_odometry(e, pn, o, frames, depths, K)[0] == E_ARG and "depths == NULL" in err()
    assert err().startswith("tcsfm_odometry_sequence: the disparity stage")
    assert _c_odometry(e, pn, default_opts(n_iters=3, argmin=1, min_depth=3.0, max_depth=2.0), frames, None, K)[0] == E_ARG and "min_depth" in err()
    assert fetch(T) == E_ARG and "nothing kept" in err() and untouched()                    # refused calls leave nothing
    # the keyword makes the setting for its call and switches the stage off afterwards, whatever the handle's setting was
    with pytest.raises(RuntimeError, match="depths == NULL"):
        pn.odometry_sequence(frames, depths, K, o, disparity="plain")
    rc, i, r = _c_odometry(e, pn, o, frames, depths, K)
    assert rc == 0 and _same(r, base[2])                                                    # (off: depths are accepted again)
    # an unknown mode is refused and leaves the setting in force
    assert lib.tcsfm_sequence_disparity(e._h, PLAIN) == 0
    for bad in (3, -1, 17):
        assert lib.tcsfm_sequence_disparity(e._h, bad) == E_ARG and "tcsfm_sequence_disparity" in err()
    rc, i, r = _c_odometry(e, pn, o, frames, None, K)
    assert rc == 0 and _same(r, base[2]) and _same(i, base[1])
    f32 = np.full((T, H, W), -7.0, np.float32)
    assert lib.tcsfm_sequence_disparities(e._h, T, 0, T, f32.ctypes.data_as(C.c_void_p), C.byref(mode)) == 0 and mode.value == PLAIN
    assert D.same_bits(f32, want_plain)
    # the fetch's own refusals
    assert lib.tcsfm_sequence_disparity(e._h, POST) == 0
    assert _c_odometry(e, pn, o, frames, None, K)[0] == 0
    mode.value = -5
    assert fetch(T - 1) == E_ARG and "T differs" in err() and untouched()                   # a wrong T
    assert fetch(T + 1) == E_ARG and untouched()
    assert fetch(T, 1, T) == E_ARG and "first + count <= T" in err() and untouched()        # first + count > T
    assert fetch(T, T - 1, 2) == E_ARG and fetch(T, -1, 1) == E_ARG and fetch(T, 0, 0) == E_ARG and untouched()
    assert fetch(T, 0, 2**31 - 1) == E_ARG and untouched()
    assert lib.tcsfm_sequence_disparities(e._h, T, 0, T, None, None) == E_ARG and "NULL" in err()
    assert fetch(T) == 0 and mode.value == POST and D.same_bits(out, want_post)
    out[:] = -7.0
    assert lib.tcsfm_sequence_disparities(e._h, T, 2, 3, out.ctypes.data_as(C.c_void_p), None) == 0      # mode_out may be NULL
    assert D.same_bits(out[:3], want_post[2:5]) and bool((out[3:] == -7.0).all())
    # a later call with the stage off leaves nothing
    assert lib.tcsfm_sequence_disparity(e._h, OFF) == 0
    assert _c_odometry(e, pn, o, frames, None, K)[0] == 0
    mode.value = -5; out[:] = -7.0
    assert fetch(T) == E_ARG and "nothing kept" in err() and untouched()
    e.close()
