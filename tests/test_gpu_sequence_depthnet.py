"""tcsfm_sequence_depthnet: the sequence calls with depths == NULL -- the attached depth network computes every frame's depth on the
device as the frame's chunk lands in the ring -- against the two-step path on the same handle: DepthNetHIP.forward per frame, then
Engine.disp_to_depth, those depths as host tensors in the existing call.  Every comparison is bitwise (int32 views, torch.equal): the
stage's head applies disp_to_depth's own expression to the value the plain head stores, so no tolerance is involved.

32 x 64 frames: the smallest size the depth network accepts.  Shapes: single-frame chunks with every ring slot recycled twice; chunks
of four with a short last chunk and mirror slots; S = 2 with the target in the middle.  One and two lanes (a lane probe that falls
back to one stream is accepted: the results are the same bits either way)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

H, W = 32, 64
E_ARG = -1

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


def _world(lanes, max_pairs=8, dn_images=8):
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    e = Engine(H, W, max_pairs, lanes=lanes)
    return e, DepthNetHIP(e, dn_images, _depth_params()), PoseNetHIP(e, max_pairs, _pose_params())


def _two_step_depths(e, dn, frames, o):
    """the yardstick: the depth network on one frame per call, then tcsfm_disp_to_depth, back on the host"""
    out = []
    for f in frames:
        disp = dn.forward(f[None].cuda())
        out.append(e.disp_to_depth(disp, o.min_depth, o.max_depth)[1].cpu())
    d = torch.cat(out).pin_memory()
    assert d.shape == (frames.shape[0], 1, H, W) and float(d.std()) > 0
    return d


def _init_poses(T, S):
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.normal(scale=[1e-3, 1e-3, 2e-3, 3e-4, 3e-4, 3e-4], size=(T - S, 2 * S, 6)).astype(np.float32))


def _c_odometry(e, pn, o, frames, depths, K, S=1, ring=0, wpc=1, tpos=0):
    """tcsfm_odometry_sequence itself -> (return code, PoseNet poses, refined poses)"""
    T = frames.shape[0]
    init = torch.zeros((T - S, 2 * S, 6)); out = torch.zeros_like(init)
    Kc = torch.as_tensor(np.ascontiguousarray(K, dtype=np.float32))
    hp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    e._bind()
    rc = e.lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kc), hp(init), hp(out), None, ring, wpc, tpos)
    return rc, init, out


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_odometry_from_frames_alone_matches_the_two_step_path(shape, lanes):
    from tightly_coupled_sfm_amd.engine import default_opts
    _, S, T, ring, wpc, tpos = shape
    e, dn, pn = _world(lanes)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    depths = _two_step_depths(e, dn, frames, o)
    kw = dict(sources=S, iterations=2, ring=ring, windows_per_call=wpc, target_pos=tpos)
    ref_init, ref_out = pn.odometry_sequence(frames, depths, K, o, **kw)
    e.attach_depthnet(dn)
    init, out = pn.odometry_sequence(frames, None, K, o, **kw)
    assert _same(init, ref_init) and _same(out, ref_out)
    assert not _same(init, out)                                  # (something was refined)
    init2, out2 = pn.odometry_sequence(frames, None, K, o, **kw)  # the same run again: the same bits
    assert _same(init2, init) and _same(out2, out)


def test_refine_and_dense_sequences_from_frames_alone():
    """tcsfm_refine_sequence with given initial poses (pose + scale: log_scale_out too) and tcsfm_refine_dense_sequence (no pack
    cache: the stage alone runs on the pack stream), chunks of four, two lanes"""
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T, wpc = 1, 11, 2
    e, dn, _ = _world(2)
    frames, K = _sequence(T)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3, refine=_lib.REFINE_POSE_SCALE)
    od = default_opts(n_iters=2)
    depths = _two_step_depths(e, dn, frames, o)
    ref_pose, ref_ls = e.refine_sequence(frames, depths, K, p0, o, sources=S, log_scale=True, windows_per_call=wpc)
    ref_dpose, ref_dmaps = e.refine_dense_sequence(frames, depths, K, p0, od, sources=S, windows_per_call=wpc)
    e.attach_depthnet(dn)
    pose, ls = e.refine_sequence(frames, None, K, p0, o, sources=S, log_scale=True, windows_per_call=wpc)
    assert _same(pose, ref_pose) and _same(ls, ref_ls) and not _same(pose, p0)
    dpose, dmaps = e.refine_dense_sequence(frames, None, K, p0, od, sources=S, windows_per_call=wpc)
    assert _same(dpose, ref_dpose) and _same(dmaps, ref_dmaps)
    # SequenceRefiner.run_native passes None through
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, default_opts(n_iters=3), S
    assert _same(sr.run_native(frames, None, K, p0), sr.run_native(frames, depths, K, p0))


def test_chunks_larger_than_max_images_run_in_groups():
    """a depth network of max_images = 2 under chunks of four frames: the stage runs groups of two, the same bits per image"""
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T, wpc = 1, 11, 2
    e, dn, pn = _world(2, dn_images=2)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    depths = _two_step_depths(e, dn, frames, o)
    ref = pn.odometry_sequence(frames, depths, K, o, sources=S, iterations=2, windows_per_call=wpc)
    e.attach_depthnet(dn)
    got = pn.odometry_sequence(frames, None, K, o, sources=S, iterations=2, windows_per_call=wpc)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


def test_fused_head_writes_the_depths_of_the_two_launch_form():
    """the ring's depth planes themselves: tcsfm_refine_dense_sequence with n_iters = 0 hands back, per directed pair, the depth plane
    it was given (through its pack); frames-only and two-step agree on every pixel's bits, one chunk"""
    from tightly_coupled_sfm_amd.engine import default_opts
    S, T = 1, 4
    e, dn, _ = _world(1)
    frames, K = _sequence(7)
    frames = frames[:T].clone().pin_memory()
    o = default_opts(n_iters=0)
    depths = _two_step_depths(e, dn, frames, o)
    p0 = _init_poses(T, S)
    ref_pose, ref_maps = e.refine_dense_sequence(frames, depths, K, p0, o, sources=S, windows_per_call=2)
    e.attach_depthnet(dn)
    pose, maps = e.refine_dense_sequence(frames, None, K, p0, o, sources=S, windows_per_call=2)
    assert _same(maps, ref_maps) and _same(pose, ref_pose)
    assert float(ref_maps.std()) > 0


def test_attachment_contract():
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    T = 7
    e, dn, pn = _world(1)
    frames, K = _sequence(T)
    o = default_opts(n_iters=3, argmin=1)
    depths = _two_step_depths(e, dn, frames, o)
    lib = e.lib
    err = lambda: lib.tcsfm_last_error(e._h).decode()

    def valid():                                                 # the handle still runs a valid call, with the same result
        rc, i, r = _c_odometry(e, pn, o, frames, depths, K)
        assert rc == 0 and _same(i, base[1]) and _same(r, base[2])

    base = _c_odometry(e, pn, o, frames, depths, K)
    assert base[0] == 0
    # nothing attached: NULL depths is refused (the code and text every later refusal of this kind must show)
    rc0 = _c_odometry(e, pn, o, frames, None, K)[0]
    text0 = err()
    assert rc0 == E_ARG and "NULL input" in text0
    valid()
    with pytest.raises(ValueError, match="attach_depthnet"):
        pn.odometry_sequence(frames, None, K, o)
    # explicit depths with a network attached: the bits of the call with nothing attached
    other = (depths * 1.25).pin_memory()
    ref_other = _c_odometry(e, pn, o, frames, other, K)
    e.attach_depthnet(dn)
    got_other = _c_odometry(e, pn, o, frames, other, K)
    assert got_other[0] == 0 and _same(got_other[1], ref_other[1]) and _same(got_other[2], ref_other[2])
    assert not _same(ref_other[2], base[2])
    # depth_is_disp with NULL depths is refused: the stage produces depths
    od = default_opts(n_iters=3, depth_is_disp=1)
    p0 = _init_poses(T, 1)
    pout = torch.zeros_like(p0)
    Kc = torch.as_tensor(K)
    hp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.tcsfm_refine_sequence(e._h, C.byref(od), T, 1, hp(frames), None, hp(Kc), hp(p0), hp(pout), None, 0, 1, 0) == E_ARG
    assert "depth_is_disp" in err()
    valid()
    assert _c_odometry(e, pn, o, frames, None, K)[0] == 0        # (still attached)
    # detached again: today's refusal, code and text
    e.attach_depthnet(None)
    assert _c_odometry(e, pn, o, frames, None, K)[0] == rc0 and err() == text0
    valid()
    # a network of another handle, and one without weights, are refused by the attach call; what was attached stays
    e.attach_depthnet(dn)
    e2 = Engine(H, W, 2)
    foreign = DepthNetHIP(e2, 1, _depth_params())
    assert lib.tcsfm_sequence_depthnet(e._h, foreign._dn) == E_ARG and "tcsfm_sequence_depthnet" in err()
    with pytest.raises(ValueError):
        e.attach_depthnet(foreign)
    unloaded = DepthNetHIP(e, 1)
    assert lib.tcsfm_sequence_depthnet(e._h, unloaded._dn) == E_ARG and "loaded" in err()
    with pytest.raises(RuntimeError):
        e.attach_depthnet(unloaded)
    valid()
    rc, i, r = _c_odometry(e, pn, o, frames, None, K)
    assert rc == 0 and _same(i, base[1]) and _same(r, base[2])
    # destroying the attached network detaches it
    dn.close()
    assert _c_odometry(e, pn, o, frames, None, K)[0] == rc0 and err() == text0
    with pytest.raises(ValueError, match="attach_depthnet"):
        pn.odometry_sequence(frames, None, K, o)
    valid()
