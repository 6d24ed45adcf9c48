"""Camera-size 8-bit frames on the device: tcsfm_resize_u8 (the operator) and tcsfm_sequence_frame_source (the three sequence calls
reading camera-size bytes).

Every comparison is on bytes or bits; no tolerance appears.  The yardstick of the operator is the fixture tests/golden/golden_resize.npz:
PILLOW's bytes for the inputs of tests/resize_inputs.py (this file never imports PIL); the float output is `fixture.float() / 255`
bit for bit.  The yardstick of a sequence call with source_size on camera-size bytes is the SAME call on the fixture-resized bytes without
source_size, on the same engine, compared as int32 views.

Operator inputs: every case of resize_inputs.CASES (both passes, one pass, none, upscaling with windows cut at the borders, two tiles per
axis with partial last tiles), interleaved and planar, byte and float outputs, and the source shifted by 0 .. 3 bytes inside a larger
buffer so that frames, rows and planes take every alignment the staging code distinguishes; sentinel pads around dst.

The sequence with the depth network attached runs at 63 x 125 -> 32 x 64 with T = 8 (the network takes multiples of 32 only); the others
at 47 x 79 -> 24 x 40 with T = 20, two windows per call and a 12-slot ring, so that the ring wraps and mirror slots are written."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_inputs as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG = -1
F32_CHW, U8_CHW, U8_HWC = 0, 1, 2
PAD = 16                    # sentinel bytes / floats on both sides of every destination
SENT_F, SENT_B = -7.5, 0xA5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- operator

@functools.lru_cache(maxsize=None)
def _engine(H, W):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(H, W, 2)


def _operator(e, name, layout, out, shift):
    """one tcsfm_resize_u8 call -> (destination with its pads, expected), CPU tensors"""
    from tightly_coupled_sfm_amd.engine import default_opts
    g = R.golden()
    _, (h, w), (H, W), N = R.CASE[name]
    src_hwc, want_hwc = torch.from_numpy(g["in_" + name]), torch.from_numpy(g["out_" + name])
    hwc = layout == "hwc"
    src = src_hwc if hwc else src_hwc.permute(0, 3, 1, 2).contiguous()
    nb = src.numel()
    buf = torch.zeros(nb + 8, dtype=torch.uint8, device="cuda")
    buf[shift:shift + nb].copy_(src.reshape(-1))
    fmt = U8_HWC if hwc else U8_CHW
    if out == "f32":
        want_body = (want_hwc.permute(0, 3, 1, 2).contiguous().float() / 255).reshape(-1)
        dst = torch.full((want_body.numel() + 2 * PAD,), SENT_F, dtype=torch.float32, device="cuda")
        want = torch.full((want_body.numel() + 2 * PAD,), SENT_F, dtype=torch.float32)
        dfmt, esz = F32_CHW, 4
    else:
        want_body = (want_hwc if hwc else want_hwc.permute(0, 3, 1, 2).contiguous()).reshape(-1)
        dst = torch.full((want_body.numel() + 2 * PAD,), SENT_B, dtype=torch.uint8, device="cuda")
        want = torch.full((want_body.numel() + 2 * PAD,), SENT_B, dtype=torch.uint8)
        dfmt, esz = fmt, 1
    want[PAD:PAD + want_body.numel()] = want_body
    o = default_opts()
    e._bind()
    rc = e.lib.tcsfm_resize_u8(e._h, C.byref(o), fmt, N, h, w, C.c_void_p(buf.data_ptr() + shift), dfmt, C.c_void_p(dst.data_ptr() + esz * PAD))
    assert rc == 0, e.last_error()
    torch.cuda.synchronize()
    return dst.cpu(), want


@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_operator_returns_pillows_bytes(name, layout, out):
    _, _, (H, W), _ = R.CASE[name]
    e = _engine(H, W)
    for shift in range(4):
        got, want = _operator(e, name, layout, out, shift)
        body = slice(PAD, got.numel() - PAD)
        if out == "u8":
            diff = int((got[body] != want[body]).sum())
            print(name, layout, out, shift, "differing bytes:", diff)
            assert diff == 0, (name, layout, shift)
            assert torch.equal(got, want), "a byte beyond dst's extent changed"
        else:
            diff = int((_bits(got[body]) != _bits(want[body])).sum())
            print(name, layout, out, shift, "differing floats:", diff)
            assert diff == 0, (name, layout, shift)
            assert torch.equal(_bits(got), _bits(want)), "a float beyond dst's extent changed"


def test_engine_method():
    g = R.golden()
    name = "kitti_ratio"
    _, (h, w), (H, W), N = R.CASE[name]
    e = _engine(H, W)
    src, want = torch.from_numpy(g["in_" + name]), torch.from_numpy(g["out_" + name])
    wf = want.permute(0, 3, 1, 2).contiguous().float() / 255
    assert _same(e.resize_u8(src.cuda(), "hwc", out="f32").cpu(), wf)
    assert torch.equal(e.resize_u8(src.cuda(), "hwc", out="u8").cpu(), want)
    chw = src.permute(0, 3, 1, 2).contiguous()
    assert _same(e.resize_u8(chw.cuda(), "chw").cpu(), wf)
    assert torch.equal(e.resize_u8(chw.cuda(), "chw", out="u8").cpu(), want.permute(0, 3, 1, 2).contiguous())
    with pytest.raises(TypeError):
        e.resize_u8(src, "hwc")                              # a CPU tensor
    with pytest.raises(TypeError):
        e.resize_u8(src.cuda(), "chw")                       # the layout is stated, not guessed
    with pytest.raises(ValueError):
        e.resize_u8(src.cuda(), "hwc", out="f16")


def test_operator_and_setter_refusals():
    from tightly_coupled_sfm_amd.engine import default_opts
    name = "kitti_ratio"
    _, (h, w), (H, W), N = R.CASE[name]
    e = _engine(H, W)
    lib, o = e.lib, default_opts()
    err = lambda: lib.tcsfm_last_error(e._h).decode()
    nb = N * 3 * h * w
    big = torch.zeros(nb * 3 + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((N * 3 * H * W + 2 * PAD,), SENT_F, dtype=torch.float32, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    e._bind()
    call = lambda fmt, n, opts, sh, sw, s, dfmt, d: lib.tcsfm_resize_u8(e._h, C.byref(opts), fmt, n, sh, sw, s, dfmt, d)
    D = P(dst, 4 * PAD)
    assert call(F32_CHW, N, o, h, w, P(big), F32_CHW, D) == E_ARG and "format" in err()
    assert call(U8_HWC, N, o, h, w, P(big), U8_CHW, D) == E_ARG and "dst_format" in err()
    assert call(U8_HWC, 0, o, h, w, P(big), F32_CHW, D) == E_ARG and "N" in err()
    assert call(U8_HWC, N, default_opts(host_ptrs=1), h, w, P(big), F32_CHW, D) == E_ARG and "host_ptrs" in err()
    assert call(U8_HWC, N, o, h, w, None, F32_CHW, D) == E_ARG
    assert call(U8_HWC, N, o, 0, w, P(big), F32_CHW, D) == E_ARG and call(U8_HWC, N, o, h, -3, P(big), F32_CHW, D) == E_ARG
    # beyond the stated limit: more than 8 times the frame along an axis; a side above 32768 (refused before any byte is read)
    assert call(U8_HWC, 1, o, 8 * H + 1, w, P(big), F32_CHW, D) == E_ARG and "8 times" in err()
    assert call(U8_HWC, 1, o, h, 8 * W + 1, P(big), F32_CHW, D) == E_ARG and "8 times" in err()
    assert call(U8_HWC, 1, o, h, 32769, P(big), F32_CHW, D) == E_ARG
    # overlap: a byte dst inside src, a float dst on src's last bytes, dst == src
    assert call(U8_HWC, N, o, h, w, P(big), U8_HWC, P(big, nb - 1)) == E_ARG and err() == "tcsfm_resize_u8: dst overlaps src"
    assert call(U8_CHW, N, o, h, w, P(big, nb), F32_CHW, P(big, 8)) == E_ARG and err() == "tcsfm_resize_u8: dst overlaps src"
    assert call(U8_CHW, N, o, h, w, P(big), U8_CHW, P(big)) == E_ARG and err() == "tcsfm_resize_u8: dst overlaps src"
    # the setter: refusals leave the setting as it was (none: a float call below still runs)
    src_fn = lib.tcsfm_sequence_frame_source
    for bad in ((-1, w), (h, -1), (0, w), (h, 0), (8 * H + 1, w), (h, 8 * W + 1), (40000, w)):
        assert src_fn(e._h, *bad) == E_ARG and "tcsfm_sequence_frame_source" in err(), bad
    assert src_fn(e._h, 8 * H, 8 * W) == 0 and src_fn(e._h, 1, 1) == 0 and src_fn(e._h, 0, 0) == 0      # the limit itself, upscaling, none
    torch.cuda.synchronize()
    assert bool((dst == SENT_F).all()) and int(big.count_nonzero()) == 0      # no refused call touched a buffer
    g = R.golden()
    got = e.resize_u8(torch.from_numpy(g["in_" + name]).cuda(), "hwc", out="u8").cpu()
    assert torch.equal(got, torch.from_numpy(g["out_" + name]))                # ... and the handle still works


# ---------------------------------------------------------------------------------------------------------- sequence calls

@functools.lru_cache(maxsize=None)
def _sequence(name):
    """-> {cam_hwc, cam_chw: the camera-size bytes (pinned), small_hwc, small_chw: Pillow's bytes for them (pinned), poison: float frames
    of another order, depths, K, sizes}"""
    from tightly_coupled_sfm_amd import synth
    g = R.golden()
    _, (h, w), (H, W), T = R.SEQUENCE[name]
    cam, small = torch.from_numpy(g["in_" + name]), torch.from_numpy(g["out_" + name])
    assert cam.shape == (T, h, w, 3) and small.shape == (T, H, W, 3) and len(np.unique(g["out_" + name])) > 32
    seq = synth.make_sequence(T, H, W, seed=4)               # depths and K of the H x W frames (the same corridor and camera path)
    depths = torch.as_tensor(np.ascontiguousarray(seq["depths"], dtype=np.float32)).pin_memory()
    chw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    f32 = chw(small).float() / 255
    return dict(cam_hwc=cam.pin_memory(), cam_chw=chw(cam).pin_memory(), small_hwc=small.pin_memory(), small_chw=chw(small).pin_memory(),
                poison=torch.roll(f32, 1, 0).pin_memory(), depths=depths, K=seq["K"].astype(np.float32), source=(h, w), size=(H, W), T=T)


def _init_poses(T, S):
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.normal(scale=[1e-3, 1e-3, 2e-3, 3e-4, 3e-4, 3e-4], size=(T - S, 2 * S, 6)).astype(np.float32))


def _all_same(got, ref):
    return len(got) == len(ref) and all(_same(g, r) for g, r in zip(got, ref))


def _check(run, s):
    """run(frames, source_size) -> tuple of result tensors.  The yardstick: Pillow's bytes without source_size.  The device ring outlives
    a call, so a float call on OTHER frames dirties every slot before each call that is compared: a call that resized nothing would
    not find the yardstick's floats there.  Afterwards a plain byte call still returns the yardstick: the setting was restored."""
    ref = run(s["small_hwc"], None)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    assert not _all_same(run(s["poison"], None), ref)
    for layout in ("hwc", "chw"):
        got = run(s["cam_" + layout], s["source"])
        assert _all_same(got, ref), layout
        run(s["poison"], None)
    assert _all_same(run(s["small_chw"], None), ref)
    return ref


@pytest.mark.parametrize("S", [1, 2])
def test_refine_sequence_on_camera_size_bytes(S):
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    s = _sequence("seq")
    (H, W), T = s["size"], s["T"]
    e = Engine(H, W, 8, lanes=2)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3, refine=_lib.REFINE_POSE_SCALE)
    run = lambda f, src: e.refine_sequence(f, s["depths"], s["K"], p0, o, sources=S, ring=12, log_scale=True, windows_per_call=2,
                                           **({} if src is None else {"source_size": src}))
    pose, ls = _check(run, s)
    assert not _same(pose, p0) and float(ls.abs().max()) > 0


def test_refine_dense_sequence_on_camera_size_bytes():
    """the mode with no other stage on the pack stream: the resize alone runs there, and writes the raw mirror slots"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    s = _sequence("seq")
    (H, W), T, S = s["size"], s["T"], 1
    e = Engine(H, W, 8, lanes=2)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=2)
    run = lambda f, src: e.refine_dense_sequence(f, s["depths"], s["K"], p0, o, sources=S, ring=12, windows_per_call=2,
                                                 **({} if src is None else {"source_size": src}))
    pose, maps = _check(run, s)
    assert not _same(pose, p0) and float(maps.std()) > 0


@functools.lru_cache(maxsize=None)
def _pose_params():
    import standins
    return standins.posenet_params(5)


@functools.lru_cache(maxsize=None)
def _depth_params():
    import depthnet_twin
    return depthnet_twin.depthnet_params(0)


def test_odometry_sequence_on_camera_size_bytes():
    """S = 2, the stand-in PoseNet reads the resized raw frames, mirror slots included"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    s = _sequence("seq")
    (H, W), S = s["size"], 2
    e = Engine(H, W, 8, lanes=2)
    pn = PoseNetHIP(e, 8, _pose_params())
    o = default_opts(n_iters=3, argmin=1)
    run = lambda f, src: pn.odometry_sequence(f, s["depths"], s["K"], o, sources=S, iterations=2, ring=12, windows_per_call=2,
                                              **({} if src is None else {"source_size": src}))
    init, out = _check(run, s)
    assert not _same(init, out) and float(init.abs().max()) > 0


def test_odometry_sequence_frames_only_on_camera_size_bytes():
    """the stand-in depth network attached and depths = None: the depth stage reads the resized frames too.  One window per call and a
    five-slot ring of single-frame chunks: every slot is recycled"""
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    s = _sequence("seq_net")
    (H, W), S = s["size"], 2
    e = Engine(H, W, 8, lanes=2)
    pn = PoseNetHIP(e, 8, _pose_params())
    dn = DepthNetHIP(e, 8, _depth_params())
    e.attach_depthnet(dn)
    o = default_opts(n_iters=3, argmin=1)
    run = lambda f, src: pn.odometry_sequence(f, None, s["K"], o, sources=S, iterations=2, ring=5, windows_per_call=1,
                                              **({} if src is None else {"source_size": src}))
    init, out = _check(run, s)
    assert not _same(init, out) and float(init.abs().max()) > 0


def test_source_setting_contract():
    """the C entry itself: sticky; refused with float frames; the overlap check counts T*3*src_h*src_w bytes"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    s = _sequence("seq")
    (H, W), (h, w), T, S = s["size"], s["source"], s["T"], 1
    e = Engine(H, W, 8)
    lib = e.lib
    err = lambda: lib.tcsfm_last_error(e._h).decode()
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3)
    Kc = torch.as_tensor(s["K"])
    hp = lambda t: C.c_void_p(t.data_ptr())

    def c_call(frames, pose_out=None):
        out = torch.zeros_like(p0) if pose_out is None else pose_out
        e._bind()
        return lib.tcsfm_refine_sequence(e._h, C.byref(o), T, S, hp(frames), hp(s["depths"]), hp(Kc), hp(p0), hp(out), None, 12, 2, 0), out

    f32 = (s["small_chw"].float() / 255).pin_memory()
    rc, ref = c_call(f32)
    assert rc == 0 and not _same(ref, p0)
    # a source with float frames: the sequence call is refused; the setting stays
    assert lib.tcsfm_sequence_frame_source(e._h, h, w) == 0
    rc, _ = c_call(f32)
    assert rc == E_ARG and "TCSFM_FRAMES_F32_CHW" in err()
    # sticky: two byte calls after one setting, a refused setter call in between
    assert lib.tcsfm_sequence_frame_format(e._h, U8_HWC) == 0
    rc, got = c_call(s["cam_hwc"])
    assert rc == 0 and _same(got, ref), err()
    assert lib.tcsfm_sequence_frame_source(e._h, h, 0) == E_ARG
    rc, got = c_call(s["cam_hwc"])
    assert rc == 0 and _same(got, ref)
    # the frames range is T*3*h*w bytes: an output right behind them is disjoint, one on their last byte is refused
    nb = T * 3 * h * w
    room = torch.zeros(nb + p0.numel() * 4 + 8, dtype=torch.uint8).pin_memory()
    room[:nb].copy_(s["cam_hwc"].reshape(-1))
    behind = (nb + 3) // 4 * 4
    out_behind = room[behind:behind + p0.numel() * 4].view(torch.float32).view(p0.shape)
    rc, got = c_call(room, out_behind)
    assert rc == 0 and _same(got, ref), err()
    inside = (nb - 1) // 4 * 4
    out_inside = room[inside:inside + p0.numel() * 4].view(torch.float32).view(p0.shape)
    rc, _ = c_call(room, out_inside)
    assert rc == E_ARG and err() == "tcsfm_refine_sequence: pose_out overlaps frames"
    # (0, 0): bytes at H x W again; then floats
    assert lib.tcsfm_sequence_frame_source(e._h, 0, 0) == 0
    rc, got = c_call(s["small_hwc"])
    assert rc == 0 and _same(got, ref)
    assert lib.tcsfm_sequence_frame_format(e._h, F32_CHW) == 0
    rc, got = c_call(f32)
    assert rc == 0 and _same(got, ref)
