"""8-bit camera frames: tcsfm_frames_from_u8 (the operator) and tcsfm_sequence_frame_format (the three sequence calls reading bytes).

Every comparison is bitwise (int32 views, torch.equal).  The yardstick of the operator is `u8.float() / 255` on the CPU -- IEEE
division, correctly rounded, what the reference's ArrayToTensor computes; the yardstick of a sequence call on bytes is the SAME call
on `u8 / 255` as pinned float32 with the default format, on the same engine.  No tolerance is involved anywhere.

Operator inputs.  A frame of H W pixels has Q = H W // 4 whole quads (one thread each) and a tail of r = H W % 4 pixels.  A byte value
must be seen at each of the four positions of a quad (the four lanes of a 32-bit load and of a 16-byte store) and in the tail, in
every channel; the small sizes cannot hold 256 values per position in one input, so a case runs V = ceil(256 / min(Q, r or Q))
inputs ("variants") whose values advance so that together they hold every byte value at every position class -- _coverage() asserts
it.  The variants sit back to back in one device buffer, so their source addresses (and, with the sentinel pads, their destination
addresses) take every alignment the sizes allow; a second run shifts the whole source by one byte."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG = -1
F32_CHW, U8_CHW, U8_HWC = 0, 1, 2
PAD = 4                     # sentinel floats on both sides of every destination
SENTINEL = -7.5

#         H   W
SIZES = [(4, 4),            # one block, no tail
         (5, 7),            # H W = 35: 3 H W odd -> only the tail and the unaligned paths beyond variant / frame 0
         (30, 45),          # H W = 1350: H W % 4 = 2, 3 H W % 4 = 2 -> frames 2 and 3 of a batch are misaligned; two blocks
         (32, 64)]          # H W = 2048: all fast paths


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- operator

@functools.lru_cache(maxsize=None)
def _variants(H, W, N):
    """uint8 [V, N, 3, H W]: every byte value at every quad position and in the tail, in every channel (module docstring)"""
    hw = H * W
    Q, r = hw // 4, hw % 4
    V = -(-256 // min(Q, r or Q))
    rng = np.random.default_rng(1000 * H + W)
    v = rng.integers(0, 256, size=(V, N, 3, hw), dtype=np.uint8)               # "the rest": a fixed seed
    k = np.arange(V)[:, None, None, None]
    f = np.arange(N)[None, :, None, None]
    c = np.arange(3)[None, None, :, None]
    p = np.arange(min(Q, 256) * 4)[None, None, None, :]
    v[..., :min(Q, 256) * 4] = ((p // 4) + k * min(Q, 256) + 37 * (p % 4) + 85 * c + 11 * f) % 256
    if r:
        t = np.arange(r)[None, None, None, :]
        v[..., 4 * Q:] = (t + k * r + 53 * c + 11 * f) % 256
    return v


def _coverage(v, H, W):
    hw = H * W
    Q, r = hw // 4, hw % 4
    for c in range(3):
        for j in range(4):
            assert len(np.unique(v[:, 0, c, j:4 * Q:4])) == 256, (c, j)
        if r:
            assert len(np.unique(v[:, 0, c, 4 * Q:])) == 256, c


def _run_operator(e, fmt, v, H, W, shift):
    """every variant through tcsfm_frames_from_u8 -> (destination buffer with its pads, expected buffer), CPU tensors"""
    from tightly_coupled_sfm_amd.engine import default_opts
    V, N = v.shape[:2]
    hw = H * W
    chw = torch.from_numpy(v)                                                  # [V,N,3,hw]
    src_cpu = chw if fmt == U8_CHW else chw.permute(0, 1, 3, 2).contiguous()    # HWC: [V,N,hw,3]
    nb = N * 3 * hw
    buf = torch.zeros(V * nb + shift, dtype=torch.uint8, device="cuda")
    buf[shift:].copy_(src_cpu.reshape(-1))
    stride = nb + 2 * PAD
    dst = torch.full((V * stride,), SENTINEL, dtype=torch.float32, device="cuda")
    want = torch.full((V, stride), SENTINEL, dtype=torch.float32)
    want[:, PAD:PAD + nb] = (chw.float() / 255).reshape(V, nb)
    o = default_opts()
    e._bind()
    for k in range(V):
        rc = e.lib.tcsfm_frames_from_u8(e._h, C.byref(o), fmt, N, C.c_void_p(buf.data_ptr() + shift + k * nb),
                                        C.c_void_p(dst.data_ptr() + 4 * (k * stride + PAD)))
        assert rc == 0, e.last_error()
    torch.cuda.synchronize()
    return dst.cpu().reshape(V, stride), want


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("fmt", [U8_CHW, U8_HWC], ids=["chw", "hwc"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_operator_is_the_cpu_division_bit_for_bit(size, fmt, N):
    from tightly_coupled_sfm_amd.engine import Engine
    H, W = size
    v = _variants(H, W, N)
    _coverage(v, H, W)
    e = Engine(H, W, 2)
    for shift in (0, 1):                                   # src as the buffer gives it, then one byte into a larger buffer
        got, want = _run_operator(e, fmt, v, H, W, shift)
        nb = N * 3 * H * W
        assert torch.equal(_bits(got[:, PAD:PAD + nb]), _bits(want[:, PAD:PAD + nb])), (size, fmt, N, shift)
        assert torch.equal(_bits(got), _bits(want)), "a float beyond dst's extent changed"      # (the sentinels on both sides)


def test_engine_method_infers_the_layout():
    from tightly_coupled_sfm_amd.engine import Engine
    H, W = 30, 45
    e = Engine(H, W, 2)
    chw = torch.from_numpy(_variants(H, W, 3)[0].reshape(3, 3, H, W))
    want = chw.float() / 255
    assert _same(e.frames_from_u8(chw.cuda()).cpu(), want)
    assert _same(e.frames_from_u8(chw.permute(0, 2, 3, 1).contiguous().cuda()).cpu(), want)
    with pytest.raises(TypeError):
        e.frames_from_u8(chw)                              # a CPU tensor
    with pytest.raises(TypeError):
        e.frames_from_u8(chw.cuda()[:, :, :, :44])         # a wrong shape
    with pytest.raises(TypeError):
        e.frames_from_u8(want.cuda())                      # floats


def test_operator_refusals():
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    H, W, N = 30, 45, 3
    nb = N * 3 * H * W
    e = Engine(H, W, 2)
    lib, o = e.lib, default_opts()
    err = lambda: lib.tcsfm_last_error(e._h).decode()
    big = torch.zeros(nb * 5 + 64, dtype=torch.uint8, device="cuda")           # room for src and for a dst, wherever the cases put them
    dst = torch.full((nb + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    e._bind()
    call = lambda fmt, n, opts, s, d: lib.tcsfm_frames_from_u8(e._h, C.byref(opts), fmt, n, s, d)
    assert call(F32_CHW, N, o, P(big), P(dst, 4 * PAD)) == E_ARG and "format" in err()
    assert call(7, N, o, P(big), P(dst, 4 * PAD)) == E_ARG and "format" in err()
    assert call(U8_HWC, 0, o, P(big), P(dst, 4 * PAD)) == E_ARG and "N" in err()
    assert call(U8_HWC, N, default_opts(host_ptrs=1), P(big), P(dst, 4 * PAD)) == E_ARG and "host_ptrs" in err()
    assert call(U8_HWC, N, o, None, P(dst, 4 * PAD)) == E_ARG
    # dst inside src's range (any overlap counts: dst starting at src's last bytes; dst ending in src's first bytes)
    assert call(U8_HWC, N, o, P(big), P(big, (nb - 4) // 4 * 4)) == E_ARG and err() == "tcsfm_frames_from_u8: dst overlaps src"
    assert call(U8_CHW, N, o, P(big, 4 * nb), P(big, 8)) == E_ARG and err() == "tcsfm_frames_from_u8: dst overlaps src"
    assert call(U8_CHW, N, o, P(big), P(big)) == E_ARG and err() == "tcsfm_frames_from_u8: dst overlaps src"
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and int(big.count_nonzero()) == 0      # no refused call touched a buffer
    # ... and the handle still works
    v = torch.from_numpy(_variants(H, W, N)[0].reshape(N, 3, H, W))
    assert _same(e.frames_from_u8(v.cuda()).cpu(), v.float() / 255)


# ---------------------------------------------------------------------------------------------------------- sequence calls

#        id                     S  T   ring wpc target_pos      (the shape table of tests/test_gpu_sequence_depthnet.py)
SHAPES = [("single_frame_chunks", 1, 7, 3, 1, 0),     # every slot recycled twice: a stale byte or float slot changes the poses
          ("chunks_of_four", 1, 11, 0, 2, 0),          # a short last chunk, mirror slots
          ("middle_target", 2, 8, 0, 2, -1)]
LAYOUTS = ("chw", "hwc")


@functools.lru_cache(maxsize=None)
def _sequence(T, H, W):
    """-> {f32: the yardstick's pinned float frames u8 / 255, chw / hwc: the same frames as pinned bytes, poison: other float frames
    (f32 rolled by one frame: every ring slot gets another frame), depths, K}"""
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(T, H, W, seed=4)
    q = np.round(np.asarray(seq["frames"], dtype=np.float64) * 255).astype(np.uint8)          # [T,3,H,W]
    chw = torch.from_numpy(q).pin_memory()
    hwc = torch.from_numpy(np.ascontiguousarray(q.transpose(0, 2, 3, 1))).pin_memory()
    f32 = (chw.float() / 255).pin_memory()
    assert len(np.unique(q)) > 32
    depths = torch.as_tensor(np.ascontiguousarray(seq["depths"], dtype=np.float32)).pin_memory()
    return dict(f32=f32, chw=chw, hwc=hwc, poison=torch.roll(f32, 1, 0).pin_memory(), depths=depths, K=seq["K"].astype(np.float32))


def _init_poses(T, S):
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.normal(scale=[1e-3, 1e-3, 2e-3, 3e-4, 3e-4, 3e-4], size=(T - S, 2 * S, 6)).astype(np.float32))


def _all_same(got, ref):
    return len(got) == len(ref) and all(_same(g, r) for g, r in zip(got, ref))


def _check(run):
    """run(key of _sequence) -> tuple of result tensors.  Float frames (the yardstick), both byte layouts, float frames again (the
    setting was restored).  The device ring outlives a call, and where it does not wrap (chunks_of_four, middle_target) a call leaves
    every frame's floats in its slot and mirror slot: a byte call that converted nothing would find the yardstick's floats there.  So a
    float call on OTHER frames dirties every slot before each call that is compared."""
    ref = run("f32")
    assert not _all_same(run("poison"), ref)
    for layout in LAYOUTS:
        assert _all_same(run(layout), ref), layout
        run("poison")
    assert _all_same(run("f32"), ref)
    return ref


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_refine_sequence_on_bytes(shape, lanes):
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    H, W = 30, 45
    _, S, T, ring, wpc, tpos = shape
    e = Engine(H, W, 8, lanes=lanes)
    s = _sequence(T, H, W)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3, refine=_lib.REFINE_POSE_SCALE)
    run = lambda k: e.refine_sequence(s[k], s["depths"], s["K"], p0, o, sources=S, ring=ring, log_scale=True, windows_per_call=wpc, target_pos=tpos)
    pose, ls = _check(run)
    assert not _same(pose, p0) and float(ls.abs().max()) > 0                   # (something was refined)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_refine_dense_sequence_on_bytes(shape, lanes):
    """the mode with no other stage on the pack stream: the conversion alone runs there, and writes the raw mirror slots"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    H, W = 30, 45
    _, S, T, ring, wpc, tpos = shape
    e = Engine(H, W, 8, lanes=lanes)
    s = _sequence(T, H, W)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=2)
    run = lambda k: e.refine_dense_sequence(s[k], s["depths"], s["K"], p0, o, sources=S, ring=ring, windows_per_call=wpc, target_pos=tpos)
    pose, maps = _check(run)
    assert not _same(pose, p0) and float(maps.std()) > 0


@functools.lru_cache(maxsize=None)
def _depth_params():
    import depthnet_twin
    return depthnet_twin.depthnet_params(0)


@functools.lru_cache(maxsize=None)
def _pose_params():
    import standins
    return standins.posenet_params(5)


@pytest.mark.parametrize("attached", [False, True], ids=["depths_given", "frames_only"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_odometry_sequence_on_bytes(shape, lanes, attached):
    """depths given: the PoseNet reads the converted raw frames, mirror slots included.  frames only (a depth network attached): the
    depth stage reads them too."""
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    H, W = 32, 64
    _, S, T, ring, wpc, tpos = shape
    e = Engine(H, W, 8, lanes=lanes)
    pn = PoseNetHIP(e, 8, _pose_params())
    if attached:
        dn = DepthNetHIP(e, 8, _depth_params())
        e.attach_depthnet(dn)
    s = _sequence(T, H, W)
    o = default_opts(n_iters=3, argmin=1)
    depths = None if attached else s["depths"]
    run = lambda k: pn.odometry_sequence(s[k], depths, s["K"], o, sources=S, iterations=2, ring=ring, windows_per_call=wpc, target_pos=tpos)
    init, out = _check(run)
    assert not _same(init, out) and float(init.abs().max()) > 0


def test_run_native_takes_bytes():
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    H, W, T, S = 30, 45, 7, 1
    e = Engine(H, W, 8)
    s = _sequence(T, H, W)
    p0 = _init_poses(T, S)
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, default_opts(n_iters=3), S
    ref = sr.run_native(s["f32"], s["depths"], s["K"], p0)
    assert _same(sr.run_native(s["hwc"], s["depths"], s["K"], p0), ref)
    assert _same(sr.run_native(s["hwc"].numpy(), s["depths"], s["K"], p0), ref)
    assert not _same(ref, p0)


def test_format_setting_contract():
    """the C entry itself: sticky, an unknown format is refused and changes nothing, the overlap check counts bytes"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    H, W, T, S = 30, 45, 7, 1
    e = Engine(H, W, 8)
    lib = e.lib
    err = lambda: lib.tcsfm_last_error(e._h).decode()
    s = _sequence(T, H, W)
    p0 = _init_poses(T, S)
    o = default_opts(n_iters=3)
    Kc = torch.as_tensor(s["K"])
    hp = lambda t: C.c_void_p(t.data_ptr())

    def c_call(frames, pose_out=None):
        out = torch.zeros_like(p0) if pose_out is None else pose_out
        e._bind()
        return lib.tcsfm_refine_sequence(e._h, C.byref(o), T, S, hp(frames), hp(s["depths"]), hp(Kc), hp(p0), hp(out), None, 0, 2, 0), out

    rc, ref = c_call(s["f32"])
    assert rc == 0 and not _same(ref, p0)
    # an unknown format on a new handle: refused, and a float call still returns its bits
    assert lib.tcsfm_sequence_frame_format(e._h, 3) == E_ARG and "tcsfm_sequence_frame_format" in err()
    assert lib.tcsfm_sequence_frame_format(e._h, -1) == E_ARG
    rc, got = c_call(s["f32"])
    assert rc == 0 and _same(got, ref)
    # sticky: two byte calls after one setting; an unknown format in between leaves it as it is
    assert lib.tcsfm_sequence_frame_format(e._h, U8_HWC) == 0
    rc, got = c_call(s["hwc"])
    assert rc == 0 and _same(got, ref)
    assert lib.tcsfm_sequence_frame_format(e._h, 99) == E_ARG
    rc, got = c_call(s["hwc"])
    assert rc == 0 and _same(got, ref)
    # the frames range is T*3*H*W BYTES now: an output right behind the bytes is disjoint, one on their last byte is refused
    room = torch.zeros(T * 3 * H * W + p0.numel() * 4 + 8, dtype=torch.uint8).pin_memory()
    nb = T * 3 * H * W
    room[:nb].copy_(s["hwc"].reshape(-1))
    behind = (nb + 3) // 4 * 4
    out_behind = room[behind:behind + p0.numel() * 4].view(torch.float32).view(p0.shape)
    rc, got = c_call(room, out_behind)
    assert rc == 0 and _same(got, ref), err()
    assert bool((room[:nb] == s["hwc"].reshape(-1)).all())
    inside = (nb - 1) // 4 * 4
    out_inside = room[inside:inside + p0.numel() * 4].view(torch.float32).view(p0.shape)
    rc, _ = c_call(room, out_inside)
    assert rc == E_ARG and err() == "tcsfm_refine_sequence: pose_out overlaps frames"
    # back to floats: the float call's bits
    assert lib.tcsfm_sequence_frame_format(e._h, U8_CHW) == 0
    rc, got = c_call(s["chw"])
    assert rc == 0 and _same(got, ref)
    assert lib.tcsfm_sequence_frame_format(e._h, F32_CHW) == 0
    rc, got = c_call(s["f32"])
    assert rc == 0 and _same(got, ref)
