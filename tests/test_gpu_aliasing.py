"""The buffer-overlap contract of include/tcsfm.h ("overlapping arguments") on the raw C ABI, row by row of tests/alias_cases.py.

For every row the call first runs on disjoint buffers: the reference bits.  Then
  * every honoured pair: the same call with the output placed on the input returns TCSFM_OK and EVERY output has the reference bits;
    under opts.host_ptrs = 1 every (output, input) pair is honoured (the arrays are staged), with overlapping NumPy views;
  * every other (output, input) pair and every (output, output) pair, at the same base address and at an offset of half the smaller
    array: TCSFM_E_ARG, a message that names the entry and both arguments, both buffers keep their bits, and the handle stays usable
    (the next disjoint call gives the reference bits again).
Comparisons are on bits: the library is bit-reproducible and an honoured call has no excuse to differ."""
import ctypes as C

import numpy as np
import pytest

import alias_cases as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG = -1
QUEUED = ("tcsfm_refine_window_queued", "tcsfm_refine_window_scale_queued", "tcsfm_refine_dense_window_queued")


def _sentinel(p, nbytes=None):
    n = (p.nbytes if nbytes is None else nbytes) // p.dtype.itemsize
    return np.full(n, -7.0, p.dtype).view(np.uint8)


class Mem:
    """a range of bytes in device memory (a torch uint8 tensor) or host memory (a NumPy uint8 array)"""
    def __init__(self, data, host):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.host = host
        self.buf = data.copy() if host else torch.from_numpy(data.copy()).cuda()

    @property
    def ptr(self):
        return self.buf.ctypes.data if self.host else self.buf.data_ptr()

    def bytes(self):
        return self.buf.copy() if self.host else self.buf.cpu().numpy()


class Harness:
    """one handle and the disjoint buffers of one row; run() calls the entry with an optional alias (out, other, offset in bytes)"""
    def __init__(self, row, host=False):
        from tightly_coupled_sfm_amd import _lib
        from tightly_coupled_sfm_amd.engine import Engine
        self.row, self.host = row, host
        self.mem_host = host or row.runner == "sequence"          # the sequence calls take host arrays in every mode
        self.e = Engine(*row.hw, row.max_pairs)
        self.e._bind()
        if row.lane:
            self.e.set_lanes(2)
        if row.entry in QUEUED:
            self.e._call(self.e.lib.tcsfm_set_coalesce(self.e._h, 4))
        self.o = _lib.default_opts(**row.opts)
        self.o.host_ptrs = 1 if (host and row.runner != "sequence") else 0
        self.init = {p.name: (np.ascontiguousarray(p.gen(p)).view(np.uint8).reshape(-1) if p.role == A.IN else _sentinel(p)) for p in row.params}
        self.base = {p.name: Mem(self.init[p.name], self._where(p)) for p in row.params}

    def _where(self, p):
        return True if p.role == A.HOST_OUT else self.mem_host

    def close(self):
        self.e.close()

    def error(self):
        return self.e.lib.tcsfm_last_error(self.e._h).decode()

    def run(self, alias=None):
        """-> (rc, {output name: bytes}, arena bytes before, arena bytes after); the arena is the buffer an aliased pair shares"""
        row, e = self.row, self.e
        ptr = {k: m.ptr for k, m in self.base.items()}
        arena = before = None
        if alias:
            out, other, off = alias
            po, px = row.param(out), row.param(other)
            size = max(px.nbytes, off + po.nbytes)
            data = np.empty(size, np.uint8)
            data[:] = np.resize(_sentinel(po, 8), size)          # (float32 and float64 sentinels repeat every 8 bytes)
            if px.role != A.IN:
                data[:px.nbytes] = _sentinel(px)
            else:
                data[:px.nbytes] = self.init[other]
            arena = Mem(data, self._where(po))
            before = data.copy()
            ptr[other], ptr[out] = arena.ptr, arena.ptr + off
        cargs = [C.c_void_p(ptr[a.name]) if isinstance(a, A.P) else a for a in row.args]
        head = [e._h] + ([row.lane] if row.lane else []) + [C.byref(self.o)]
        if not self.mem_host:
            torch.cuda.synchronize()
        rc = getattr(e.lib, row.entry)(*head, *cargs)
        if rc == 0 and row.entry in QUEUED:
            rc = e.lib.tcsfm_flush(e._h)
        if rc == 0 and row.lane:
            rc = e.lib.tcsfm_lane_synchronize(e._h, row.lane)
        sync = e.lib.tcsfm_synchronize(e._h)
        torch.cuda.synchronize()
        rc = rc or sync
        outs = {}
        after = arena.bytes() if arena else None
        for p in row.params:
            if p.role == A.IN:
                continue
            if alias and p.name == alias[0]:
                outs[p.name] = after[alias[2]:alias[2] + p.nbytes]
            elif alias and p.name == alias[1]:
                outs[p.name] = after[:p.nbytes]
            else:
                outs[p.name] = self.base[p.name].bytes()
        return rc, outs, before, after

    def reset_outputs(self):
        for p in self.row.params:
            if p.role != A.IN:
                self.base[p.name] = Mem(self.init[p.name], self._where(p))


def _same_space(row, a, b, host):
    """can the two parameters share memory in this mode?  HOST_OUT arrays live on the host, the others where the mode puts them"""
    ha = a.role == A.HOST_OUT or host or row.runner == "sequence"
    hb = b.role == A.HOST_OUT or host or row.runner == "sequence"
    return ha == hb


def _offsets(po, px):
    half = (min(po.nbytes, px.nbytes) // 2) // 8 * 8
    return [0] + ([half] if half else [])


def _pairs_of(row, host):
    """(out, other, offset, honoured) over every (out, in) and (out, out) pair that can share memory in this mode"""
    outs = [p for p in row.params if p.role in (A.OUT, A.HOST_OUT)]
    for i, po in enumerate(outs):
        for px in row.params:
            if px is po or px.role == A.HOST_IN or (px.role != A.IN and outs.index(px) < i) or not _same_space(row, po, px, host):
                continue
            for off in _offsets(po, px):
                io = px.role == A.IN
                ok = io and (row.is_honoured(po.name, px.name, off == 0) or (host and row.runner != "sequence"))
                yield po.name, px.name, off, ok


def _assert_same(got, ref, what):
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, int(np.count_nonzero(got[k] != ref[k])), "bytes differ")


def _reference(hs, row):
    rc, ref, _, _ = hs.run()
    assert rc == 0, (row.entry, hs.error())
    for p in row.params:          # the call wrote every output: no sentinel survives whole, and something finite came out
        if p.role != A.IN:
            v = ref[p.name].view(p.dtype)
            assert np.isfinite(v).any() and not np.array_equal(ref[p.name], _sentinel(p)), (row.entry, p.name)
    hs.reset_outputs()
    return ref


GENERIC = [r for r in A.ROWS if r.runner in ("generic", "sequence")]
DEVICE_ONLY = QUEUED + ("tcsfm_refine_window_async", "tcsfm_refine_dense_window_async")


@pytest.mark.parametrize("row", GENERIC, ids=A.row_id)
def test_honoured_pairs_keep_the_bits(row):
    modes = [False] + ([True] if row.entry not in DEVICE_ONLY and row.runner != "sequence" else [])
    for host in modes:
        hs = Harness(row, host)
        ref = _reference(hs, row)
        n = 0
        for out, other, off, ok in _pairs_of(row, host):
            if not ok:
                continue
            rc, got, _, _ = hs.run((out, other, off))
            assert rc == 0, (row.entry, host, out, other, off, hs.error())
            _assert_same(got, ref, (row.entry, "host" if host else "device", out, other, off))
            hs.reset_outputs()
            n += 1
        assert n >= len(row.honoured), (row.entry, n)
        hs.close()


@pytest.mark.parametrize("row", GENERIC, ids=A.row_id)
def test_everything_else_is_refused(row):
    modes = [False] + ([True] if row.entry not in DEVICE_ONLY and row.runner != "sequence" else [])
    n = 0
    for host in modes:
        hs = Harness(row, host)
        ref = _reference(hs, row)
        for out, other, off, ok in _pairs_of(row, host):
            if ok:
                continue
            rc, _, before, after = hs.run((out, other, off))
            msg = hs.error()
            what = (row.entry, "host" if host else "device", out, other, off, rc, msg)
            assert rc == E_ARG, what
            assert msg.startswith(row.entry + ": ") and " overlaps " in msg, what
            assert {out, other} == set(msg[len(row.entry) + 2:].split(" overlaps ")), what
            assert np.array_equal(before, after), what          # both buffers keep their pre-call bits
            n += 1
        outs = [p for p in row.params if p.role != A.IN]
        # nothing else was touched either, and the handle is usable: the next disjoint call gives the reference bits
        for p in outs:
            assert np.array_equal(hs.base[p.name].bytes(), hs.init[p.name]), (row.entry, p.name)
        rc, got, _, _ = hs.run()
        assert rc == 0, (row.entry, hs.error())
        _assert_same(got, ref, (row.entry, "after the refusals"))
        hs.close()
    # (an entry whose only output lives on the host has nothing a device input could overlap, and host staging honours the rest)
    assert n >= 1 or all(p.role == A.HOST_OUT for p in row.params if p.role != A.IN), row.entry


# ---- the dense window mode: depth_out on the depth inputs, every form ------------------------------------------------------------------
def _dense_row(opts):
    base = A.rows_for("tcsfm_refine_dense_window")[0]
    return A.Row(base.entry, base.args, base.honoured, dict(opts), base.hw, "generic", base.max_pairs)


DENSE_FORMS = {"pair": dict(window_rule=0, dense_joint=0, argmin=1), "joint": dict(window_rule=0, dense_joint=1, argmin=1),
               "reference": dict(window_rule=1, w_dc=0.15, argmin=1), "reference_quarter": dict(window_rule=1, w_dc=0.15, argmin=1, depth_param=1)}


@pytest.mark.parametrize("n_iters", [0, 2])
@pytest.mark.parametrize("form", list(DENSE_FORMS))
def test_dense_window_honoured(form, n_iters):
    """tcsfm_refine_dense_window with depth_out == depth_t, == depth_s and one map into depth_s, device pointers and host views: B = 2,
    S = 2 (at B = 1 the forward slot of depth_out and depth_t hold the same map, which hides an early write).

    What proves the reference mode's fix is the OFFSET case (one map into depth_s; the queued half-way case of the generic runner is the
    other): there a workgroup of the pack writes a slot that another workgroup still reads.  At the base address of depth_s the thread
    of k_pack that writes output slot n has itself read source map n before, and at the base of depth_t the slots receive the values
    they already hold, so those two cases keep their bits with or without the fix: they pin the contract, not the race."""
    row = _dense_row(dict(DENSE_FORMS[form], n_iters=n_iters))
    H, W = row.hw
    one_map = H * W * 4
    for host in (False, True):
        hs = Harness(row, host)
        ref = _reference(hs, row)
        for other, off in (("depth_t", 0), ("depth_s", 0), ("depth_s", one_map), ("pose_in", 0)):
            out = "pose_out" if other == "pose_in" else "depth_out"
            rc, got, _, _ = hs.run((out, other, off))
            assert rc == 0, (form, n_iters, host, other, off, hs.error())
            _assert_same(got, ref, (form, n_iters, "host" if host else "device", other, off))
            hs.reset_outputs()
        if not host:          # depth_out over any other input is refused
            rc, _, before, after = hs.run(("depth_out", "srcs", 0))
            assert rc == E_ARG and "depth_out overlaps srcs" in hs.error() and np.array_equal(before, after), hs.error()
        hs.close()


@pytest.mark.parametrize("form", ["pair_s1", "reference"])
def test_two_queued_dense_calls_one_aliased(form):
    """two queued dense calls of a mergeable kind, the second with depth_out on its own depth_s: it is honoured by running at once
    (after flushing the first), and both calls return the bits of the plain call"""
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine
    H, W = A.PAIR_HW
    B, S = (2, 1) if form == "pair_s1" else (2, 2)
    N = 2 * B * S
    w = A._window(B, S)
    o = _lib.default_opts(n_iters=2, argmin=1, **(dict(window_rule=0) if form == "pair_s1" else dict(window_rule=1, w_dc=0.15)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    ins = lambda: [t(w[k]) for k in ("tgt", "srcs", "depth_t", "depth_s", "K", "pose")]
    e = Engine(H, W, 4 * N)
    e._bind()
    p = lambda x: C.c_void_p(x.data_ptr())
    a = ins()
    pose_ref, depth_ref = torch.full((N, 6), -7.0, device="cuda"), torch.full((N, 1, H, W), -7.0, device="cuda")
    torch.cuda.synchronize()
    e._call(e.lib.tcsfm_refine_dense_window(e._h, C.byref(o), B, S, *[p(x) for x in a], p(pose_ref), p(depth_ref), None))
    e._call(e.lib.tcsfm_synchronize(e._h))
    e._call(e.lib.tcsfm_set_coalesce(e._h, 4))
    a1, a2 = ins(), ins()
    pose1, depth1, pose2 = torch.full((N, 6), -7.0, device="cuda"), torch.full((N, 1, H, W), -7.0, device="cuda"), torch.full((N, 6), -7.0, device="cuda")
    arena = torch.full((N, 1, H, W), -7.0, device="cuda")          # call 2: depth_s and depth_out share it
    arena[:S * B] = a2[3].reshape(S * B, 1, H, W)
    torch.cuda.synchronize()
    b0, c0 = C.c_int(0), C.c_int(0)
    e._call(e.lib.tcsfm_coalesce_counts(e._h, C.byref(b0), C.byref(c0)))
    e._call(e.lib.tcsfm_refine_dense_window_queued(e._h, C.byref(o), B, S, *[p(x) for x in a1], p(pose1), p(depth1)))
    args2 = [p(x) for x in a2]
    args2[3] = p(arena)
    e._call(e.lib.tcsfm_refine_dense_window_queued(e._h, C.byref(o), B, S, *args2, p(pose2), p(arena)))
    e._call(e.lib.tcsfm_flush(e._h))
    e._call(e.lib.tcsfm_synchronize(e._h))
    torch.cuda.synchronize()
    b1, c1 = C.c_int(0), C.c_int(0)
    e._call(e.lib.tcsfm_coalesce_counts(e._h, C.byref(b1), C.byref(c1)))
    assert (b1.value - b0.value, c1.value - c0.value) == (1, 1)          # the first call ran as a sequence of its own, the aliased one plainly
    bits = lambda x: x.cpu().numpy().view(np.uint8)
    for got, ref in ((pose1, pose_ref), (depth1, depth_ref), (pose2, pose_ref), (arena, depth_ref)):
        assert np.array_equal(bits(got), bits(ref))
    assert np.isfinite(depth_ref.cpu().numpy()).all() and not (depth_ref == -7.0).any()
    e.close()


# ---- the networks and the optimiser: every output against the largest input, and two outputs on each other -------------------------------
def _refused(e, rc, entry, a, b):
    msg = e.lib.tcsfm_last_error(e._h).decode()
    assert rc == E_ARG and msg.startswith(entry + ": ") and " overlaps " in msg, (entry, rc, msg)
    named = {s.split("[")[0] for s in msg[len(entry) + 2:].split(" overlaps ")}
    assert named == {a, b}, (entry, msg, a, b)


def test_networks_refuse():
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP, named_table, SKIP_CHANNELS
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    import depthnet_twin
    import standins
    H, W = A.NET_HW
    N = 2
    e = Engine(H, W, 16)
    e._bind()
    lib = e.lib
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    z = lambda *s: torch.full(s, -7.0, device="cuda")
    rng = np.random.default_rng(2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    unchanged = lambda x: bool((x == -7.0).all())

    # -- PoseNet
    pn = PoseNetHIP(e, 8, standins.posenet_params(1))
    imgs6 = t(rng.uniform(0, 1, size=(N, 6, H, W)))
    keep = imgs6.clone()
    _refused(e, lib.tcsfm_posenet_forward(pn._pn, N, p(imgs6), p(imgs6, 64)), "tcsfm_posenet_forward", "pose_out", "imgs")
    tape_n = pn.tape_size(N)
    tape = z(tape_n)
    _refused(e, lib.tcsfm_posenet_forward_train(pn._pn, N, p(imgs6), p(imgs6), p(tape)), "tcsfm_posenet_forward_train", "pose_out", "imgs")
    big = z(max(tape_n, imgs6.numel()))
    big[:imgs6.numel()] = imgs6.reshape(-1)
    po6 = z(N, 6)
    _refused(e, lib.tcsfm_posenet_forward_train(pn._pn, N, p(big), p(po6), p(big)), "tcsfm_posenet_forward_train", "tape", "imgs")
    _refused(e, lib.tcsfm_posenet_forward_train(pn._pn, N, p(imgs6), p(tape, 16), p(tape)), "tcsfm_posenet_forward_train", "pose_out", "tape")
    pose, tape = pn.forward_train(imgs6)
    d_pose, tape0 = t(rng.normal(size=(N, 6))), tape.clone()
    _refused(e, lib.tcsfm_posenet_backward(pn._pn, N, p(tape), p(d_pose), p(tape)), "tcsfm_posenet_backward", "d_imgs", "tape")
    nul7 = (C.c_void_p * 7)()
    w1 = z(16, 6, 7, 7)
    tab = (C.c_void_p * 7)(); tab[0] = w1.data_ptr()
    tab_t = (C.c_void_p * 7)(); tab_t[0] = tape.data_ptr()
    d_imgs = z(N, 6, H, W)
    _refused(e, lib.tcsfm_posenet_param_backward(pn._pn, N, p(imgs6), p(tape), p(d_pose), p(tape), nul7, nul7, nul7, nul7, None, None),
             "tcsfm_posenet_param_backward", "d_imgs", "tape")
    for k in range(4):          # conv_w_g, conv_b_g, gn_w_g, gn_b_g [0] on the tape
        tabs = [nul7] * 4
        tabs[k] = tab_t
        _refused(e, lib.tcsfm_posenet_param_backward(pn._pn, N, p(imgs6), p(tape), p(d_pose), p(d_imgs), *tabs, None, None),
                 "tcsfm_posenet_param_backward", ("conv_w_g", "conv_b_g", "gn_w_g", "gn_b_g")[k], "tape")
    _refused(e, lib.tcsfm_posenet_param_backward(pn._pn, N, p(imgs6), p(tape), p(d_pose), p(d_imgs), nul7, nul7, nul7, nul7, p(tape), None),
             "tcsfm_posenet_param_backward", "head_w_g", "tape")
    _refused(e, lib.tcsfm_posenet_param_backward(pn._pn, N, p(imgs6), p(tape), p(d_pose), p(d_imgs), nul7, nul7, nul7, nul7, None, p(tape, 32)),
             "tcsfm_posenet_param_backward", "head_b_g", "tape")
    _refused(e, lib.tcsfm_posenet_param_backward(pn._pn, N, p(imgs6), p(tape), p(d_pose), p(d_imgs), tab, tab, nul7, nul7, None, None),
             "tcsfm_posenet_param_backward", "conv_w_g", "conv_b_g")
    B, S = 1, 2
    w = A._window(B, S)          # frames of the pair size: only the refusal is exercised, on a handle of the network size
    tg, sr = t(rng.uniform(0, 1, size=(B, 3, H, W))), t(rng.uniform(0, 1, size=(S, B, 3, H, W)))
    dt_, ds_, K = t(rng.uniform(1, 2, size=(B, 1, H, W))), t(rng.uniform(1, 2, size=(S, B, 1, H, W))), t(w["K"])
    sr0 = sr.clone()
    _refused(e, lib.tcsfm_solve_pose_iteratively(e._h, pn._pn, 2, B, S, p(tg), p(sr), p(dt_), p(ds_), p(K), p(sr), None),
             "tcsfm_solve_pose_iteratively", "poses_out", "srcs")
    po = z(2 * B * S, 6)
    _refused(e, lib.tcsfm_solve_pose_iteratively(e._h, pn._pn, 2, B, S, p(tg), p(sr), p(dt_), p(ds_), p(K), p(po), p(sr, 128)),
             "tcsfm_solve_pose_iteratively", "stacked_out", "srcs")
    _refused(e, lib.tcsfm_solve_pose_iteratively(e._h, pn._pn, 2, B, S, p(tg), p(sr), p(dt_), p(ds_), p(K), p(po), p(po)),
             "tcsfm_solve_pose_iteratively", "poses_out", "stacked_out")
    # the odometry sequence: host arrays, two outputs on each other and an output on the frames
    T = 4
    from tightly_coupled_sfm_amd import _lib
    o = _lib.default_opts(n_iters=1)
    frames, depths = rng.uniform(0, 1, size=(T, 3, H, W)).astype(np.float32), rng.uniform(1, 2, size=(T, 1, H, W)).astype(np.float32)
    depths0 = depths.copy()
    Kh = np.ascontiguousarray(w["K"][0], np.float32)
    nwin = T - S
    pout = np.full((nwin, 2 * S, 6), -7.0, np.float32)
    hp = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    f0 = frames.copy()
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kh), hp(pout), hp(pout), None, 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_init_out", "pose_out")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kh), None, hp(frames, 48), None, 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_out", "frames")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kh), hp(frames), hp(pout), None, 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_init_out", "frames")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(o), T, S, hp(frames), hp(depths), hp(Kh), hp(depths, 96), hp(pout), None, 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_init_out", "depths")
    # the log depth-scales are an output under TCSFM_REFINE_POSE_SCALE only
    os_ = _lib.default_opts(n_iters=1, refine=_lib.REFINE_POSE_SCALE)
    pinit = np.full((nwin, 2 * S, 6), -7.0, np.float32)
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(os_), T, S, hp(frames), hp(depths), hp(Kh), hp(pinit), hp(pout), hp(frames, 16), 0, 1, -1),
             "tcsfm_odometry_sequence", "log_scale_out", "frames")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(os_), T, S, hp(frames), hp(depths), hp(Kh), hp(pinit), hp(pout), hp(depths), 0, 1, -1),
             "tcsfm_odometry_sequence", "log_scale_out", "depths")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(os_), T, S, hp(frames), hp(depths), hp(Kh), hp(pinit), hp(pout), hp(pout, 24), 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_out", "log_scale_out")
    _refused(e, lib.tcsfm_odometry_sequence(e._h, pn._pn, 2, C.byref(os_), T, S, hp(frames), hp(depths), hp(Kh), hp(pinit), hp(pout), hp(pinit), 0, 1, -1),
             "tcsfm_odometry_sequence", "pose_init_out", "log_scale_out")
    torch.cuda.synchronize()
    assert np.array_equal(frames, f0) and np.array_equal(depths, depths0) and (pout == -7.0).all() and (pinit == -7.0).all()
    assert torch.equal(imgs6, keep) and torch.equal(tape, tape0) and torch.equal(sr, sr0) and unchanged(po) and unchanged(w1) and unchanged(d_imgs)
    pose_again = pn(imgs6)          # the handle and the network are usable
    assert torch.equal(pose_again, pose)

    # -- depth network
    sd = depthnet_twin.depthnet_params(3)
    dn = DepthNetHIP(e, N, sd)
    named = [(k, v.float().contiguous().cuda()) for k, v in sd.items() if not k.endswith("num_batches_tracked")]
    e._call(lib.tcsfm_depthnet_load_device(dn._dn, *named_table(named)))
    imgs = t(rng.uniform(0, 1, size=(N, 3, H, W)))
    imgs0 = imgs.clone()
    disp_ref = dn.forward(imgs)
    shapes = [(N, H >> (k + 1), W >> (k + 1), c) for k, c in enumerate(SKIP_CHANNELS)]
    skips = [z(*s) for s in shapes]
    sk_tab = lambda lst: C.cast((C.c_void_p * 5)(*[x if isinstance(x, int) else x.data_ptr() for x in lst]), C.c_void_p)
    on_imgs = list(skips); on_imgs[4] = imgs.data_ptr()          # skip 4 is the smallest: nested in imgs
    _refused(e, lib.tcsfm_depthnet_encode(dn._dn, N, p(imgs), 0, sk_tab(on_imgs)), "tcsfm_depthnet_encode", "skips_out", "imgs")
    twice = list(skips); twice[4] = skips[3].data_ptr()
    _refused(e, lib.tcsfm_depthnet_encode(dn._dn, N, p(imgs), 0, sk_tab(twice)), "tcsfm_depthnet_encode", "skips_out", "skips_out")
    _refused(e, lib.tcsfm_depthnet_forward(dn._dn, N, p(imgs), 0, p(imgs, 4 * H * W)), "tcsfm_depthnet_forward", "disp_out", "imgs")
    real = dn.encode(imgs)
    real0 = [s.clone() for s in real]
    _refused(e, lib.tcsfm_depthnet_decode(dn._dn, N, sk_tab(real), p(real[0])), "tcsfm_depthnet_decode", "disp_out", "skips_in")
    te, td = C.c_int64(0), C.c_int64(0)
    e._call(lib.tcsfm_depthnet_tape_size(dn._dn, N, C.byref(te), C.byref(td)))
    tape_e, tape_d = z(te.value), z(td.value)
    _refused(e, lib.tcsfm_depthnet_encode_train(dn._dn, N, p(imgs), sk_tab(on_imgs), p(tape_e)), "tcsfm_depthnet_encode_train", "skips_out", "imgs")
    big_e = z(max(te.value, imgs.numel()))          # a buffer that starts with the images: the tape on its largest input
    big_e[:imgs.numel()] = imgs.reshape(-1)
    big_e0 = big_e.clone()
    _refused(e, lib.tcsfm_depthnet_encode_train(dn._dn, N, p(big_e), sk_tab(skips), p(big_e)), "tcsfm_depthnet_encode_train", "tape", "imgs")
    _refused(e, lib.tcsfm_depthnet_encode_train(dn._dn, N, p(big_e), sk_tab(skips), p(big_e, 4 * imgs.numel() // 2)), "tcsfm_depthnet_encode_train", "tape", "imgs")
    torch.cuda.synchronize()
    assert torch.equal(big_e, big_e0) and all(unchanged(x) for x in skips)
    on_tape = list(skips); on_tape[0] = tape_e.data_ptr()
    _refused(e, lib.tcsfm_depthnet_encode_train(dn._dn, N, p(imgs), sk_tab(on_tape), p(tape_e)), "tcsfm_depthnet_encode_train", "skips_out", "tape")
    _refused(e, lib.tcsfm_depthnet_decode_train(dn._dn, N, sk_tab(real), p(real[0]), p(tape_d)), "tcsfm_depthnet_decode_train", "disp_out", "skips_in")
    _refused(e, lib.tcsfm_depthnet_decode_train(dn._dn, N, sk_tab(real), p(tape_d, 256), p(tape_d)), "tcsfm_depthnet_decode_train", "disp_out", "tape")
    big_s = real[0]          # the largest input of the decoder
    in_s0 = [big_s] + real[1:]
    spare = z(N, 1, H, W)
    _refused(e, lib.tcsfm_depthnet_decode_train(dn._dn, N, sk_tab(in_s0), p(spare), p(big_s)), "tcsfm_depthnet_decode_train", "tape", "skips_in")
    # the backward passes: run the training forwards, then put each kind of output on the tape (their largest input)
    e._call(lib.tcsfm_depthnet_encode_train(dn._dn, N, p(imgs), sk_tab(skips), p(tape_e)))
    disp = z(N, 1, H, W)
    e._call(lib.tcsfm_depthnet_decode_train(dn._dn, N, sk_tab(skips), p(disp), p(tape_d)))
    torch.cuda.synchronize()
    assert torch.equal(disp, disp_ref) and all(torch.equal(a_, b_) for a_, b_ in zip(skips, real))
    te0, td0 = tape_e.clone(), tape_d.clone()
    d_disp = t(rng.normal(size=(N, 1, H, W)))
    dsk = [z(*s) for s in shapes]
    dname, ename = "iconvs.4.0.conv.weight", "encoder.encoder.conv1.weight"
    names = lambda *ks: C.cast((C.c_char_p * len(ks))(*[k.encode() for k in ks]), C.c_void_p)
    ptrs = lambda *xs: C.cast((C.c_void_p * len(xs))(*[x if isinstance(x, int) else x.data_ptr() for x in xs]), C.c_void_p)
    g_d, g_e = z(*sd[dname].shape), z(*sd[ename].shape)
    dsk_on = list(dsk); dsk_on[2] = tape_d.data_ptr()
    _refused(e, lib.tcsfm_depthnet_decode_backward(dn._dn, N, p(tape_d), p(d_disp), sk_tab(dsk_on), 0, None, None),
             "tcsfm_depthnet_decode_backward", "d_skips", "tape")
    _refused(e, lib.tcsfm_depthnet_decode_backward(dn._dn, N, p(tape_d), p(d_disp), sk_tab(dsk), 1, names(dname), ptrs(tape_d.data_ptr() + 64)),
             "tcsfm_depthnet_decode_backward", "grads", "tape")
    _refused(e, lib.tcsfm_depthnet_decode_backward(dn._dn, N, p(tape_d), p(d_disp), sk_tab(dsk), 1, names(dname), ptrs(dsk[0])),
             "tcsfm_depthnet_decode_backward", "grads", "d_skips")
    _refused(e, lib.tcsfm_depthnet_encode_backward(dn._dn, N, p(tape_e), sk_tab(dsk), 1, names(ename), ptrs(tape_e)),
             "tcsfm_depthnet_encode_backward", "grads", "tape")
    _refused(e, lib.tcsfm_depthnet_encode_backward(dn._dn, N, p(tape_e), sk_tab(dsk), 1, names(ename), ptrs(dsk[1])),
             "tcsfm_depthnet_encode_backward", "grads", "d_skips")
    torch.cuda.synchronize()
    assert torch.equal(imgs, imgs0) and torch.equal(tape_e, te0) and torch.equal(tape_d, td0) and all(torch.equal(a_, b_) for a_, b_ in zip(real, real0))
    assert all(unchanged(x) for x in dsk) and unchanged(g_d) and unchanged(g_e)
    # usable: the disjoint backward runs and the forward has its bits
    e._call(lib.tcsfm_depthnet_decode_backward(dn._dn, N, p(tape_d), p(d_disp), sk_tab(dsk), 1, names(dname), ptrs(g_d)))
    e._call(lib.tcsfm_depthnet_encode_backward(dn._dn, N, p(tape_e), sk_tab(dsk), 1, names(ename), ptrs(g_e)))
    torch.cuda.synchronize()
    assert not unchanged(g_d) and not unchanged(g_e) and torch.isfinite(g_d).all() and torch.isfinite(g_e).all()
    assert torch.equal(dn.forward(imgs), disp_ref)
    e.close()


def test_optimiser_refuses():
    """three tensors of 5, 64 and 257 floats: two parameters sharing memory, a gradient on a parameter, the two moment outputs on each other"""
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine
    e = Engine(*A.NET_HW, 2)
    e._bind()
    lib = e.lib
    numel = [5, 64, 257]
    rng = np.random.default_rng(4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    params = [t(rng.normal(size=n)) for n in numel]
    grads = [t(rng.normal(size=n)) for n in numel]
    p0 = [x.clone() for x in params]
    tab = lambda xs: (C.c_void_p * 3)(*[x if isinstance(x, int) or x is None else x.data_ptr() for x in xs])
    nm = (C.c_int64 * 3)(*numel)
    lr = (C.c_double * 3)(1e-2, 1e-2, 1e-2)

    def create(ptrs):
        o = C.c_void_p()
        return lib.tcsfm_optim_create(e._h, _lib.OPTIM_ADAM, 3, tab(ptrs), nm, C.byref(o)), o

    rc, o = create([params[0], params[2].data_ptr() + 4 * 100, params[2]])          # tensor 1 nested in tensor 2
    _refused(e, rc, "tcsfm_optim_create", "params", "params")
    assert not o.value
    rc, o = create([params[2].data_ptr() + 4 * 255, params[1], params[2]])            # tensor 0 across the end of tensor 2: partial
    _refused(e, rc, "tcsfm_optim_create", "params", "params")
    rc, ref_o = create(params)
    assert rc == 0
    rc, opt = create(params)          # (a second optimiser over the same tensors is another call: outside the contract)
    assert rc == 0
    lib.tcsfm_optim_destroy(opt)
    step = lambda o_, g: lib.tcsfm_optim_step(o_, tab(g), lr, 0.9, 0.999, 1e-8)
    _refused(e, step(ref_o, [grads[0], params[1], grads[2]]), "tcsfm_optim_step", "params", "grads")          # in-place gradient
    _refused(e, step(ref_o, [grads[0], grads[1], params[2].data_ptr() + 4]), "tcsfm_optim_step", "params", "grads")
    _refused(e, step(ref_o, [params[2].data_ptr() + 4 * 10, grads[1], grads[2]]), "tcsfm_optim_step", "params", "grads")   # tensor 0's gradient in tensor 2
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(params, p0))
    steps = C.c_int64(-1)
    m = torch.full((257,), -7.0, device="cuda")
    _refused(e, lib.tcsfm_optim_get_state(ref_o, 2, C.c_void_p(m.data_ptr()), C.c_void_p(m.data_ptr()), C.byref(steps)),
             "tcsfm_optim_get_state", "exp_avg_out", "exp_avg_sq_out")
    assert bool((m == -7.0).all())
    # usable, and no refused step counted: one real step equals the step of a fresh optimiser on copies
    assert step(ref_o, grads) == 0
    copies = [x.clone() for x in p0]
    rc, o2 = create(copies)
    assert rc == 0 and step(o2, grads) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(params, copies)) and not torch.equal(params[2], p0[2])
    e._call(lib.tcsfm_optim_get_state(ref_o, 2, None, None, C.byref(steps)))
    assert steps.value == 1
    lib.tcsfm_optim_destroy(ref_o); lib.tcsfm_optim_destroy(o2)
    e.close()
