"""The refusals of the drop-in operators and the evaluation entries on the raw C ABI: one table of rows (entry, what is wrong, expected
code, expected substring of tcsfm_last_error).  Per entry: NULL options, each required NULL array, a count out of range, the entry's own
refusals (depth_is_disp, no cotangent, no output wanted, more than 65535 planes, S outside 1 .. 4, negative w_dc, image too small,
host_ptrs != 0 for the device-only entry) and non-pinhole host intrinsics.  After EVERY refused call a valid call on the same handle
returns the bits it returned before: a refusal leaves nothing behind.  Refusals happen before anything is enqueued, so a refused call
launches nothing; every count the table plants is one the entry's first checks refuse whatever the arrays hold.

The arguments come from tests/alias_cases.py, rescaled to 5 x 7 (the smallest frame scale recovery accepts; hw & 3 == 3) and 17 x 33;
tcsfm_scale_recovery_frames, whose void pointers keep it out of that table, borrows tcsfm_scale_recovery's inputs.  The frame-preparation
entries (void pointers too; the entries that check alignment) have a table of their own at the end: host_ptrs != 0, misaligned pointers,
unknown formats, NULL arguments, N = 0 -- a refused call writes nothing, the valid call after it returns the same bits."""
import ctypes as C

import numpy as np
import pytest

import alias_cases as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG, E_INTRINSICS = -1, -3
SHAPES = [(5, 7), (17, 33)]
PAIR_NULL = ["src", "depth_t", "depth_s", "pose", "K"]
WL_FWD, WL_INV = ["fwd_diff", "fwd_valid", "fwd_weight", "fwd_auto_err"], ["inv_diff", "inv_valid", "inv_weight", "inv_auto_mask"]
WIN = "need 1 <="

# entry -> required arrays with the substring of their refusal; counts: (index into the row's args, value, substring); own: (what,
# keyword changes of the call, substring); intrinsics: the entry reads K
SPEC = {
    "tcsfm_disp_to_depth": dict(null={k: "bad argument" for k in ["disp"]}, no_opts="bad argument", counts=[(0, 0, "bad argument")]),
    "tcsfm_disp_to_depth_backward": dict(null={k: "bad argument" for k in ["disp", "g_disp"]}, no_opts="bad argument", counts=[(0, 0, "bad argument")],
                                         own=[("no cotangent", dict(null=["g_scaled", "g_depth"]), "no cotangent given")]),
    "tcsfm_ssim": dict(null={k: "bad argument" for k in ["x", "y", "out"]}, no_opts="bad argument", counts=[(0, 0, "bad argument")]),
    "tcsfm_ssim_backward": dict(null={k: "bad argument" for k in ["x", "y", "g_out"]}, no_opts="bad argument", counts=[(0, 0, "bad argument")],
                                own=[("no output wanted", dict(null=["g_x", "g_y"]), "no output wanted"),
                                     ("more than 65535 planes", dict(args={0: 65536}), "more than 65535 planes")]),
    "tcsfm_smooth_loss": dict(null={k: "NULL argument" for k in ["disp", "img", "loss_out"]}),
    "tcsfm_smooth_loss_device": dict(null={k: "NULL argument" for k in ["disp", "img", "loss_out", "stats_out"]}),
    "tcsfm_smooth_loss_backward": dict(null={k: "NULL argument" for k in ["disp", "img", "stats", "g_loss", "g_disp"]}),
    "tcsfm_window_loss": dict(null={**{k: "NULL forward map" for k in WL_FWD}, **{k: "NULL inverse map" for k in WL_INV}, "loss_out": "NULL output", "stats_out": "NULL output"},
                              counts=[(0, 0, "B must be at least 1"), (0, 8, "N out of range"), (1, 0, "S must be 1 .. 4"), (1, 5, "S must be 1 .. 4")],
                              own=[("negative w_dc", dict(opts=dict(w_dc=-0.5)), "w_dc must be >= 0")], row=1),
    "tcsfm_window_loss_backward": dict(null={**{k: "NULL forward map" for k in WL_FWD}, **{k: "NULL inverse map" for k in WL_INV}, "stats": "NULL argument", "g_loss": "NULL argument"},
                                       counts=[(0, 0, "B must be at least 1"), (0, 8, "N out of range"), (1, 0, "S must be 1 .. 4"), (1, 5, "S must be 1 .. 4")],
                                       own=[("negative w_dc", dict(opts=dict(w_dc=-0.5)), "w_dc must be >= 0"),
                                            ("no output wanted", dict(null=["g_fwd_diff", "g_fwd_weight", "g_inv_diff", "g_inv_weight"]), "no output requested")], row=1),
    "tcsfm_warp": dict(null={k: "NULL input" for k in PAIR_NULL}, own=[("depth_is_disp", dict(opts=dict(depth_is_disp=1)), "takes depth maps")], K=True),
    "tcsfm_warp_posenet_input": dict(null={k: "NULL argument" for k in ["tgt"] + PAIR_NULL + ["posenet_in"]},
                                     own=[("depth_is_disp", dict(opts=dict(depth_is_disp=1)), "takes depth maps")], K=True),
    "tcsfm_warp_backward": dict(null={k: "NULL input" for k in PAIR_NULL}, own=[("depth_is_disp", dict(opts=dict(depth_is_disp=1)), "takes depth maps")], K=True),
    "tcsfm_photometric_maps_backward": dict(null={k: "NULL input" for k in ["tgt", "img_rec", "proj_depth", "comp_depth"]}),
    "tcsfm_photometric_backward": dict(null={k: "NULL input" for k in ["tgt"] + PAIR_NULL},
                                       own=[("depth_is_disp", dict(opts=dict(depth_is_disp=1)), "takes depth maps")], K=True),
    "tcsfm_photometric": dict(null={k: "NULL input" for k in ["tgt"] + PAIR_NULL}, K=True),
    "tcsfm_linearize": dict(null={k: "NULL input" for k in ["tgt"] + PAIR_NULL}, K=True),
    "tcsfm_linearize_window": dict(null={k: "NULL input" for k in ["tgt", "srcs", "depth_t", "depth_s", "pose", "K"]},
                                   counts=[(0, 0, WIN), (1, 0, WIN), (0, 5, WIN)], K=True),
    "tcsfm_loss_surface": dict(null={k: "NULL argument" for k in ["tgt", "src", "depth_t", "depth_s", "poses", "K", "cost_out"]},
                               counts=[(5, 0, "N out of range"), (5, 9, "N out of range")], K=True),
    "tcsfm_linearize_dense_window": dict(null={k: "NULL argument" for k in ["tgt", "srcs", "depth_t", "depth_s", "K", "pose", "scal_out", "g_pose_out", "g_rho_out"]},
                                         counts=[(0, 0, "need 1 <= S <= 4"), (1, 0, "need 1 <= S <= 4"), (1, 5, "need 1 <= S <= 4"), (0, 5, "need 1 <= S <= 4")], K=True),
    "tcsfm_linearize_dense_window_sources": dict(null={k: "NULL argument" for k in ["tgt", "srcs", "depth_t", "depth_s", "K", "pose", "scal_out", "g_pose_out", "g_rho_out", "g_rho_src_out"]},
                                                 counts=[(0, 0, "need 1 <= S <= 4"), (1, 5, "need 1 <= S <= 4"), (0, 5, "need 1 <= S <= 4")], K=True),
    "tcsfm_scale_recovery": dict(null={k: "NULL argument" for k in ["depth", "K", "scale_out"]}, K=True),
    "tcsfm_scale_recovery_frames": dict(null={k: "NULL argument" for k in ["depth", "K", "scale_out"]},
                                        own=[("host_ptrs = 1", dict(opts=dict(host_ptrs=1)), "host_ptrs must be 0")]),
}
PAIR_COUNT = [(0, 0, "N out of range"), (0, 9, "N out of range")]      # max_pairs is 8


def _row(entry):
    if entry == "tcsfm_scale_recovery_frames":
        r = A.rows_for("tcsfm_scale_recovery")[0]
        n = r.args[0]
        return A.Row(entry, [n, r.param("depth"), r.param("K"), 1.65, A.P("scale_out", A.OUT, (n,)), A.P("median_out", A.OUT, (n,)),
                             A.P("count_out", A.OUT, (n,), np.int32)])
    return A.rows_for(entry)[SPEC[entry].get("row", 0)]


def _at(row, hw):
    """the row at another frame size: the arrays' extents follow, inputs whose shape changes are drawn afresh (seeded by their name)"""
    (H0, W0), (h, w) = row.hw, hw

    def shape(s):
        if len(s) >= 2 and tuple(s[-2:]) == (H0, W0):
            return tuple(s[:-2]) + (h, w)
        if s[-1] >= H0 * W0 and s[-1] % (H0 * W0) == 0:
            return tuple(s[:-1]) + (s[-1] // (H0 * W0) * h * w,)
        return tuple(s)

    args = []
    for i, a in enumerate(row.args):
        if isinstance(a, A.P):
            s = shape(a.shape)
            gen = a.gen if s == tuple(a.shape) else (A.g_mask if a.gen is A.g_mask else A.g_uniform(0.1, 0.9))
            a = A.P(a.name, a.role, s, a.dtype, gen)
        elif i == 0 and row.entry.startswith("tcsfm_disp_to_depth"):
            a = a // (H0 * W0) * h * w
        args.append(a)
    return A.Row(row.entry, args, row.honoured, row.opts, hw, row.runner, row.max_pairs)


class Harness:
    def __init__(self, row, host=False):
        from tightly_coupled_sfm_amd.engine import Engine
        self.row, self.host = row, host
        self.e = Engine(*row.hw, row.max_pairs)
        self.e._bind()
        self.init = {p.name: np.ascontiguousarray(p.gen(p)) for p in row.params if p.role == A.IN}

    def error(self):
        return self.e.lib.tcsfm_last_error(self.e._h).decode()

    def run(self, null=(), args=None, opts=None, no_opts=False, data=None):
        """-> (rc, {output: bytes}); null: arrays passed as NULL; args: {index: value} over the row's arguments; opts: option changes"""
        from tightly_coupled_sfm_amd import _lib
        o = _lib.default_opts(**{**self.row.opts, **(opts or {})})
        if "host_ptrs" not in (opts or {}):
            o.host_ptrs = 1 if self.host else 0
        keep, cargs = {}, []
        for i, a in enumerate(self.row.args):
            if not isinstance(a, A.P):
                cargs.append((args or {}).get(i, a))
                continue
            v = (data or {}).get(a.name, self.init.get(a.name))
            v = np.full(a.shape, -7.0, a.dtype) if v is None else v
            on_host = self.host or a.role == A.HOST_OUT
            keep[a.name] = np.array(v) if on_host else torch.from_numpy(np.array(v)).cuda()
            ptr = keep[a.name].ctypes.data if on_host else keep[a.name].data_ptr()
            cargs.append(None if a.name in null else C.c_void_p(ptr))
        torch.cuda.synchronize()
        rc = getattr(self.e.lib, self.row.entry)(self.e._h, None if no_opts else C.byref(o), *cargs)
        msg = self.error() if rc else ""
        sync = self.e.lib.tcsfm_synchronize(self.e._h)
        torch.cuda.synchronize()
        assert sync == 0, (self.row.entry, self.error())
        outs = {p.name: (keep[p.name] if isinstance(keep[p.name], np.ndarray) else keep[p.name].cpu().numpy()).tobytes()
                for p in self.row.params if p.role != A.IN and p.name not in null}
        return rc, msg, outs


def _refusals(entry):
    """the table's rows of one entry: (what, keyword arguments of Harness.run, code, substring)"""
    s = SPEC[entry]
    rows = [("NULL options", dict(no_opts=True), E_ARG, s.get("no_opts", "opts is NULL"))]
    rows += [(f"NULL {k}", dict(null=[k]), E_ARG, msg) for k, msg in s["null"].items()]
    rows += [(f"argument {i} = {v}", dict(args={i: v}), E_ARG, msg) for i, v, msg in s.get("counts", PAIR_COUNT)]
    rows += [(what, kw, E_ARG, msg) for what, kw, msg in s.get("own", [])]
    return rows


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("entry", sorted(SPEC))
def test_refusals_leave_nothing_behind(entry, hw):
    row = _at(_row(entry), hw)
    hs = Harness(row)
    rc, msg, ref = hs.run()
    assert rc == 0, (entry, msg)
    for p in row.params:          # the valid call wrote its outputs
        if p.role != A.IN:
            assert ref[p.name] != np.full(p.shape, -7.0, p.dtype).tobytes(), (entry, p.name)
    table = _refusals(entry)
    assert len(table) >= 2 + len(SPEC[entry]["null"])
    for what, kw, code, sub in table:
        rc, msg, _ = hs.run(**kw)
        assert rc == code and sub in msg, (entry, what, rc, msg)
        rc, msg, got = hs.run()
        assert rc == 0 and got == ref, (entry, "the valid call after", what, rc, msg)
    hs.e.close()
    if SPEC[entry].get("K"):          # non-pinhole HOST intrinsics: refused on the host, before anything is staged
        hs = Harness(row, host=True)
        rc, msg, ref = hs.run()
        assert rc == 0, (entry, msg)
        K = hs.init["K"].copy()
        K.reshape(-1, 9)[-1, 1] = 0.5
        rc, msg, _ = hs.run(data=dict(K=K))
        assert rc == E_INTRINSICS and "intrinsics must be pinhole" in msg, (entry, rc, msg)
        rc, msg, got = hs.run()
        assert rc == 0 and got == ref, (entry, "the valid call after non-pinhole intrinsics", rc, msg)
        hs.e.close()


@pytest.mark.parametrize("entry", ["tcsfm_scale_recovery", "tcsfm_scale_recovery_frames"])
def test_scale_recovery_refuses_a_frame_too_small(entry):
    """4 x 7 is a frame the handle takes and scale recovery does not; the handle's other entries go on working"""
    row = _at(_row(entry), (4, 7))
    hs = Harness(row)
    other = Harness.__new__(Harness)
    other.row, other.host, other.e = _at(_row("tcsfm_disp_to_depth"), (4, 7)), False, hs.e
    other.init = {p.name: np.ascontiguousarray(p.gen(p)) for p in other.row.params if p.role == A.IN}
    rc, msg, ref = other.run()
    assert rc == 0, msg
    rc, msg, _ = hs.run()
    assert rc == E_ARG and "image too small" in msg, (entry, rc, msg)
    rc, msg, got = other.run()
    assert rc == 0 and got == ref, (entry, rc, msg)
    hs.e.close()


# ---- the frame-preparation entries: device pointers only, and the ones that check alignment.  Their arrays are void pointers, so they are
# no rows of alias_cases.py either: the arguments are built here.
FRAME_TABLE = [
    # (entry, what is wrong, changes of the call's keyword arguments, substring)
    ("tcsfm_disp_post_process", "host_ptrs = 1", dict(host_ptrs=1), "host_ptrs must be 0"),
    ("tcsfm_disp_post_process", "l_disp off by two bytes", dict(shift=dict(l=2)), "must be aligned for float, out for double"),
    ("tcsfm_disp_post_process", "out off by four bytes", dict(shift=dict(out=4)), "must be aligned for float, out for double"),
    ("tcsfm_disp_post_process", "NULL r_disp_mirrored", dict(null=["r"]), "NULL argument"),
    ("tcsfm_disp_post_process", "NULL options", dict(no_opts=True), "NULL argument"),
    ("tcsfm_disp_post_process", "N = 0", dict(N=0), "N must be at least 1"),
    ("tcsfm_frames_from_u8", "host_ptrs = 1", dict(host_ptrs=1), "host_ptrs must be 0"),
    ("tcsfm_frames_from_u8", "dst off by two bytes", dict(shift=dict(dst=2)), "dst must be aligned for float"),
    ("tcsfm_frames_from_u8", "an unknown format", dict(format=7), "format must be"),
    ("tcsfm_frames_from_u8", "NULL src", dict(null=["src"]), "NULL argument"),
    ("tcsfm_frames_from_u8", "N = 0", dict(N=0), "N must be at least 1"),
    ("tcsfm_resize_u8", "host_ptrs = 1", dict(host_ptrs=1), "host_ptrs must be 0"),
    ("tcsfm_resize_u8", "a float dst off by two bytes", dict(shift=dict(dst=2)), "a float dst must be aligned for float"),
    ("tcsfm_resize_u8", "bytes out in the other layout", dict(dst_format=1), "dst_format must be"),
    ("tcsfm_resize_u8", "src_h = 0", dict(src_h=0), "src_h and src_w must be positive"),
    ("tcsfm_resize_u8", "NULL dst", dict(null=["dst"]), "NULL argument"),
    ("tcsfm_resize_u8", "N = 0", dict(N=0), "N must be at least 1"),
]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_preparation_refusals_leave_nothing_behind(hw):
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine
    (H, W), N = hw, 2
    sh, sw = 2 * H + 1, 2 * W + 3
    e = Engine(H, W, 8)
    e._bind()
    rng = np.random.default_rng(H * W)
    f = lambda *s: torch.from_numpy(rng.uniform(0.1, 0.9, size=s).astype(np.float32)).cuda()
    u = lambda *s: torch.from_numpy(rng.integers(0, 256, size=s, dtype=np.uint8)).cuda()
    ins = {"tcsfm_disp_post_process": dict(l=f(N, H, W), r=f(N, H, W)), "tcsfm_frames_from_u8": dict(src=u(N, 3, H, W)), "tcsfm_resize_u8": dict(src=u(N, 3, sh, sw))}
    out_bytes = {"tcsfm_disp_post_process": ("out", N * H * W * 8), "tcsfm_frames_from_u8": ("dst", N * 3 * H * W * 4), "tcsfm_resize_u8": ("dst", N * 3 * H * W * 4)}

    def run(entry, host_ptrs=0, shift=None, null=(), no_opts=False, **kw):
        """-> (rc, message, the output's bytes); a shifted pointer stays inside its allocation (16 spare bytes)"""
        o = _lib.default_opts()
        o.host_ptrs = host_ptrs
        name, nbytes = out_bytes[entry]
        out = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        bufs = dict(ins[entry], **{name: out})
        p = {k: (None if k in null else C.c_void_p(t.data_ptr() + (shift or {}).get(k, 0))) for k, t in bufs.items()}
        po, n = None if no_opts else C.byref(o), kw.get("N", N)
        torch.cuda.synchronize()
        if entry == "tcsfm_disp_post_process":
            rc = e.lib.tcsfm_disp_post_process(e._h, po, n, p["l"], p["r"], p["out"])
        elif entry == "tcsfm_frames_from_u8":
            rc = e.lib.tcsfm_frames_from_u8(e._h, po, kw.get("format", _lib.FRAMES_U8_HWC), n, p["src"], p["dst"])
        else:
            rc = e.lib.tcsfm_resize_u8(e._h, po, _lib.FRAMES_U8_HWC, n, kw.get("src_h", sh), sw, p["src"], kw.get("dst_format", _lib.FRAMES_F32_CHW), p["dst"])
        msg = e.lib.tcsfm_last_error(e._h).decode() if rc else ""
        assert e.lib.tcsfm_synchronize(e._h) == 0
        torch.cuda.synchronize()
        return rc, msg, out.cpu().numpy().tobytes()

    ref = {}
    for entry in ins:
        rc, msg, ref[entry] = run(entry)
        assert rc == 0 and ref[entry] != bytes([0xA5]) * len(ref[entry]), (entry, msg)
    for entry, what, kw, sub in FRAME_TABLE:
        rc, msg, got = run(entry, **kw)
        assert rc == E_ARG and sub in msg, (entry, what, rc, msg)
        assert got == bytes([0xA5]) * len(got), (entry, what, "the refused call wrote")
        rc, msg, got = run(entry)
        assert rc == 0 and got == ref[entry], (entry, "the valid call after", what, rc, msg)
    e.close()
