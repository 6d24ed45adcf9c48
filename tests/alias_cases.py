"""The buffer-overlap contract of include/tcsfm.h ("overlapping arguments") as a table: one row per ABI entry that takes array arguments.
A row names every pointer parameter of the prototype with its role and extent, lists the (out, in) pairs the contract honours and -- for
the entries the generic runner of tests/test_gpu_aliasing.py drives -- builds a small set of valid arguments.  Everything that is not
honoured is expected to be refused.  No GPU import here: tests/test_alias_cases_cpu.py checks the table against the header on any box."""
import numpy as np

IN, OUT, HOST_OUT = "in", "out", "host_out"      # HOST_OUT: written on the host in every mode (float64 results)
HOST_IN = "host_in"                              # a host-side table (learning rates, element counts, names): takes no part in overlap
SAME, ANY = "=", "~"                             # honoured: out at the base address of in / overlapping it in any way

PAIR_HW = (24, 40)        # pair and window entries
PLANE_HW = (17, 33)       # per-plane operators: odd sizes, more than one 256-thread block per plane
NET_HW = (32, 64)         # the networks (multiples of 32)
NSTAT = 10


class P:
    """a pointer parameter: header name, role, shape (None: a pointer array / table that the row's own test handles), dtype, generator"""
    def __init__(self, name, role, shape=None, dtype=np.float32, gen=None):
        self.name, self.role, self.shape, self.dtype, self.gen = name, role, shape, np.dtype(dtype), gen

    @property
    def nbytes(self):
        return int(np.prod(self.shape)) * self.dtype.itemsize


class Row:
    """entry: the function; args: what follows (handle, opts) in call order, P for a pointer parameter and a plain value for a scalar;
    honoured: [(out, in, SAME | ANY)]; opts: keyword arguments of default_opts; hw: the handle's frame size; lane: the lane of an _async
    entry; runner: "generic" / "sequence" (test_gpu_aliasing drives the row from this table: device or host arrays), or the name of
    the dedicated test that does."""
    def __init__(self, entry, args, honoured=(), opts=None, hw=PAIR_HW, runner="generic", max_pairs=8, takes_opts=True, lane=None):
        self.entry, self.args, self.honoured, self.opts, self.hw = entry, args, list(honoured), dict(opts or {}), hw
        self.runner, self.max_pairs, self.takes_opts, self.lane = runner, max_pairs, takes_opts, lane

    @property
    def params(self):
        return [a for a in self.args if isinstance(a, P)]

    def param(self, name):
        return next(p for p in self.params if p.name == name)

    def is_honoured(self, out, other, same_base):
        return any(o == out and i == other and (k == ANY or same_base) for o, i, k in self.honoured)


# ---- input generators (seeded: the arguments of a row are the same in every run)
def _rng(tag):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(tag)))


def g_uniform(lo, hi):
    return lambda p: _rng(p.name).uniform(lo, hi, size=p.shape).astype(p.dtype)


def g_normal(scale=1.0):
    return lambda p: (_rng(p.name).normal(size=p.shape) * scale).astype(p.dtype)


def g_mask(p):
    return (_rng(p.name).uniform(size=p.shape) > 0.3).astype(p.dtype)


def g_const(values):
    return lambda p: np.broadcast_to(np.asarray(values, p.dtype), p.shape).copy()


_CACHE = {}


def _pairs(N=2):
    from tightly_coupled_sfm_amd import synth
    if ("pairs", N) not in _CACHE:
        _CACHE[("pairs", N)] = synth.make_batch(N, *PAIR_HW, seed0=5, both_directions=True)
    return _CACHE[("pairs", N)]


def _window(B, S, seed=11):
    """B targets of S sources each, as tests/test_gpu_host_pointers.py builds them"""
    from tightly_coupled_sfm_amd import synth
    if ("win", B, S) in _CACHE:
        return _CACHE[("win", B, S)]
    H, W = PAIR_HW
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0 if s == 0 else -1.0)
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base, dtype=np.float32)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"][None] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"][None] * (1.0 + 0.01 * s)); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    w = dict(tgt=np.stack(tg), srcs=np.stack([np.stack(x) for x in sr]), depth_t=np.stack(dt),
             depth_s=np.stack([np.stack(x) for x in ds]), K=np.stack(K), pose=np.concatenate([fwd, -fwd]).astype(np.float32))
    _CACHE[("win", B, S)] = w
    return w


def g_pair(key, N=2):
    return lambda p: np.ascontiguousarray(_pairs(N)[key], np.float32).reshape(p.shape)


def g_win(key, B, S):
    return lambda p: np.ascontiguousarray(_window(B, S)[key], np.float32).reshape(p.shape)


def g_seq(key, T):
    def gen(p):
        from tightly_coupled_sfm_amd import synth
        if ("seq", T) not in _CACHE:
            _CACHE[("seq", T)] = synth.make_sequence(T, *PAIR_HW, seed=3)
        q = _CACHE[("seq", T)]
        if key == "K":
            return np.ascontiguousarray(q["K"], np.float32).reshape(p.shape)
        return np.ascontiguousarray(q[key], np.float32).reshape(p.shape)
    return gen


# ---- the rows
def _pair_inputs(N, tgt=True):
    H, W = PAIR_HW
    a = [P("tgt", IN, (N, 3, H, W), gen=g_pair("tgt", N))] if tgt else []
    return a + [P("src", IN, (N, 3, H, W), gen=g_pair("src", N)), P("depth_t", IN, (N, 1, H, W), gen=g_pair("depth_t", N)),
                P("depth_s", IN, (N, 1, H, W), gen=g_pair("depth_s", N))]


def _pose_K(N, pose="pose"):
    return [P(pose, IN, (N, 6), gen=g_pair("pose_init", N)), P("K", IN, (N, 3, 3), gen=g_pair("K", N))]


def _win_inputs(B, S, pose):
    H, W = PAIR_HW
    return [P("tgt", IN, (B, 3, H, W), gen=g_win("tgt", B, S)), P("srcs", IN, (S, B, 3, H, W), gen=g_win("srcs", B, S)),
            P("depth_t", IN, (B, 1, H, W), gen=g_win("depth_t", B, S)), P("depth_s", IN, (S, B, 1, H, W), gen=g_win("depth_s", B, S)),
            P("K", IN, (B, 3, 3), gen=g_win("K", B, S)), P(pose, IN, (2 * S * B, 6), gen=g_win("pose", B, S))]


def _rows():
    H, W = PAIR_HW
    h, w = PLANE_HW
    N = 2
    n = N * h * w
    rows = []
    add = rows.append
    pl = dict(hw=PLANE_HW)

    # -- the drop-in operators, per plane
    add(Row("tcsfm_disp_to_depth", [n, P("disp", IN, (n,), gen=g_uniform(0.05, 0.95)), P("scaled_disp", OUT, (n,)), P("depth", OUT, (n,))],
            honoured=[("scaled_disp", "disp", SAME), ("depth", "disp", SAME)], **pl))
    add(Row("tcsfm_ssim", [3 * N, P("x", IN, (3 * N, h, w), gen=g_uniform(0, 1)), P("y", IN, (3 * N, h, w), gen=g_uniform(0, 1)),
                           P("out", OUT, (3 * N, h, w))], **pl))
    add(Row("tcsfm_smooth_loss", [N, P("disp", IN, (N, 1, h, w), gen=g_uniform(0.05, 0.95)), P("img", IN, (N, 3, h, w), gen=g_uniform(0, 1)),
                                  P("loss_out", HOST_OUT, (1,), np.float64)], **pl))
    add(Row("tcsfm_disp_to_depth_backward", [n, P("disp", IN, (n,), gen=g_uniform(0.05, 0.95)), P("g_scaled", IN, (n,), gen=g_normal()),
                                             P("g_depth", IN, (n,), gen=g_normal()), P("g_disp", OUT, (n,))],
            honoured=[("g_disp", "disp", SAME), ("g_disp", "g_scaled", SAME), ("g_disp", "g_depth", SAME)], **pl))
    add(Row("tcsfm_ssim_backward", [3 * N, P("x", IN, (3 * N, h, w), gen=g_uniform(0, 1)), P("y", IN, (3 * N, h, w), gen=g_uniform(0, 1)),
                                    P("g_out", IN, (3 * N, h, w), gen=g_normal()), P("g_x", OUT, (3 * N, h, w)), P("g_y", OUT, (3 * N, h, w))], **pl))
    add(Row("tcsfm_smooth_loss_device", [N, P("disp", IN, (N, 1, h, w), gen=g_uniform(0.05, 0.95)), P("img", IN, (N, 3, h, w), gen=g_uniform(0, 1)),
                                         P("loss_out", OUT, (1,)), P("stats_out", OUT, (N, 3), np.float64)], **pl))
    add(Row("tcsfm_smooth_loss_backward", [N, P("disp", IN, (N, 1, h, w), gen=g_uniform(0.05, 0.95)), P("img", IN, (N, 3, h, w), gen=g_uniform(0, 1)),
                                           P("stats", IN, (N, 3), np.float64, gen=g_const([0.5, 40.0, 35.0])), P("g_loss", IN, (1,), gen=g_const(1.0)),
                                           P("g_disp", OUT, (N, 1, h, w))], **pl))
    B, S = 2, 2
    m = (S * B, 1, h, w)
    wl_in = [P("fwd_diff", IN, m, gen=g_uniform(0, 1)), P("fwd_valid", IN, m, gen=g_mask), P("fwd_weight", IN, m, gen=g_uniform(0.2, 1)),
             P("fwd_auto_err", IN, m, gen=g_uniform(0, 1)), P("inv_diff", IN, m, gen=g_uniform(0, 1)), P("inv_valid", IN, m, gen=g_mask),
             P("inv_weight", IN, m, gen=g_uniform(0.2, 1)), P("inv_auto_mask", IN, m, gen=g_mask)]
    for argmin in (0, 1):        # the non-argmin form re-reads fwd_diff after it has stored g_fwd_diff
        add(Row("tcsfm_window_loss", [B, S, argmin, 1] + wl_in + [P("loss_out", OUT, (1,)), P("stats_out", OUT, (7,), np.float64)],
                opts=dict(w_dc=0.15), **pl))
        add(Row("tcsfm_window_loss_backward", [B, S, argmin, 1] + wl_in +
                [P("stats", IN, (7,), np.float64, gen=g_const([300.0, 900.0, 250.0, 800.0, 1500.0, 1400.0, float(S * B * h * w)])),
                 P("g_loss", IN, (1,), gen=g_const(1.0)), P("g_fwd_diff", OUT, m), P("g_fwd_weight", OUT, m), P("g_inv_diff", OUT, m),
                 P("g_inv_weight", OUT, m)], opts=dict(w_dc=0.15), **pl))

    # -- warp, photometric and their backward passes
    m1, m3 = (N, 1, H, W), (N, 3, H, W)
    add(Row("tcsfm_warp", [N] + _pair_inputs(N, tgt=False) + _pose_K(N) +
            [P("img_rec", OUT, m3), P("valid", OUT, m1), P("proj_depth", OUT, m1), P("comp_depth", OUT, m1)]))
    add(Row("tcsfm_warp_backward", [N] + _pair_inputs(N, tgt=False) + _pose_K(N) +
            [P("g_rec", IN, m3, gen=g_normal()), P("g_proj_depth", IN, m1, gen=g_normal()), P("g_comp_depth", IN, m1, gen=g_normal()),
             P("d_depth_t", OUT, m1), P("d_depth_s", OUT, m1), P("d_pose", OUT, (N, 6))]))
    add(Row("tcsfm_photometric_maps_backward", [N, P("tgt", IN, m3, gen=g_pair("tgt")), P("img_rec", IN, m3, gen=g_pair("src")),
                                                P("proj_depth", IN, m1, gen=g_pair("depth_t")), P("comp_depth", IN, m1, gen=g_pair("depth_s")),
                                                P("g_diff", IN, m1, gen=g_normal()), P("g_weight", IN, m1, gen=g_normal()),
                                                P("g_rec", OUT, m3), P("g_proj_depth", OUT, m1), P("g_comp_depth", OUT, m1)]))
    add(Row("tcsfm_photometric_backward", [N] + _pair_inputs(N) + _pose_K(N) +
            [P("g_diff", IN, m1, gen=g_normal()), P("g_weight", IN, m1, gen=g_normal()), P("g_img_rec", IN, m3, gen=g_normal()),
             P("d_depth_t", OUT, m1), P("d_depth_s", OUT, m1), P("d_pose", OUT, (N, 6))]))
    add(Row("tcsfm_warp_posenet_input", [N] + _pair_inputs(N) + _pose_K(N) + [P("posenet_in", OUT, (N, 6, H, W)), P("valid", OUT, m1)]))
    add(Row("tcsfm_photometric", [N] + _pair_inputs(N) + _pose_K(N) +
            [P(k, OUT, m1) for k in ("diff", "valid", "weight", "auto_err", "auto_mask")] + [P("img_rec", OUT, m3)]))
    p1 = [P("tgt", IN, (3, H, W), gen=lambda p: _pairs()["tgt"][0]), P("src", IN, (3, H, W), gen=lambda p: _pairs()["src"][0]),
          P("depth_t", IN, (1, H, W), gen=lambda p: _pairs()["depth_t"][0]), P("depth_s", IN, (1, H, W), gen=lambda p: _pairs()["depth_s"][0]),
          P("K", IN, (3, 3), gen=lambda p: _pairs()["K"][0])]
    add(Row("tcsfm_loss_surface", p1 + [3, P("poses", IN, (3, 6), gen=lambda p: _pairs()["pose_init"][0] + np.linspace(-0.01, 0.01, 3)[:, None].astype(np.float32)),
                                        P("cost_out", HOST_OUT, (3,), np.float64)]))

    # -- the engine: linearisations and refinements
    ls = lambda count: g_const(np.linspace(-0.03, 0.02, count))
    add(Row("tcsfm_linearize", [N] + _pair_inputs(N) + [P("pose", IN, (N, 6), gen=g_pair("pose_init")), P("log_scale", IN, (N,), gen=ls(N)),
                                                        P("K", IN, (N, 3, 3), gen=g_pair("K")), P("Hmat", HOST_OUT, (N, 7, 7), np.float64),
                                                        P("g", HOST_OUT, (N, 7), np.float64), P("stats", HOST_OUT, (N, 4), np.float64)],
            opts=dict(refine=1)))
    Bw, Sw = 1, 2
    Nw = 2 * Bw * Sw
    add(Row("tcsfm_linearize_window", [Bw, Sw] + _win_inputs(Bw, Sw, "pose") +
            [P("log_scale", IN, (Nw,), gen=ls(Nw)), P("Hmat", HOST_OUT, (Nw, 7, 7), np.float64), P("g", HOST_OUT, (Nw, 7), np.float64),
             P("stats", HOST_OUT, (Nw, 4), np.float64)], opts=dict(refine=1, argmin=1)))
    it = 2
    refine_tail = lambda Np: [P("log_scale_in", IN, (Np,), gen=ls(Np)), P("pose_out", OUT, (Np, 6)), P("log_scale_out", OUT, (Np,)),
                              P("stats_out", OUT, (Np, it + 1, NSTAT))]
    pair_core = _pair_inputs(N) + [P("K", IN, (N, 3, 3), gen=g_pair("K")), P("pose_in", IN, (N, 6), gen=g_pair("pose_init"))]
    add(Row("tcsfm_refine", [N] + pair_core + refine_tail(N), honoured=[("pose_out", "pose_in", SAME)], opts=dict(n_iters=it, refine=1)))
    add(Row("tcsfm_refine_window", [Bw, Sw] + _win_inputs(Bw, Sw, "pose_in") + refine_tail(Nw), honoured=[("pose_out", "pose_in", SAME)],
            opts=dict(n_iters=it, refine=1, argmin=1)))
    dense_h = [("pose_out", "pose_in", SAME), ("depth_out", "depth_t", ANY), ("depth_out", "depth_s", ANY)]
    dense_tail = lambda Np, stats=True: [P("pose_out", OUT, (Np, 6)), P("depth_out", OUT, (Np, 1, H, W))] + \
        ([P("stats_out", OUT, (Np, it + 1, NSTAT))] if stats else [])
    add(Row("tcsfm_refine_dense", [N] + pair_core + dense_tail(N), honoured=dense_h, opts=dict(n_iters=it)))
    Bd, Sd = 2, 2                   # B = 1 would write identical values over depth_t and hide the reference mode's race
    Nd = 2 * Bd * Sd
    add(Row("tcsfm_refine_dense_window", [Bd, Sd] + _win_inputs(Bd, Sd, "pose_in") + dense_tail(Nd), honoured=dense_h,
            opts=dict(n_iters=it, window_rule=1, w_dc=0.15, argmin=1)))
    lin_dense = lambda src: [Bw, Sw] + _win_inputs(Bw, Sw, "pose") + \
        [P("depth0", IN, (Bw, 1, H, W), gen=lambda p: (_window(Bw, Sw)["depth_t"] * 0.97).astype(np.float32)),
         P("scal_out", HOST_OUT, (8,), np.float64), P("g_pose_out", HOST_OUT, (Nw, 6), np.float64), P("g_rho_out", OUT, (Bw, H * W))] + \
        ([P("g_rho_src_out", OUT, (Sw, Bw, H * W))] if src else [])
    add(Row("tcsfm_linearize_dense_window", lin_dense(False), opts=dict(window_rule=1, w_dc=0.15, argmin=1)))
    add(Row("tcsfm_linearize_dense_window_sources", lin_dense(True), opts=dict(window_rule=1, w_dc=0.15, argmin=1)))
    add(Row("tcsfm_scale_recovery", [N, P("depth", IN, m1, gen=g_pair("depth_t")), P("K", IN, (N, 3, 3), gen=g_pair("K")), 1.65, 4,
                                     P("scale_out", OUT, (1,)), P("median_out", OUT, (1,)), P("height_out", OUT, (N, 1, H, W)),
                                     P("mask_out", OUT, (N, 1, H, W))]))

    # -- lanes and queued calls (device pointers; the queued rows are flushed by the runner)
    add(Row("tcsfm_refine_window_async", [Bw, Sw] + _win_inputs(Bw, Sw, "pose_in") + refine_tail(Nw), honoured=[("pose_out", "pose_in", SAME)],
            opts=dict(n_iters=it, refine=1, argmin=1), lane=1))
    add(Row("tcsfm_refine_dense_window_async", [Bd, Sd] + _win_inputs(Bd, Sd, "pose_in") + dense_tail(Nd), honoured=dense_h,
            opts=dict(n_iters=it, window_rule=1, w_dc=0.15, argmin=1), lane=1))
    add(Row("tcsfm_refine_window_queued", [Bw, Sw] + _win_inputs(Bw, Sw, "pose_in") + [P("pose_out", OUT, (Nw, 6))],
            honoured=[("pose_out", "pose_in", SAME)], opts=dict(n_iters=it, argmin=1)))
    add(Row("tcsfm_refine_window_scale_queued", [Bw, Sw] + _win_inputs(Bw, Sw, "pose_in") +
            [P("log_scale_in", IN, (Nw,), gen=ls(Nw)), P("pose_out", OUT, (Nw, 6)), P("log_scale_out", OUT, (Nw,))],
            honoured=[("pose_out", "pose_in", SAME)], opts=dict(n_iters=it, refine=1, argmin=1)))
    add(Row("tcsfm_refine_dense_window_queued", [Bd, Sd] + _win_inputs(Bd, Sd, "pose_in") + dense_tail(Nd, stats=False), honoured=dense_h,
            opts=dict(n_iters=it, window_rule=1, w_dc=0.15, argmin=1)))

    # -- the sequence calls: host pointers whatever opts.host_ptrs says, streamed
    T, Ss = 5, 2
    nw_, Ns = T - Ss, 2 * Ss
    seq_in = [P("frames", IN, (T, 3, H, W), gen=g_seq("frames", T)), P("depths", IN, (T, 1, H, W), gen=g_seq("depths", T)),
              P("K", IN, (3, 3), gen=g_seq("K", T))]
    pinit = P("pose_init", IN, (nw_, Ns, 6), gen=g_normal(0.003))
    add(Row("tcsfm_refine_sequence", [T, Ss] + seq_in + [pinit, P("pose_out", OUT, (nw_, Ns, 6)), P("log_scale_out", OUT, (nw_, Ns)), 0, 2, -1],
            honoured=[("pose_out", "pose_init", SAME)], opts=dict(n_iters=it, refine=1), runner="sequence", max_pairs=16))
    add(Row("tcsfm_refine_dense_sequence", [T, Ss] + seq_in + [pinit, P("pose_out", OUT, (nw_, Ns, 6)), P("depth_out", OUT, (nw_, Ns, H, W)), 0, 2, -1],
            honoured=[("pose_out", "pose_init", SAME)], opts=dict(n_iters=it), runner="sequence", max_pairs=16))
    add(Row("tcsfm_odometry_sequence", ["pn", 2, "opts", T, Ss] + seq_in +
            [P("pose_init_out", OUT, (nw_, Ns, 6)), P("pose_out", OUT, (nw_, Ns, 6)), P("log_scale_out", OUT, (nw_, Ns)), 0, 2, -1],
            opts=dict(n_iters=it, refine=1), runner="test_networks_refuse", max_pairs=16))

    # -- the networks and the optimiser: classified here, driven by test_networks_refuse / test_optimiser_refuses (each output against the
    #    largest input; pointer arrays contribute one range per element)
    net = dict(hw=NET_HW, runner="test_networks_refuse", takes_opts=False)
    add(Row("tcsfm_posenet_forward", [P("imgs", IN), P("pose_out", OUT)], **net))
    add(Row("tcsfm_solve_pose_iteratively", [P("tgt", IN), P("srcs", IN), P("depth_t", IN), P("depth_s", IN), P("K", IN), P("poses_out", OUT),
                                             P("stacked_out", OUT)], **net))
    add(Row("tcsfm_posenet_forward_train", [P("imgs", IN), P("pose_out", OUT), P("tape", OUT)], **net))
    add(Row("tcsfm_posenet_backward", [P("tape", IN), P("d_pose", IN), P("d_imgs", OUT)], **net))
    add(Row("tcsfm_posenet_param_backward", [P("imgs", IN), P("tape", IN), P("d_pose", IN), P("d_imgs", OUT), P("conv_w_g", OUT), P("conv_b_g", OUT),
                                             P("gn_w_g", OUT), P("gn_b_g", OUT), P("head_w_g", OUT), P("head_b_g", OUT)], **net))
    add(Row("tcsfm_depthnet_encode", [P("imgs", IN), P("skips_out", OUT)], **net))
    add(Row("tcsfm_depthnet_decode", [P("skips_in", IN), P("disp_out", OUT)], **net))
    add(Row("tcsfm_depthnet_forward", [P("imgs", IN), P("disp_out", OUT)], **net))
    add(Row("tcsfm_depthnet_encode_train", [P("imgs", IN), P("skips_out", OUT), P("tape", OUT)], **net))
    add(Row("tcsfm_depthnet_decode_train", [P("skips_in", IN), P("disp_out", OUT), P("tape", OUT)], **net))
    add(Row("tcsfm_depthnet_decode_backward", [P("tape", IN), P("d_disp", IN), P("d_skips", OUT), P("names", HOST_IN), P("grads", OUT)], **net))
    add(Row("tcsfm_depthnet_encode_backward", [P("tape", IN), P("d_skips", IN), P("names", HOST_IN), P("grads", OUT)], **net))
    opt = dict(hw=NET_HW, runner="test_optimiser_refuses", takes_opts=False)
    add(Row("tcsfm_optim_create", [P("params", OUT), P("numel", HOST_IN)], **opt))
    add(Row("tcsfm_optim_step", [P("grads", IN), P("lr", HOST_IN)], **opt))
    add(Row("tcsfm_optim_get_state", [P("exp_avg_out", OUT), P("exp_avg_sq_out", OUT)], **opt))
    return rows


ROWS = _rows()

# Entries with pointer parameters that carry no caller arrays an output could overlap: each with its reason.
EXEMPT = {
    "tcsfm_posenet_load": "inputs only (host tensors are copied into the instance)",
    "tcsfm_posenet_load_device": "inputs only (device tensors are copied into the instance)",
    "tcsfm_depthnet_load": "inputs only (host tensors are copied into the instance)",
    "tcsfm_depthnet_load_device": "inputs only (device tensors are copied into the instance)",
    "tcsfm_lane_probe": "two host scalars of a measurement",
    "tcsfm_debug_posenet_layer": "debug reader: copies of the instance's own activations",
    "tcsfm_debug_posenet_tape_layer": "debug reader: copies of one tape layer",
    "tcsfm_profile_end": "profiling: host sums",
    "tcsfm_profile_kernel_time": "profiling: host scalars",
    "tcsfm_profile_kernel_busy": "profiling: host scalars",
    "tcsfm_debug_stamps": "debug reader: eight host counters",
    "tcsfm_pose_to_matrix": "SE(3) host utility on small fixed arrays",
    "tcsfm_matrix_to_pose": "SE(3) host utility on small fixed arrays",
    "tcsfm_se3_exp": "SE(3) host utility on small fixed arrays",
    "tcsfm_se3_log": "SE(3) host utility on small fixed arrays",
    "tcsfm_se3_mul": "SE(3) host utility on small fixed arrays",
    "tcsfm_se3_inv": "SE(3) host utility on small fixed arrays",
}


def rows_for(entry):
    return [r for r in ROWS if r.entry == entry]


def row_id(r):
    i = rows_for(r.entry).index(r)
    return r.entry if len(rows_for(r.entry)) == 1 else f"{r.entry}#{i}"
