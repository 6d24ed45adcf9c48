"""Non-default values of the public tcsfm_opts fields, in every solver family.

The rest of the GPU suite compares the kernels with the float64 oracle almost only at the default options.  Every field below is copied
into each kernel family's parameters separately (the photometric weights into the pack, the linearisation, the dense, joint and
reference-loss kernels and the loss surface; the LM schedule into three solvers; prior_scale into the pose solver; the depth bounds into
the dense modes; the disparity conversion into k_pack and k_frame_pack), so each copy is checked on its own here:

  * linearisation level: cost, mask count, gradient and GN matrix at (w_l1, w_ssim) in {(0.5, 0.5), (1, 0), (0, 1)} and a non-default
    irls_eps, for the pair, window (both rules) and reference-loss dense linearisations, the photometric maps and the loss surface;
  * iterates with the engine's decisions replayed through the oracle (parity_util) at (0.4, 0.6): LM with a non-default schedule whose
    rejects are asserted and whose lambda column is checked row by row, prior_scale, windows, dense pairs, the library's joint mode, the
    reference-loss dense mode (full, quarter, free) and depth bounds that bind;
  * sigmoid-disparity inputs (depth_is_disp = 1) give the bits of the depths Engine.disp_to_depth makes from them, in every family;
  * queued calls, graph replay, lanes and the sequence loops carry the options: bit-identical to the direct calls.

Every case also runs once with the option at its default and requires different output bits, so an option read nowhere cannot pass
by being too small to see against the oracle's tolerance.  The bars are the suite's (parity_util): pose 1e-4, depth 1e-4 per pixel,
cost 2e-5, gradient / GN matrix 2e-4 of their largest entry."""
import numpy as np
import pytest
import torch

import parity_util as PU
from oracle.oracle import default_opts as oracle_opts

pytestmark = pytest.mark.gpu

WEIGHTS = [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)]
W_IT = dict(w_l1=0.4, w_ssim=0.6)                                              # the iterate-level weights
LM = dict(solver=1, lambda0=1e-2, lambda_up=4.0, lambda_down=0.5, lambda_min=1e-3)  # a non-default LM schedule
DISP_BOUNDS = (0.1, 80.0)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _eng(H, W, n, lanes=1):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(H, W, n, lanes=lanes)


def _opts(**kw):
    from tightly_coupled_sfm_amd.engine import default_opts
    return default_opts(**kw)


def _with(o, **kw):
    """a copy of engine options o with some fields replaced"""
    from tightly_coupled_sfm_amd.engine import _copy_opts
    c = _copy_opts(o)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _outs_differ(a, b):
    return any(x is not None and not torch.equal(x, y) for x, y in zip(a, b))


def _guard(call, o, **defaults):
    """option read nowhere: `call(opts)` -> tuple of output tensors must change when the named fields go back to their defaults"""
    a = call(o)
    b = call(_with(o, **defaults))
    torch.cuda.synchronize()
    assert _outs_differ(a, b), ("output bits do not depend on", defaults)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.abs(b).max(), 1e-300))


def _assert_lin(tag, cost, n_mask, g, Hm, ref):
    assert abs(cost - ref["cost"]) < PU.COST_TOL * ref["cost"], (tag, cost, ref["cost"])
    assert abs(n_mask - ref["n_mask"]) <= 0.003 * ref["n_mask"] + 1, (tag, n_mask, ref["n_mask"])
    assert _rel(g, ref["g"]) < 2e-4, (tag, "g", _rel(g, ref["g"]))
    assert _rel(Hm, ref["H"]) < 2e-4, (tag, "H", _rel(Hm, ref["H"]))


def _lm_schedule(costs, dec, o, rows):
    """the damping of every stats row implied by the costs: rows 0 and 1 lambda0 (the first linearisation is accepted unconditionally);
    after an accepted row max(lambda * down, min), after a rejected one lambda * up.  A decision is taken from the costs unless the two
    costs tie (then the engine's, see check_lm_decisions)"""
    lam, cur, out = float(o.lambda0), costs[0], [float(o.lambda0)] * 2
    for it in range(1, rows - 1):
        c = costs[it]
        acc = bool(dec[it]) if abs(c - cur) <= PU.COST_TIE * cur else c < cur
        if acc:
            lam = max(lam * float(o.lambda_down), float(o.lambda_min)); cur = c
        else:
            lam *= float(o.lambda_up)
        out.append(lam)
    return np.array(out)


def _check_lambda_column(st, rst, dec, o, tag):
    rows = int(o.n_iters) + 1
    for n in range(st.shape[0]):
        want = _lm_schedule(rst[n][:rows, 0], dec[:, n], o, rows)
        assert np.allclose(st[n, :rows, 3], want, rtol=1e-6, atol=0), (tag, n, st[n, :rows, 3], want)
        assert np.allclose(rst[n][:rows, 3], want, rtol=1e-12), (tag, n, rst[n][:rows, 3], want)


def _window(B, S, H, W, seed, mind=0.06, maxd=2.67):
    import standins
    from oracle.oracle import Oracle
    w = standins.make_window(B, S, H, W, seed0=seed)
    o64 = Oracle("f64")
    w["depth_t"] = o64.disp_to_depth(w["disp_t"], mind, maxd)[1].astype(np.float32)
    w["depth_s"] = o64.disp_to_depth(w["disp_s"], mind, maxd)[1].astype(np.float32)
    return w


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. linearisation level: photometric weights and irls_eps
@pytest.mark.parametrize("H,W", [(28, 48), (96, 320)])
def test_linearisations_at_photometric_weights(H, W, oracle64):
    from tightly_coupled_sfm_amd import synth, _lib
    import test_gpu_dense_shapes as DS
    N = 2
    b = synth.make_batch(N, H, W, seed0=5, both_directions=True)
    d = [_t(b[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K")]
    p0 = _t(b["pose_init"])
    ls = np.array([0.03, -0.04], np.float32)
    w = _window(1, 2, H, W, seed=95)
    wt = [_t(w[k]) for k in ("target", "sources", "depth_t", "depth_s", "K", "first")]
    rw = DS._window(1, 2, H, W, seed=61)
    rt = {k: _t(v) for k, v in rw.items()}
    rdt, rds = rt["depth_t"][:, None].contiguous(), rt["depth_s"][:, :, None].contiguous()
    e = _eng(H, W, 8)
    eps = 3e-3
    for wl, ws in WEIGHTS:
        tag = (wl, ws)
        kw = dict(w_l1=wl, w_ssim=ws, irls_eps=eps)
        # pairs, 6 and 7 parameters
        for refine in (0, 1):
            o = _opts(refine=refine, w_dc=0.15, **kw)
            lin = lambda oo: e.linearize(*d, p0, oo, log_scale=_t(ls) if refine else None)
            out = lin(o)
            for n in range(N):
                ref = oracle64.linearize(b["tgt"][n], b["src"][n], b["depth_t"][n, 0], b["depth_s"][n, 0], b["pose_init"][n], b["K"][n],
                                         oracle_opts(nparam=6 + refine, w_dc=0.15, **kw), log_scale=float(ls[n]) if refine else 0.0)
                _assert_lin((tag, "pair", refine, n), out["cost"][n], out["n_mask"][n], out["g"][n], out["H"][n], ref)
            ow, od = lin(_with(o, w_l1=0.15, w_ssim=0.85)), lin(_with(o, irls_eps=1e-3))
            assert not np.array_equal(out["g"], ow["g"]) and not np.array_equal(out["H"], od["H"]), tag      # both options are read
        # windows, both rules, min over the sources
        for rule in (_lib.WINDOW_PAIR, _lib.WINDOW_REFERENCE):
            o = _opts(window_rule=rule, **kw)
            out = e.linearize_window(*wt, o, argmin=True)
            ref = oracle64.linearize_window(w["target"], w["sources"], w["depth_t"][:, 0], w["depth_s"][:, :, 0], w["K"], w["first"],
                                            oracle_opts(**kw), argmin=True, rule=rule)
            for m in range(len(ref["cost"])):
                _assert_lin((tag, "window", rule, m), out["cost"][m], out["n_mask"][m], out["g"][m], out["H"][m],
                            {k: ref[k][m] for k in ("cost", "n_mask", "g", "H")})
            assert not np.array_equal(out["g"], e.linearize_window(*wt, _with(o, w_l1=0.15, w_ssim=0.85), argmin=True)["g"]), tag
        # the reference-loss dense linearisation: gradient w.r.t. every pose, the target map and (free sources) the source maps
        o = _opts(n_iters=1, w_dc=0.15, prior_init=0.1, min_depth=0.06, max_depth=2.67, **kw)
        L = e.linearize_dense_window(rt["tgt"], rt["srcs"], rdt, rds, rt["K"], rt["pose"], o, argmin=True, sources=True)
        Lo = oracle64.linearize_dense_ref(_f32(rw["tgt"]), _f32(rw["srcs"]), _f32(rw["depth_t"]), _f32(rw["depth_s"]), _f32(rw["K"]), _f32(rw["pose"]),
                                          oracle_opts(n_iters=1, w_dc=0.15, **kw), argmin=True, w_init=0.1, min_depth=0.06, max_depth=2.67)
        assert abs(L["loss"] - Lo["loss"]) < PU.COST_TOL * Lo["loss"] and L["K_f"] == Lo["K_f"] and L["K_i"] == Lo["K_i"], (tag, L["loss"], Lo["loss"])
        assert _rel(L["g_pose"], Lo["g_xi"]) < 2e-4, tag
        assert _rel(L["g_rho"][:, 0].cpu().numpy(), Lo["g_rho"]) < 2e-4, tag
        assert _rel(L["g_rho_src"][:, :, 0].cpu().numpy(), Lo["g_rho_s"]) < 2e-4, tag
        L0 = e.linearize_dense_window(rt["tgt"], rt["srcs"], rdt, rds, rt["K"], rt["pose"], _with(o, w_l1=0.15, w_ssim=0.85), argmin=True)
        assert L0["loss"] != L["loss"] and not torch.equal(L0["g_rho"], L["g_rho"]), tag
        # photometric maps and the loss surface
        r = e.compute_photometric_error(*d[:4], p0, d[4], _opts(**kw))
        for n in range(N):
            ph = oracle64.photometric(b["tgt"][n], b["src"][n], b["depth_t"][n, 0], b["depth_s"][n, 0], b["pose_init"][n], b["K"][n], w_l1=wl, w_ssim=ws)
            valid = r["warp_valid"][n, 0].cpu().numpy()
            vbad = valid != ph["valid"]
            near = np.zeros_like(vbad)                 # the diff of a pixel reads the 3 x 3 neighbourhood of the reconstruction
            for dv in (-1, 0, 1):
                for du in (-1, 0, 1):
                    near |= np.roll(np.roll(vbad, dv, 0), du, 1)
            ok = ~near
            assert np.abs(r["diff_img"][n, 0].cpu().numpy() - ph["diff"])[ok].max() < 2e-5, tag
            assert np.abs(r["auto_mask_error"][n, 0].cpu().numpy() - ph["auto_err"]).max() < 2e-5, tag
            assert np.abs(r["weight_mask"][n, 0].cpu().numpy() - ph["weight"])[~vbad].max() < 2e-5, tag
        r0 = e.compute_photometric_error(*d[:4], p0, d[4], _opts())
        assert not torch.equal(r0["diff_img"], r["diff_img"]) and not torch.equal(r0["auto_mask_error"], r["auto_mask_error"]), tag
        poses = np.stack([b["pose_init"][0] * (1 + 0.2 * k) for k in range(-2, 3)]).astype(np.float32)
        one = [x[0:1].contiguous() for x in d]
        surf = e.loss_surface(*one[:4], one[4], _t(poses), _opts(w_dc=0.15, **kw))
        for k, p in enumerate(poses):
            c = oracle64.cost(b["tgt"][0], b["src"][0], b["depth_t"][0, 0], b["depth_s"][0, 0], p, b["K"][0], oracle_opts(w_dc=0.15, **kw))
            assert abs(surf[k] - c) < PU.COST_TOL * c, (tag, k, surf[k], c)
        assert not np.array_equal(surf, e.loss_surface(*one[:4], one[4], _t(poses), _opts(w_dc=0.15, irls_eps=eps))), tag
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. iterates with the engine's decisions replayed
def test_lm_schedule_on_pose_pairs(oracle64):
    """LM with lambda0 = 1e-2, up = 4, down = 0.5, min = 1e-3 on pairs that reject (seeds found with the oracle): every row of the
    TCSFM_STAT_LAMBDA column is the schedule the replayed oracle's costs imply"""
    from tightly_coupled_sfm_amd import synth
    H, W, seeds = 48, 160, (21, 26, 30, 31)
    ps = [synth.make_pair(H, W, seed=s) for s in seeds]
    b = {k: np.stack([p[k] for p in ps]) for k in ("tgt", "src", "K")}
    b["depth_t"] = np.stack([p["depth_t"] for p in ps])[:, None]; b["depth_s"] = np.stack([p["depth_s"] for p in ps])[:, None]
    b["pose_init"] = np.stack([synth.perturb_pose(p["pose_gt"], s, sigma_t=0.004, sigma_r=0.0012) for p, s in zip(ps, seeds)]).astype(np.float32)
    kw = dict(n_iters=8, **W_IT, **LM)
    o = _opts(**kw)
    e = _eng(H, W, len(seeds))
    r = PU.replay_pairs(e, oracle64, b, o, oracle_opts(**kw), _t)
    dec = r["decide"]
    assert int((dec[1:] == 0).sum()) >= 3, dec                                  # the schedule is exercised by rejects
    _check_lambda_column(r["stats"], np.stack(r["ref_stats"]), dec, o, "pairs")
    args = [_t(b[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K", "pose_init")]
    call = lambda oo: e.refine(*args, oo, stats=True)[::2]
    for f, v in dict(lambda0=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-5, w_l1=0.15).items():
        _guard(call, o, **{f: v})
    e.close()


@pytest.mark.parametrize("solver", [0, 1], ids=["gn", "lm"])
def test_pose_scale_prior(solver, oracle64):
    """REFINE_POSE_SCALE at prior_scale 0.1 and 10: poses, log scales and costs (which carry the prior) against the oracle"""
    from tightly_coupled_sfm_amd import synth
    H, W, N = 96, 320, 2
    b = synth.make_batch(N, H, W, seed0=12, both_directions=True)
    ls0 = np.array([0.04, -0.03], np.float32)
    e = _eng(H, W, N)
    args = [_t(b[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K", "pose_init")]
    moved = []
    for ps in (0.1, 10.0):
        kw = dict(n_iters=4, prior_scale=ps, **W_IT, **(LM if solver else dict(solver=0)))
        o = _opts(refine=1, **kw)
        r = PU.replay_pairs(e, oracle64, b, o, oracle_opts(nparam=7, **kw), _t, log_scale=ls0)
        moved.append(np.abs(r["log_scale"] - ls0).max())
        _guard(lambda oo: e.refine(*args, oo, log_scale=_t(ls0), stats=True), o, prior_scale=1.0)
    assert moved[0] > moved[1] > 0, moved                  # the stronger prior holds the scale closer to its start
    e.close()


def test_pose_pairs_full_size(oracle64):
    """192 x 640 (configs 2 / 5): weights and irls_eps through four Gauss-Newton iterations"""
    from tightly_coupled_sfm_amd import synth
    H, W, N = 192, 640, 2
    b = synth.make_batch(N, H, W, seed0=0, both_directions=True)
    kw = dict(n_iters=4, irls_eps=3e-3, **W_IT)
    e = _eng(H, W, N)
    PU.replay_pairs(e, oracle64, b, _opts(**kw), oracle_opts(**kw), _t)
    args = [_t(b[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K", "pose_init")]
    _guard(lambda oo: e.refine(*args, oo)[:1], _opts(**kw), w_l1=0.15, w_ssim=0.85)
    e.close()


@pytest.mark.parametrize("rule", [0, 1], ids=["pair-rule", "reference-rule+pose-consist"])
def test_windows_at_options(rule, oracle64):
    """window argmin with S = 2 (LM schedule) and the REFERENCE rule with w_pose_consist (GN)"""
    from tightly_coupled_sfm_amd import _lib
    B, S, H, W = 1, 2, 96, 320
    w = _window(B, S, H, W, seed=90)
    kw = dict(n_iters=4, **W_IT, **(LM if rule == 0 else dict(w_pose_consist=0.1)))
    o = _opts(window_rule=rule, **kw)
    e = _eng(H, W, 2 * S * B)
    r = PU.replay_window(e, oracle64, w, o, oracle_opts(**kw), _t, argmin=True, rule=rule)
    args = [_t(w[k]) for k in ("target", "sources", "depth_t", "depth_s", "K", "first")]
    call = lambda oo: e.refine_window(*args, oo, stats=True, argmin=True)[::2]
    if rule == 0:
        _check_lambda_column(r["stats"], r["ref_stats"], r["decide"], o, "window")
        _guard(call, o, lambda_up=10.0, lambda_down=0.1, lambda0=1e-4)
    else:
        _guard(call, o, w_pose_consist=0.0)
    _guard(call, o, w_l1=0.15, w_ssim=0.85)
    e.close()


@pytest.mark.parametrize("solver", [0, 1], ids=["gn", "lm"])
def test_dense_pairs_at_options(solver, oracle64):
    """dense pairs with lambda_depth = 0.3, prior_depth = 3 and the weights (LM: the non-default schedule)"""
    from tightly_coupled_sfm_amd import synth
    H, W, N = 48, 160, 2
    b = synth.make_batch(N, H, W, seed0=31, both_directions=True)
    d0 = (b["depth_t"] * (1 + 0.03 * np.sin(np.arange(W) / 9.0))[None, None, None, :]).astype(np.float32)
    kw = dict(n_iters=5, **W_IT, **(LM if solver else {}))
    o = _opts(lambda_depth=0.3, prior_depth=3.0, w_dc=0.0, **kw)
    e = _eng(H, W, N)
    r = PU.replay_dense_pairs(e, oracle64, b, d0, o, oracle_opts(**kw), _t)
    if solver:
        _check_lambda_column(r["stats"], np.stack(r["ref_stats"]), r["decide"], o, "dense pairs")
    args = [_t(b["tgt"]), _t(b["src"]), _t(d0), _t(b["depth_s"]), _t(b["K"]), _t(b["pose_init"])]
    call = lambda oo: e.refine_dense(*args, oo)[:2]
    _guard(call, o, lambda_depth=1.0)
    _guard(call, o, prior_depth=10.0)
    _guard(call, o, w_l1=0.15, w_ssim=0.85)
    e.close()


def test_library_joint_mode_lm_schedule(oracle64):
    """the library's joint mode (dense_joint = 1) at S = 2 under LM with the non-default schedule; the seed rejects twice at the end
    (found with orc_refine_dense_joint), so lambda_up is applied by the joint solver"""
    B, S, H, W = 1, 2, 48, 160
    mind, maxd = DISP_BOUNDS
    w = _window(B, S, H, W, seed=104, mind=mind, maxd=maxd)
    w["depth_t"] = (w["depth_t"] * (1 + 0.05 * np.sin(np.arange(W) / 7.0))[None, None, None, :]).astype(np.float32)
    gt = w["gt"].reshape(S * B, 6).astype(np.float64)
    f = (gt + 3.0 * (w["first"][:S * B].astype(np.float64) - gt)).astype(np.float32)
    w["first"] = np.concatenate([f, w["first"][S * B:]])
    kw = dict(n_iters=6, **W_IT, **LM)
    o = _opts(w_dc=0.0, lambda_depth=0.5, prior_depth=3.0, min_depth=mind, max_depth=maxd, **kw)
    e = _eng(H, W, 2 * S * B)
    r = PU.replay_window(e, oracle64, w, o, oracle_opts(**kw), _t, argmin=True, dense=True, joint=True)
    dec = r["decide"][:, :S * B]
    assert int((dec[1:] == 0).sum()) >= 2, dec
    _check_lambda_column(r["stats"][:S * B], r["ref_stats"][:S * B], dec, o, "joint")
    args = [_t(w[k]) for k in ("target", "sources", "depth_t", "depth_s", "K", "first")]
    call = lambda oo: e.refine_dense_window(*args, oo, stats=True, argmin=True)
    _guard(call, o, lambda_up=10.0)
    _guard(call, o, w_l1=0.15, w_ssim=0.85)
    e.close()


def _ref_dense_case(oracle64, H, W, S, quarter, free, mind, maxd, seed, n_it=3, bias=1.02):
    """the reference-loss dense mode at the iterate weights, lambda_depth = 0.5, prior_init = 0.3: replayed through the oracle.
    -> (engine poses, depth slots, oracle target maps, oracle source maps or None, options, call)"""
    from tightly_coupled_sfm_amd import _lib
    import test_gpu_dense_shapes as DS
    B = 1
    N = 2 * S * B
    w = DS._window(B, S, H, W, seed=seed, bias=bias)
    e = _eng(H, W, N)
    o = _opts(n_iters=n_it, w_dc=0.15, prior_init=0.3, min_depth=mind, max_depth=maxd, window_rule=_lib.WINDOW_REFERENCE, lambda_depth=0.5,
              depth_param=_lib.DEPTH_QUARTER if quarter else _lib.DEPTH_FULL, free_source_depths=1 if free else 0, **W_IT)
    t = {k: _t(v) for k, v in w.items()}
    dt4, ds5 = t["depth_t"][:, None].contiguous(), t["depth_s"][:, :, None].contiguous()
    call = lambda oo: e.refine_dense_window(t["tgt"], t["srcs"], dt4, ds5, t["K"], t["pose"], oo, stats=True, argmin=True)
    (pose, depth, _), bits, _ = PU.traced_and_production(e, n_it, N, lambda: call(o))
    pose = pose.cpu().numpy().astype(np.float64); depth = depth.cpu().numpy().astype(np.float64)[:, 0]
    fn = {(False, False): oracle64.refine_dense_ref, (True, False): oracle64.refine_dense_ref_q,
          (False, True): oracle64.refine_dense_ref_free, (True, True): oracle64.refine_dense_ref_q_free}[(quarter, free)]
    oracle64.flip_stats_reset()
    res = fn(_f32(w["tgt"]), _f32(w["srcs"]), _f32(w["depth_t"]), _f32(w["depth_s"]), _f32(w["K"]), _f32(w["pose"]),
             oracle_opts(n_iters=n_it, w_dc=0.15, **W_IT), argmin=True, w_init=0.3, lambda_depth=0.5, min_depth=mind, max_depth=maxd,
             bits=bits.reshape(n_it, N, H * W))
    nf, hard = oracle64.flip_stats(n_it)
    assert hard.sum() == 0 and np.all(nf <= 2 + 5e-4 * N * H * W), (nf, hard)
    for m in range(N):
        PU.assert_pose(pose[m], res[0][m], ("pair", m))
    for s in range(S):
        assert np.abs(depth[s] / res[1][0] - 1).max() < PU.DEPTH_TOL, s
    if free:
        assert np.abs(depth[S:].reshape(S, H, W) / res[2][:, 0] - 1).max() < PU.DEPTH_TOL
    return pose, depth, res[1][0], (res[2][:, 0] if free else None), o, call


@pytest.mark.parametrize("quarter,free", [(False, False), (True, False), (False, True)], ids=["full", "quarter", "free"])
def test_reference_loss_dense_mode_at_options(quarter, free, oracle64):
    H, W, S = 28, 48, 2
    *_, o, call = _ref_dense_case(oracle64, H, W, S, quarter, free, 0.06, 2.67, seed=71)
    _guard(call, o, w_l1=0.15, w_ssim=0.85)
    _guard(call, o, lambda_depth=1.0)


def test_dense_depth_bounds_bind(oracle64):
    """min_depth / max_depth of the dense modes chosen inside the range of the depths: more than 1 % of the pixels end ON a bound, in the
    oracle and in the engine alike (dense pairs and the reference-loss mode)"""
    from tightly_coupled_sfm_amd import synth
    H, W, N = 48, 160, 2
    b = synth.make_batch(N, H, W, seed0=3, both_directions=True)
    d0 = (b["depth_t"] * (1 + 0.03 * np.sin(np.arange(W) / 9.0))[None, None, None, :]).astype(np.float32)
    mind, maxd = float(np.quantile(d0, 0.3)), float(np.quantile(d0, 0.7))      # (pixels outside the frame keep their depth: wide margins)
    kw = dict(n_iters=4, **W_IT)
    o = _opts(lambda_depth=0.3, prior_depth=3.0, w_dc=0.0, min_depth=mind, max_depth=maxd, **kw)
    e = _eng(H, W, N)
    r = PU.replay_dense_pairs(e, oracle64, b, d0, o, oracle_opts(**kw), _t)
    for n in range(N):
        rd, dg = r["ref_depth"][n], r["depth"][n]
        for bound in (mind, maxd):
            on = np.abs(rd / bound - 1) < 1e-6
            assert on.mean() > 0.01, (n, bound, on.mean())
            assert np.abs(dg[on] / bound - 1).max() < 1e-6
    args = [_t(b["tgt"]), _t(b["src"]), _t(d0), _t(b["depth_s"]), _t(b["K"]), _t(b["pose_init"])]
    _guard(lambda oo: e.refine_dense(*args, oo)[:2], o, min_depth=0.06, max_depth=2.67)
    e.close()
    # the reference-loss mode: its target inverse-depth map clamped at the bounds
    import test_gpu_dense_shapes as DS
    w = DS._window(1, 2, 28, 48, seed=71)
    lo, hi = float(np.quantile(w["depth_t"], 0.3)), float(np.quantile(w["depth_t"], 0.7))
    _, depth, do, _, o, call = _ref_dense_case(oracle64, 28, 48, 2, False, False, lo, hi, seed=71)
    for bound in (lo, hi):
        on = np.abs(do / bound - 1) < 1e-6
        assert on.mean() > 0.01, (bound, on.mean())
        assert np.abs(depth[0][on] / bound - 1).max() < 1e-6
    _guard(call, o, min_depth=0.06, max_depth=2.67)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. sigmoid-disparity inputs: the bits of the converted depths, in every family
def _disp_data(H, W, T):
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(T, H, W, seed=21)
    mind, maxd = DISP_BOUNDS
    seq["disps"] = synth.depth_to_sigmoid_disp(seq["depths"].astype(np.float64), mind, maxd).astype(np.float32)
    return seq


def test_disparity_inputs_equal_converted_depths_everywhere():
    from tightly_coupled_sfm_amd import _lib
    H, W, T = 48, 96, 12
    mind, maxd = DISP_BOUNDS
    seq = _disp_data(H, W, T)
    e = _eng(H, W, 8, lanes=2)
    disp = _t(seq["disps"])
    _, depth = e.disp_to_depth(disp, mind, maxd)
    torch.cuda.synchronize()
    fr, K1 = _t(seq["frames"]), _t(seq["K"][None])
    base = dict(min_depth=mind, max_depth=maxd, n_iters=3, **W_IT)

    def both(tag, run, o):
        """run(opts, maps) -> outputs; maps [T,1,H,W] are disparities (depth_is_disp = 1) or the converted depths (0)"""
        a = run(_with(o, depth_is_disp=1), disp)
        b = run(_with(o, depth_is_disp=0), depth)
        c = run(_with(o, depth_is_disp=0), disp)          # the guard: disparities read as depths are another problem
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(a, b)):
            if x is not None:
                assert torch.equal(x, y), (tag, i, int((x != y).sum()), float((x.double() - y.double()).abs().max()))
        assert _outs_differ(a, c), tag

    # pairs: frame k -> k + 1
    N = 4
    p0 = _t(seq["init"][:N, 0])
    pair = lambda m: (fr[:N], fr[1:N + 1], m[:N], m[1:N + 1], K1.expand(N, 3, 3).contiguous(), p0)
    both("refine", lambda o, m: e.refine(*pair(m), o, stats=True), _opts(**base))
    both("refine scale", lambda o, m: e.refine(*pair(m), o, log_scale=_t(np.full(N, 0.02)), stats=True), _opts(refine=1, **base))
    both("refine_dense", lambda o, m: e.refine_dense(*pair(m), o, stats=True), _opts(**base))
    # windows: target frame 1, sources frames 0 and 2
    init = np.stack([seq["init"][0, 1], seq["init"][1, 0], seq["init"][0, 0], seq["init"][1, 1]]).astype(np.float32)
    p4 = _t(init)
    win = lambda m: (fr[1:2], torch.stack([fr[0:1], fr[2:3]]), m[1:2], torch.stack([m[0:1], m[2:3]]), K1, p4)
    both("refine_window", lambda o, m: e.refine_window(*win(m), o, stats=True, argmin=True), _opts(**base))
    both("refine_window scale", lambda o, m: e.refine_window(*win(m), o, stats=True, argmin=True), _opts(refine=1, **base))
    both("dense joint", lambda o, m: e.refine_dense_window(*win(m), o, stats=True, argmin=True), _opts(**base))
    both("dense per-pair", lambda o, m: e.refine_dense_window(*win(m), o, stats=True, argmin=True), _opts(dense_joint=0, **base))
    for tag, kw in (("ref full", {}), ("ref quarter", dict(depth_param=_lib.DEPTH_QUARTER)), ("ref free", dict(free_source_depths=1))):
        both(tag, lambda o, m: e.refine_dense_window(*win(m), o, stats=True, argmin=True), _opts(window_rule=_lib.WINDOW_REFERENCE, **kw, **base))
    # merged queued calls: three windows (frame k -> k + 1) per launch sequence
    e.set_coalesce(3)
    inits = [_t(seq["init"][k]) for k in range(3)]          # (a queued call keeps its pointers until it runs)
    q = lambda k, m: (fr[k:k + 1], fr[k + 1:k + 2][None], m[k:k + 1], m[k + 1:k + 2][None], K1, inits[k])

    def queued(o, m):
        po = [torch.zeros(2, 6, device="cuda") for _ in range(3)]
        for k in range(3):
            e.refine_window_queued(*q(k, m), po[k], o)
        e.synchronize()
        return po

    def queued_dense(o, m):
        po = [torch.zeros(2, 6, device="cuda") for _ in range(3)]; do = [torch.zeros(2, 1, H, W, device="cuda") for _ in range(3)]
        for k in range(3):
            e.refine_dense_window_queued(*q(k, m), po[k], do[k], o)
        e.synchronize()
        return po + do

    c0 = e.coalesce_counts()
    both("queued", queued, _opts(**base))
    both("queued dense", queued_dense, _opts(**base))
    c1 = e.coalesce_counts()
    assert c1[0] - c0[0] == 6 and c1[1] - c0[1] == 18, (c0, c1)          # three calls per launch sequence: they were merged
    e.set_coalesce(0)
    e.close()
    # sequences: the pose loop takes the frame-pack cache (k_frame_pack converts), the dense loop the raw frames (k_pack converts);
    # a ring of S + 3 slots wraps, one frame copy at a time, and several windows per call
    e = _eng(H, W, 8, lanes=2)
    frames_c = torch.as_tensor(seq["frames"]).pin_memory()
    init_seq = seq["init"][:T - 1]
    seqrun = lambda o, m: [e.refine_sequence(frames_c, m.cpu().pin_memory(), seq["K"], init_seq, o, sources=1, ring=4, windows_per_call=2)]
    both("refine_sequence", seqrun, _opts(**base))
    seqrun8 = lambda o, m: [e.refine_sequence(frames_c, m.cpu().pin_memory(), seq["K"], init_seq, o, sources=1, ring=0, windows_per_call=4)]
    both("refine_sequence wpc 4", seqrun8, _opts(**base))
    dseq = lambda o, m: list(e.refine_dense_sequence(frames_c, m.cpu().pin_memory(), seq["K"], init_seq, o, sources=1, ring=4, windows_per_call=2))
    both("refine_dense_sequence", dseq, _opts(**base))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the options through the indirect paths
def test_options_through_queued_calls(oracle64):
    """queued pose, pose-scale, per-pair dense and reference-loss dense calls at non-default options: the bits of the direct calls;
    two calls that differ in one option are not merged"""
    from tightly_coupled_sfm_amd import _lib
    H, W = 48, 96
    seq = _disp_data(H, W, 8)
    fr, dp, K1 = _t(seq["frames"]), _t(seq["depths"]), _t(seq["K"][None])
    inits = [_t(seq["init"][k]) for k in range(7)]          # (a queued call keeps its pointers until it runs)
    call = lambda k: (fr[k:k + 1], fr[k + 1:k + 2][None], dp[k:k + 1], dp[k + 1:k + 2][None], K1, inits[k])
    ref = _eng(H, W, 2)
    e = _eng(H, W, 8)
    e.set_coalesce(3)
    o_pose = _opts(n_iters=4, **W_IT, **LM)
    o_scale = _opts(n_iters=4, refine=1, prior_scale=10.0, **W_IT)
    o_dense = _opts(n_iters=3, lambda_depth=0.3, prior_depth=3.0, min_depth=0.1, max_depth=80.0, **W_IT)
    o_ref = _opts(n_iters=3, window_rule=_lib.WINDOW_REFERENCE, lambda_depth=0.5, prior_init=0.3, min_depth=0.1, max_depth=80.0, **W_IT)
    ls = _t(np.array([0.02, -0.02]))
    for tag, o in (("pose", o_pose), ("scale", o_scale), ("dense", o_dense), ("ref", o_ref)):
        ks = range(3)
        if tag in ("pose", "scale"):
            want = [ref.refine_window(*call(k), o, log_scale=ls if tag == "scale" else None) for k in ks]
            want = [(p.clone(), None if l is None else l.clone()) for p, l, _ in want]
            po = [torch.zeros(2, 6, device="cuda") for _ in ks]; lo = [torch.zeros(2, device="cuda") for _ in ks]
            for k in ks:
                if tag == "scale":
                    e.refine_window_scale_queued(*call(k), ls, po[k], lo[k], o)
                else:
                    e.refine_window_queued(*call(k), po[k], o)
            e.synchronize()
            for k in ks:
                assert torch.equal(po[k], want[k][0]), (tag, k)
                assert tag != "scale" or torch.equal(lo[k], want[k][1]), (tag, k)
        else:
            want = [tuple(x.clone() for x in ref.refine_dense_window(*call(k), o)[:2]) for k in ks]
            po = [torch.zeros(2, 6, device="cuda") for _ in ks]; do = [torch.zeros(2, 1, H, W, device="cuda") for _ in ks]
            for k in ks:
                e.refine_dense_window_queued(*call(k), po[k], do[k], o)
            e.synchronize()
            for k in ks:
                assert torch.equal(po[k], want[k][0]) and torch.equal(do[k], want[k][1]), (tag, k)
    # two calls differing in w_l1 only: two launch sequences, each the bits of its own direct call
    o2 = _with(o_pose, w_l1=0.3)
    wa, wb = ref.refine_window(*call(0), o_pose)[0].clone(), ref.refine_window(*call(1), o2)[0].clone()
    assert not torch.equal(ref.refine_window(*call(1), o_pose)[0], wb)
    pa, pb = torch.zeros(2, 6, device="cuda"), torch.zeros(2, 6, device="cuda")
    c0 = e.coalesce_counts()
    e.refine_window_queued(*call(0), pa, o_pose)
    e.refine_window_queued(*call(1), pb, o2)
    e.synchronize()
    c1 = e.coalesce_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2), (c0, c1)
    assert torch.equal(pa, wa) and torch.equal(pb, wb)
    e.set_coalesce(0)
    e.close(); ref.close()


def test_options_through_graph_replay_lanes_and_sequences():
    """graph replay, asynchronous calls on lanes and the sequence loops at non-default options: the bits of the direct calls"""
    H, W, T = 48, 96, 9
    seq = _disp_data(H, W, T)
    fr, dp, K1 = _t(seq["frames"]), _t(seq["depths"]), _t(seq["K"][None])
    o = _opts(n_iters=4, **W_IT, **LM)
    od = _opts(n_iters=3, lambda_depth=0.3, prior_depth=3.0, min_depth=0.1, max_depth=80.0, **W_IT)
    ref = _eng(H, W, 2)
    # graph replay of the pair form
    args = (fr[0:2].contiguous(), fr[1:3].contiguous(), dp[0:2].contiguous(), dp[1:3].contiguous(), K1.expand(2, 3, 3).contiguous(),
            _t(seq["init"][0:2, 0]))
    want = ref.refine(*args, o)[0].clone()
    torch.cuda.synchronize()
    e = _eng(H, W, 2, lanes=2)
    e.use_own_stream()
    e.set_graph_replay(2)
    out = torch.zeros(2, 6, device="cuda")
    for _ in range(3):
        out.zero_(); torch.cuda.synchronize()
        e.refine_into(*args, out, o)
        e.synchronize()
        assert torch.equal(out, want)
    assert e.graph_replay_counts()[1] >= 1
    e.set_graph_replay(0)
    # lanes
    inits = [_t(seq["init"][k]) for k in range(T - 1)]      # (an asynchronous call reads its inputs after it returns)
    win = lambda k: (fr[k:k + 1], fr[k + 1:k + 2][None], dp[k:k + 1], dp[k + 1:k + 2][None], K1, inits[k])
    wp = [ref.refine_window(*win(k), o)[0].clone() for k in range(2)]
    wd = [tuple(x.clone() for x in ref.refine_dense_window(*win(k), od)[:2]) for k in range(2)]
    torch.cuda.synchronize()
    po = [torch.zeros(2, 6, device="cuda") for _ in range(4)]; do = [torch.zeros(2, 1, H, W, device="cuda") for _ in range(2)]
    for k in range(2):
        e.refine_window_async(k, *win(k), po[k], o)
    for k in range(2):
        e.lane_synchronize(k)
    for k in range(2):
        e.refine_dense_window_async(k, *win(k), po[2 + k], do[k], od)
    for k in range(2):
        e.lane_synchronize(k)
    for k in range(2):
        assert torch.equal(po[k], wp[k]) and torch.equal(po[2 + k], wd[k][0]) and torch.equal(do[k], wd[k][1]), k
    e.close()
    # the sequence loops against one window call per window
    e = _eng(H, W, 4, lanes=2)
    plain = torch.stack([ref.refine_window(*win(k), o)[0].cpu() for k in range(T - 1)])
    dplain = [ref.refine_dense_window(*win(k), od)[:2] for k in range(T - 1)]
    frames_c, depths_c = torch.as_tensor(seq["frames"]).pin_memory(), torch.as_tensor(seq["depths"]).pin_memory()
    got = e.refine_sequence(frames_c, depths_c, seq["K"], seq["init"], o, sources=1, ring=4, windows_per_call=2)
    assert torch.equal(got, plain)
    gp, gd = e.refine_dense_sequence(frames_c, depths_c, seq["K"], seq["init"], od, sources=1, windows_per_call=2)
    assert torch.equal(gp, torch.stack([p.cpu() for p, _ in dplain])) and torch.equal(gd, torch.stack([d.cpu() for _, d in dplain]))
    e.close(); ref.close()
