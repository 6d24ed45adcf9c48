"""Joint dense modes at RAGGED frame sizes: the dense mode on the reference's loss (window_rule = TCSFM_WINDOW_REFERENCE: k_dense_joint
on its own 32 x 8 tiles, k_dense_joint2, k_qres_*, k_solve_joint*) and the library's own joint mode (dense_joint = 1) on frames that fit
none of their tile grids -- a half-empty last tile column, one row into a second tile row, frames smaller than one tile or one quarter
cell group, the KITTI raw size with its split record sum.  Every case replays the engine's decisions through the float64 oracle at the
tolerances of test_gpu_dense_reference.py (poses 1e-4, every pixel of every unknown map 1e-4, no hard flip) and checks that the
production kernels (trace off) return the bits of the recording ones.

Until the joint kernels' workgroup-record scratch was sized from their own grid (it took the 16 x 16 tile count of the pose path), every
size whose 32 x 8 tile count exceeds that count -- ceil(W / 16) odd and ceil(H / 8) even: about a third of all frame sizes, 16 x 48,
28 x 48, 192 x 624, 480 x 720 among them -- was refused with an `internal:` error."""
import numpy as np
import pytest
import torch

import parity_util as PU
from oracle.oracle import default_opts as oracle_opts

pytestmark = pytest.mark.gpu

MIND, MAXD = 0.06, 2.67


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)         # the oracle starts from the SAME float32 inputs


def _window(B, S, H, W, seed, bias=1.02):
    """B targets x S sources (layout of test_gpu_dense_reference._window); source s moves by a different multiple of one base motion, so
    that no two sources of a target are the same image"""
    from tightly_coupled_sfm_amd import synth
    tg, dt, sr, ds, K, p0 = [], [], [[] for _ in range(S)], [[] for _ in range(S)], [], [[] for _ in range(S)]
    for bb in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0, -1.0, 1.6, -1.6)[s]
            p = synth.make_pair(H, W, seed=seed + 7 * bb, pose_gt=base, dtype=np.float64)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * bias); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    return dict(tgt=np.stack(tg), srcs=np.stack([np.stack(x) for x in sr]), depth_t=np.stack(dt), depth_s=np.stack([np.stack(x) for x in ds]),
                K=np.stack(K), pose=np.concatenate([fwd, -fwd]))


def _check_flips(orc, n_it, pixels, max_frac=5e-4):
    """no hard flip; near-tie flips per linearisation within 2 + max_frac * pixels (on a frame of a few dozen pixels the bar of
    check_dense_ref_flips, max_frac * pixels, rounds to zero)"""
    nf, hard = orc.flip_stats(n_it)
    assert hard.sum() == 0 and np.all(nf <= 2 + max_frac * pixels), (nf, hard)


# (H, W, B, S, extras): quarter = the quarter-resolution unknown, free = the source maps are unknowns too, tiny = too few pixels to
# demand that the cost falls or the map moves.  The sub-tile frames run without the min over the sources and without the auto-mask: at
# 4 x 4 / 5 x 9 the motion is sub-pixel, the identity reconstruction wins every pixel and the auto-mask would leave pairs without a
# single pixel -- a singular 6 x 6 pose block, whose "solution" is no parity check of anything.  On the sub-tile frames the linearisation at
# the start is compared with the oracle's as well (loss, every pose and pixel gradient).
# Two cases take ONE Gauss-Newton step.  375 x 1242 with free source maps (which have no prior): after the second step single source pixels
# of the float64 oracle itself move by 1.2e-3 under a 6e-8 relative perturbation of its float32 inputs (after one: the whole map by 2e-6).
# 4 x 4 with the quarter-resolution unknown: 16 pixels, one cell, poses coupled to it through every pixel -- the Schur-reduced pose systems
# lose digits to cancellation in fp32.  Measured after one step against the oracle: gradients 2e-7 (poses) / 1.3e-5 (map), the refined map
# 7e-8, the poses 2.5e-4 (4 x 8: 4.6e-5, 8 x 8: 9e-6, 12 x 12: 1e-5); its poses are held to pose_tol = 1e-3 (a wrong step is off by O(1)),
# everything else to the bar.  The further steps of both modes and the 1e-4 pose bar on a sub-tile frame (5 x 9) are covered by the others.
CASES = [
    (16, 48, 2, 2, dict()),                                          # LEAN S = 2 kernel, half-empty last tile column
    (28, 48, 2, 2, dict(quarter=True)),                              # the size of golden G13 winloss28x48
    (12, 36, 1, 3, dict(argmin=False)),                              # one full and one ragged tile row
    (9, 40, 1, 1, dict(w_smooth=2.0)),                               # one row into a second tile row; the rolled kernel
    (64, 208, 1, 2, dict(quarter=True, free=True)),                  # k_dense_joint2
    (192, 624, 1, 2, dict()),                                        # a KITTI-like width
    (480, 720, 1, 1, dict(n_it=2)),
    (4, 4, 1, 2, dict(n_it=1, quarter=True, tiny=True, argmin=False, automask=0, pose_tol=1e-3)),     # smaller than one tile: ONE quarter cell
    (5, 9, 1, 2, dict(tiny=True, argmin=False, automask=0)),
    (20, 36, 2, 4, dict(free=True)),                                 # five-frame window, ragged both ways
    (52, 100, 1, 3, dict(quarter=True, free=True, w_pc=0.5)),        # ragged quarter cell groups
    (375, 1242, 1, 2, dict(n_it=2)),                                 # KITTI raw: 1833 tile records per target, split record sum
    (375, 1242, 1, 2, dict(n_it=1, free=True)),
]


def _case_id(c):
    H, W, B, S, x = c
    return f"{H}x{W}-B{B}-S{S}" + "".join(f"-{k}" for k in ("quarter", "free", "tiny") if x.get(k)) + \
        ("-noargmin" if x.get("argmin") is False else "") + ("-noautomask" if x.get("automask") == 0 else "") + ("-smooth" if x.get("w_smooth") else "") + ("-pc" if x.get("w_pc") else "")


@pytest.mark.parametrize("H,W,B,S,x", CASES, ids=[_case_id(c) for c in CASES])
def test_reference_loss_dense_mode_at_ragged_sizes(H, W, B, S, x, oracle64):
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd import _lib
    n_it, quarter, free, argmin = x.get("n_it", 3), x.get("quarter", False), x.get("free", False), x.get("argmin", True)
    w_smooth, w_pc, automask = x.get("w_smooth", 0.0), x.get("w_pc", 0.0), x.get("automask", 1)
    w = _window(B, S, H, W, seed=41 + H + W)
    N = 2 * S * B
    e = Engine(H, W, N)
    o = default_opts(n_iters=n_it, w_dc=0.15, prior_init=0.1, min_depth=MIND, max_depth=MAXD, window_rule=_lib.WINDOW_REFERENCE, lambda_depth=1.0,
                     depth_param=_lib.DEPTH_QUARTER if quarter else _lib.DEPTH_FULL, free_source_depths=1 if free else 0, w_smooth=w_smooth,
                     w_pose_consist=w_pc, automask=automask)
    t = {k: _dev(v) for k, v in w.items()}
    dt4, ds5 = t["depth_t"][:, None].contiguous(), t["depth_s"][:, :, None].contiguous()
    try:
        (pose, depth, st), bits, _ = PU.traced_and_production(
            e, n_it, N, lambda: e.refine_dense_window(t["tgt"], t["srcs"], dt4, ds5, t["K"], t["pose"], o, stats=True, argmin=argmin))
    except RuntimeError as err:
        assert "internal:" not in str(err), f"{H}x{W}: a valid call refused by the library's own sizing: {err}"
        raise
    pose = pose.cpu().numpy().astype(np.float64); depth = depth.cpu().numpy().astype(np.float64)
    assert np.isfinite(pose).all() and np.isfinite(depth).all() and np.isfinite(st.cpu().numpy()).all()
    fn = {(False, False): oracle64.refine_dense_ref, (True, False): oracle64.refine_dense_ref_q,
          (False, True): oracle64.refine_dense_ref_free, (True, True): oracle64.refine_dense_ref_q_free}[(quarter, free)]
    oracle64.flip_stats_reset()
    res = fn(_f32(w["tgt"]), _f32(w["srcs"]), _f32(w["depth_t"]), _f32(w["depth_s"]), _f32(w["K"]), _f32(w["pose"]),
             oracle_opts(n_iters=n_it, w_dc=0.15, w_smooth=w_smooth, w_pose_consist=w_pc, automask=automask), argmin=argmin, w_init=0.1, lambda_depth=1.0,
             min_depth=MIND, max_depth=MAXD, bits=bits.reshape(n_it, N, H * W))
    po, do = res[0], res[1]
    dso, so = (res[2], res[3]) if free else (None, res[2])
    _check_flips(oracle64, n_it, N * H * W)
    for m in range(N):
        PU.assert_pose(pose[m], po[m], ("pair", m), tol=x.get("pose_tol", PU.POSE_TOL))
    for s in range(S):       # the S forward slots carry the same refined map; every pixel within 1e-4
        rel = np.abs(depth[s * B:(s + 1) * B, 0] / do - 1)
        assert rel.max() < 1e-4, (s, rel.max())
    src_gpu = depth[S * B:, 0].reshape(S, B, H, W)
    if free:                 # every pixel of every source map within 1e-4
        rel = np.abs(src_gpu / dso - 1)
        assert rel.max() < 1e-4, np.sort(rel.ravel())[-6:]
    else:                    # source maps are not unknowns: the inputs come back
        assert np.array_equal(src_gpu, _f32(w["depth_s"]).astype(np.float32).astype(np.float64))
    if not x.get("tiny"):
        assert np.all(np.diff(so[:, 0]) < 0), so[:, 0]                                   # the loss falls
        assert np.abs(depth[0, 0] / _f32(w["depth_t"])[0] - 1).max() > 1e-3               # the map really moved
    else:                    # the linearisation at the start (tolerances of test_gpu_dense_reference.py's)
        ol = default_opts(n_iters=1, w_dc=0.15, prior_init=0.1, min_depth=MIND, max_depth=MAXD, automask=automask)
        L = e.linearize_dense_window(t["tgt"], t["srcs"], dt4, ds5, t["K"], t["pose"], ol, argmin=argmin, depth0=dt4)
        Lo = oracle64.linearize_dense_ref(_f32(w["tgt"]), _f32(w["srcs"]), _f32(w["depth_t"]), _f32(w["depth_s"]), _f32(w["K"]), _f32(w["pose"]),
                                          oracle_opts(n_iters=1, w_dc=0.15, automask=automask), argmin=argmin, w_init=0.1, min_depth=MIND, max_depth=MAXD)
        assert abs(L["loss"] - Lo["loss"]) < 1e-5 * Lo["loss"] and L["K_f"] == Lo["K_f"] and L["K_i"] == Lo["K_i"], (L["loss"], Lo["loss"])
        assert np.abs(L["g_pose"] - Lo["g_xi"]).max() < 2e-4 * np.abs(Lo["g_xi"]).max()
        assert np.abs(L["g_rho"][:, 0].cpu().numpy() - Lo["g_rho"]).max() < 2e-4 * np.abs(Lo["g_rho"]).max()
    e.close()


@pytest.mark.parametrize("shape,kw", [
    ((2, 2, 16, 48), dict(n_iters=3)),                               # LEAN S = 2 joint kernel, half-empty last tile column
    ((1, 3, 64, 208), dict(n_iters=3)),                              # three sources: 18 x 18 systems
    ((1, 2, 33, 70), dict(n_iters=4, solver=1, lambda0=1e-3)),       # LM: one row into a fifth tile row, ragged last column
], ids=["16x48-S2-B2", "64x208-S3", "33x70-S2-lm"])
def test_library_joint_dense_mode_at_ragged_sizes(shape, kw, oracle64):
    """the library's own joint mode (dense_joint = 1, window_rule PAIR) shares k_dense_joint's tile grid: poses and every pixel of the
    shared map follow orc_refine_dense_joint (inverse pairs: orc_refine_dense), decisions replayed, production bits = recording bits"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    import standins
    B, S, H, W = shape
    w = standins.make_window(B, S, H, W, seed0=90)
    w["depth_t"] = oracle64.disp_to_depth(w["disp_t"], MIND, MAXD)[1].astype(np.float32)
    w["depth_s"] = oracle64.disp_to_depth(w["disp_s"], MIND, MAXD)[1].astype(np.float32)
    w["depth_t"] = (w["depth_t"] * (1 + 0.02 * np.sin(np.arange(W) / 11.0))[None, None, None, :]).astype(np.float32)
    e = Engine(H, W, 2 * S * B)
    o = default_opts(w_dc=0.0, min_depth=MIND, max_depth=MAXD, **kw)
    r = PU.replay_window(e, oracle64, w, o, oracle_opts(**kw), _dev, argmin=True, dense=True, joint=True)
    nit = int(o.n_iters)
    assert np.all(r["stats"][:S * B, nit - 1, 0] < r["stats"][:S * B, 0, 0])          # the joint cost goes down
    assert not np.array_equal(r["depth"][0], w["depth_t"][0, 0])                       # and the shared map moved
    e.close()


@pytest.mark.parametrize("quarter", [False, True], ids=["full-resolution", "quarter-resolution"])
def test_merged_reference_loss_calls_at_a_ragged_size(quarter):
    """queued reference-loss calls at 28 x 48 (refused until the joint scratch was sized from the joint grid) merge into one launch sequence
    whose every call returns the bits of the call on its own (test_gpu_coalesce.py, at tile-exact sizes)"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd import _lib
    H, W, S, B = 28, 48, 2, 1
    N = 2 * S * B
    calls = []
    for i in range(6):
        w = _window(B, S, H, W, seed=300 + 13 * i)
        t = {k: _dev(v) for k, v in w.items()}
        calls.append((t["tgt"], t["srcs"], t["depth_t"][:, None].contiguous(), t["depth_s"][:, :, None].contiguous(), t["K"], t["pose"]))
    o = default_opts(n_iters=3, w_dc=0.15, prior_init=0.1, min_depth=MIND, max_depth=MAXD, window_rule=_lib.WINDOW_REFERENCE,
                     depth_param=_lib.DEPTH_QUARTER if quarter else _lib.DEPTH_FULL)
    o.argmin = 1
    ref = Engine(H, W, N)
    want = []
    for c in calls:
        p, d, _ = ref.refine_dense_window(*c, o, argmin=True)
        want.append((p.clone(), d.clone()))
    torch.cuda.synchronize()
    e = Engine(H, W, N * 4, lanes=2)
    e.set_coalesce(4); e.set_coalesce_lanes(2)
    po = [torch.zeros(N, 6, device="cuda") for _ in calls]
    do = [torch.zeros(N, 1, H, W, device="cuda") for _ in calls]
    for c, p, d in zip(calls, po, do):
        e.refine_dense_window_queued(*c, p, d, o)
    assert e.coalesce_counts() == (1, 4)                 # four calls ran as one sequence, two are waiting
    e.synchronize()
    assert e.coalesce_counts() == (2, 6)
    for i, ((wp, wd), p, d) in enumerate(zip(want, po, do)):
        assert torch.equal(p, wp), (i, (p - wp).abs().max())
        assert torch.equal(d, wd), (i, (d - wd).abs().max())
    e.set_coalesce_lanes(1); e.set_coalesce(0)
    e.close(); ref.close()
