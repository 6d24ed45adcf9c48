"""Shared machinery of the GPU parity tests: tie-proof comparison of the HIP engine with the float64 oracle.

The reference's residual has discontinuous decisions -- the auto-mask `diff < auto_err` (helpers.py:17-19), the warp validity
(stn.py:268-269), the per-pixel min over the sources (optimizer.py:47-69) -- and LM adds accept / reject on a cost comparison.
Near a tie the fp32 engine and a float64 checker may decide differently, after which the two trajectories are simply different
problems.  Instead of loosening the tolerance in such cases, every iterate-level test here does BOTH of

  (1) REPLAY: the engine records its decisions (tcsfm_debug_trace: per linearisation and pixel one byte -- mask, warp validity,
      parity of the bilinear cell (grid_sample's backward is discontinuous across texel boundaries), sign of cd - pd and of
      rec - tgt per channel (the kinks of the depth-consistency and L1 terms); per linearisation the LM decision); the oracle
      re-runs the refinement with exactly these decisions and the results are compared at the north-star tolerance (1e-4
      relative on translation, rotation, depth scale, per-pixel depth) in EVERY case.  Measured effect of NOT replaying: three
      texel-boundary ties in 4 iterations of a 96x320 pair move the weakest rotation component by 3.5e-4 (reproduced on the CPU
      by flipping those three bits in the oracle's own trace);
  (2) DECISIONS: the engine's decisions themselves are checked against the oracle's own AT EVERY LINEARISATION: while it replays, the
      oracle also takes every mask decision itself at its (replayed) iterate and counts the pixels it would have decided
      differently, and those of them that are not near-ties (Oracle.flip_stats; the iterates agree to ~1e-6, so beyond ties the
      decisions must agree -- a kernel bug that corrupts masks only after the first pose update, e.g. a stale PairConst or a
      wrong ping-pong buffer, fails here at linearisation >= 1): none may be hard, and their number is bounded; at the first
      linearisation additionally against Oracle.photometric; every LM decision that differs from what the oracle's costs imply
      must be a near-tie of the two costs.
"""
import numpy as np
import torch

POSE_TOL = 1e-4          # BASELINE.json: pose translations / rotations within 1e-4 relative
COST_TOL = 2e-5          # cost at every linearisation, relative
TIE_TOL = 5e-5           # |diff - auto_err| of a pixel the two sides may legitimately decide differently (fp32 SSIM: ~1e-5)
DEPTH_TOL = 1e-4         # BASELINE.json: per-pixel depth within 1e-4 relative
COST_TIE = 2e-5          # relative cost difference below which an LM decision may legitimately differ


def assert_depth(depth, ref, tag=None):
    """per-pixel depth against the replayed oracle: 1e-4 relative on EVERY pixel.  A pixel's own depth update is driven by that
    pixel's derivative alone, so one discrete decision taken differently shows up at full size at that pixel (measured: 1e-4 ..
    5e-3) while everything else agrees to ~1e-6 -- which is why the trace carries every such decision of the residual's
    derivative: mask, validity, the bilinear cell, and the signs of the L1 and depth-consistency terms."""
    rel = np.abs(np.asarray(depth, np.float64) / ref - 1)
    assert rel.max() < DEPTH_TOL, (tag, int((rel >= DEPTH_TOL).sum()), float(rel.max()))
    assert np.quantile(rel, 0.999) < 1e-5, (tag, float(np.quantile(rel, 0.999)))       # the bulk is two orders tighter than the bar
    return 0


def n_lin(o):
    """linearisations of one refine call: n_iters, plus LM's final cost check"""
    return int(o.n_iters) + (1 if int(o.solver) == 1 and int(o.n_iters) > 0 else 0)


def pose_err(p, r):
    p, r = np.asarray(p, np.float64), np.asarray(r, np.float64)
    return (np.linalg.norm(p[:3] - r[:3]) / np.linalg.norm(r[:3]), np.linalg.norm(p[3:] - r[3:]) / np.linalg.norm(r[3:]))


def assert_pose(p, r, tag=None, tol=POSE_TOL):
    et, er = pose_err(p, r)
    assert et < tol and er < tol, (tag, et, er, p, r)


def check_lm_decisions(rst, dec, o, tag=None):
    """the engine's accept / keep decisions against the costs of the replayed float64 run: a decision may differ from
    `cost < accepted cost` only when the two costs tie to rounding"""
    if int(o.solver) != 1 or int(o.n_iters) == 0:
        return 0
    cur, flips = rst[0, 0], 0
    for it in range(1, int(o.n_iters) + 1):
        c = rst[it, 0]
        want = c < cur
        if bool(dec[it]) != want:
            flips += 1
            assert abs(c - cur) <= COST_TIE * cur, (tag, it, c, cur, dec)
        if dec[it] and it < int(o.n_iters):
            cur = c
    return flips


def check_first_masks(bits0, ph, automask, tag=None, max_frac=1e-3):
    """decisions of the FIRST linearisation (identical pose on both sides) against the oracle's own maps `ph`
    (Oracle.photometric): flipped pixels must be near-ties of diff vs auto_err (or validity ties on the border of the
    valid region) and rare.  -> number of flipped pixels"""
    valid_o = ph["valid"] > 0.5
    m_o = valid_o & ((ph["diff"] < ph["auto_err"]) if automask else True)
    m_e, valid_e = (bits0 & 1) > 0, (bits0 & 2) > 0
    vflip = valid_e != valid_o
    flip = (m_e != m_o)
    tie = np.abs(ph["diff"] - ph["auto_err"]) < TIE_TOL
    assert np.all(~flip | tie | vflip), (tag, int(flip.sum()), float(np.abs(ph["diff"] - ph["auto_err"])[flip & ~vflip].max()))
    assert vflip.sum() <= 2 + 2e-4 * flip.size, (tag, int(vflip.sum()))
    assert flip.sum() <= 2 + max_frac * flip.size, (tag, int(flip.sum()))
    return int(flip.sum())


def _flip_report(tag, kind, frac, allowed):
    """TCSFM_TEST_FLIP_REPORT=<file>: append the measured flip fraction of every check (how much of the allowance the near-ties really use)"""
    import os
    f = os.environ.get("TCSFM_TEST_FLIP_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{tag}\t{kind}\t{frac:.3e}\t{allowed:.1e}\n")


def check_dense_ref_flips(nf, hard, pixels, max_frac=5e-4):
    """dense mode on the reference's loss: no hard flip, at most max_frac of the decisions of a linearisation flip as near-ties"""
    _flip_report("dense_ref", "every_lin", float(np.max(nf)) / pixels if len(nf) else 0.0, max_frac)
    assert hard.sum() == 0 and nf.max() <= max_frac * pixels, (nf, hard)


def check_flips_every_linearisation(orc, nit, pixels, tag=None, max_frac=5e-5):
    """after forced replays covering `pixels` mask decisions per linearisation: per linearisation, no hard (non-tie) flip and at
    most 2 + max_frac * pixels flips in all -> total number of flips.  The allowance was 1e-3 / 2e-3 until round 5; measured over the whole
    GPU suite (profiles/r05_flip_report.tsv, TCSFM_TEST_FLIP_REPORT): at most 8.1e-6 of the decisions are near-ties that flip"""
    fn, fh = orc.flip_stats(nit)
    _flip_report(tag, "every_lin", float(np.max(fn)) / pixels if len(fn) else 0.0, max_frac)
    assert not fh.any(), (tag, "non-tie mask flips per linearisation", fh.tolist(), fn.tolist())
    assert np.all(fn <= 2 + max_frac * pixels), (tag, fn.tolist(), pixels)
    return int(fn.sum())


def traced_and_production(e, n_lin, n_pairs, call):
    """PRODUCTION == RECORDING: `call()` -- one Engine.refine* call -> tuple of output tensors (poses, depth maps or log-scales,
    stats; None where absent) -- runs once with the decision trace on (the TRACE = true instantiations of the kernels, whose decisions
    the oracle replays) and once with it off (the TRACE = false ones users and bench.py run: compiled separately, registers allocated
    differently).  Every output must be the same bits, so that every oracle comparison of the traced run vouches for the production
    kernels.  -> (traced outputs, bits, decide)"""
    e.trace_begin(n_lin, n_pairs)
    traced = call()
    bits, dec = e.trace_end()
    prod = call()
    assert len(traced) == len(prod)
    for i, (a, p) in enumerate(zip(traced, prod)):
        assert (a is None) == (p is None), i
        if a is not None:
            assert torch.equal(a, p), ("production kernels differ from the recording ones: output", i,
                                       int((a != p).sum()), float((a.double() - p.double()).abs().max()))
    return traced, bits, dec


def replay_pairs(e, orc, b, o, oopts, tdev, log_scale=None, pose_key="pose_init", first_masks=True):
    """N directed pairs through Engine.refine with the decision trace on, then the oracle replay per pair.
    b: synth batch (numpy); o: engine opts; oopts: oracle opts; tdev: numpy -> cuda tensor.  -> dict of results"""
    N = b["tgt"].shape[0]
    nl, nit = n_lin(o), int(o.n_iters)
    refine = int(o.refine)
    args = (tdev(b["tgt"]), tdev(b["src"]), tdev(b["depth_t"]), tdev(b["depth_s"]), tdev(b["K"]), tdev(b[pose_key]))
    (pose, ls, st), bits, dec = traced_and_production(e, nl, N, lambda: e.refine(*args, o, log_scale=tdev(log_scale) if refine else None, stats=True))
    pose, st = pose.cpu().numpy().astype(np.float64), st.cpu().numpy()
    ls = ls.cpu().numpy() if refine else None
    out = dict(pose=pose, stats=st, bits=bits, decide=dec, log_scale=ls, ref_pose=[], ref_stats=[], mask_flips=0, lm_flips=0)
    orc.flip_stats_reset()
    for n in range(N):
        a = (b["tgt"][n], b["src"][n], b["depth_t"][n, 0], b["depth_s"][n, 0], b[pose_key][n], b["K"][n])
        s0 = float(log_scale[n]) if refine else 0.0
        rp, rls, rst = orc.refine(*a, oopts, log_scale=s0, bits=bits[:, n], decide=dec[:, n])
        assert_pose(pose[n], rp, ("pair", n))
        if refine:       # depth = exp(log_scale) * depth0: 1e-4 relative on every depth value
            assert abs(float(ls[n]) - rls) < POSE_TOL, (n, float(ls[n]), rls)
        rows = nit + (1 if int(o.solver) == 1 and nit > 0 else 0)
        assert np.max(np.abs(st[n, :rows, 0] - rst[:rows, 0]) / rst[:rows, 0]) < COST_TOL, (n, st[n, :rows, 0], rst[:rows, 0])
        assert np.array_equal(st[n, :nit, 2], rst[:nit, 2])                  # the replay really used the engine's masks
        assert np.array_equal(rst[:nit, 2], (bits[:nit, n] & 1).sum((1, 2)))
        out["lm_flips"] += check_lm_decisions(rst, dec[:, n], o, ("pair", n))
        if first_masks and nit > 0:
            ph = orc.photometric(*a[:4], a[4], a[5], log_scale=s0, w_l1=float(o.w_l1), w_ssim=float(o.w_ssim))
            out["mask_flips"] += check_first_masks(bits[0, n], ph, int(o.automask), ("pair", n))
        out["ref_pose"].append(rp); out["ref_stats"].append(rst)
    out["flips_all_lin"] = check_flips_every_linearisation(orc, nit, N * bits.shape[-1] * bits.shape[-2], "pairs")
    return out


def window_pair_views(w):
    """(tgt, src, depth_t, depth_s, K) numpy views of the 2*S*B directed pairs of a window, stacked order of train_mono.py:54-62"""
    S, B = w["sources"].shape[:2]
    out = []
    for m in range(2 * S * B):
        inv, q = m >= S * B, m % (S * B)
        s, bb = q // B, q % B
        t, sr, dt, ds = w["target"][bb], w["sources"][s, bb], w["depth_t"][bb, 0], w["depth_s"][s, bb, 0]
        out.append((sr, t, ds, dt, w["K"][bb]) if inv else (t, sr, dt, ds, w["K"][bb]))
    return out


def replay_window(e, orc, w, o, oopts, tdev, argmin=True, dense=False, log_scale=None, max_flip_frac=5e-5, rule=0, joint=False):
    """a window (B targets x S sources -> 2*S*B directed pairs) through Engine.refine_window / refine_dense_window with the
    decision trace on, then ONE oracle replay of the whole window.  w: dict(target, sources, depth_t, depth_s, K, first)."""
    S, B = w["sources"].shape[:2]
    N = 2 * S * B
    H, W = w["target"].shape[2:]
    nl, nit = n_lin(o), int(o.n_iters)
    refine = int(o.refine)
    args = tuple(tdev(w[k]) for k in ("target", "sources", "depth_t", "depth_s", "K", "first"))
    oargs = (w["target"], w["sources"], w["depth_t"][:, 0], w["depth_s"][:, :, 0], w["K"], w["first"])
    depth = ls = None
    if dense:
        import ctypes as _C
        o2 = type(o)(); _C.memmove(_C.byref(o2), _C.byref(o), _C.sizeof(o2)); o = o2
        o.dense_joint = 1 if joint else 0            # joint: one depth map per target shared by its S forward pairs (tcsfm.h)
        o.window_rule = 0
        (pose, depth, st), bits, dec = traced_and_production(e, nl, N, lambda: e.refine_dense_window(*args, o, stats=True, argmin=argmin))
        depth = depth.cpu().numpy()[:, 0]
    else:
        (pose, ls, st), bits, dec = traced_and_production(
            e, nl, N, lambda: e.refine_window(*args, o, stats=True, argmin=argmin, log_scale=tdev(log_scale) if refine else None))
        ls = ls.cpu().numpy() if refine else None
    pose, st = pose.cpu().numpy().astype(np.float64), st.cpu().numpy()
    orc.flip_stats_reset()
    if dense and joint:
        # forward group: the joint oracle (shared depth, 6S x 6S reduced system); inverse pairs: the pair-form dense oracle
        SB = S * B
        kwj = dict(lambda_depth=float(o.lambda_depth), w_prior=float(o.prior_depth), min_depth=float(o.min_depth), max_depth=float(o.max_depth))
        pf, df, sf = orc.refine_dense_joint(w["target"], w["sources"], w["depth_t"][:, 0], w["depth_s"][:, :, 0], w["K"], w["first"][:SB], oopts,
                                            argmin=argmin, rule=rule, bits=bits[:, :SB], decide=dec[:, :SB], **kwj)
        rp, rd, rst = np.zeros((N, 6)), np.zeros((N, H, W)), np.zeros((N, nit + 1, 4))
        rp[:SB], rst[:SB] = pf, sf
        for m in range(SB):
            rd[m] = df[m % B]
        views = window_pair_views(w)
        for m in range(SB, N):
            t, sr, dt, ds, K = views[m]
            rp[m], rd[m], rst[m] = orc.refine_dense(t, sr, dt, ds, w["first"][m], K, oopts, bits=bits[:, m], decide=dec[:, m], **kwj)
        rls = None
        assert all(np.array_equal(depth[s_ * B + b_], depth[b_]) for s_ in range(S) for b_ in range(B))     # the S forward slots hold ONE map
    elif dense:
        rp, rd, rst = orc.refine_dense_window(*oargs, oopts, argmin=argmin, lambda_depth=float(o.lambda_depth), w_prior=float(o.prior_depth),
                                              min_depth=float(o.min_depth), max_depth=float(o.max_depth), bits=bits, decide=dec)
        rls = None
    else:
        rp, rls, rst = orc.refine_window(*oargs, oopts, argmin=argmin, log_scale=np.asarray(log_scale, np.float64) if refine else None,
                                         bits=bits, decide=dec, rule=rule)
        rd = None
    flips_all = check_flips_every_linearisation(orc, nit, N * H * W, "window", max_frac=max_flip_frac)
    rows = nit + (1 if int(o.solver) == 1 and nit > 0 else 0)
    lm_flips = 0
    for n in range(N):
        assert_pose(pose[n], rp[n], ("window pair", n))
        if refine:
            assert abs(float(ls[n]) - rls[n]) < POSE_TOL
        assert np.max(np.abs(st[n, :rows, 0] - rst[n, :rows, 0]) / rst[n, :rows, 0]) < COST_TOL, (n, st[n, :rows, 0], rst[n, :rows, 0])
        assert np.array_equal(st[n, :nit, 2], rst[n, :nit, 2])
        lm_flips += check_lm_decisions(rst[n], dec[:, n], o, ("window pair", n))
        if dense:    # per-pixel depth within 1e-4 relative (BASELINE.json): the decisions are the same on both sides
            assert_depth(depth[n], rd[n], ("window pair", n))
    # decisions of the first linearisation against the oracle's own (same poses): count only -- with the min over the sources a
    # flip is a near-tie between two sources' errors or between the minimum and the auto-mask threshold
    flips = 0
    if nit > 0:
        own = np.zeros((N, H, W), bool)
        views = window_pair_views(w)
        ls0 = np.zeros(N) if log_scale is None else np.asarray(log_scale, np.float64)
        for n in range(N):
            t, sr, dt, ds, K = views[n]
            ph = orc.photometric(t, sr, dt, ds, w["first"][n], K, log_scale=float(ls0[n]), w_l1=float(o.w_l1), w_ssim=float(o.w_ssim))
            # REFERENCE rule / joint dense mode without argmin: no auto-mask on the forward term (optimizer.py:71-73)
            am = int(o.automask) and not ((rule == 1 or (dense and joint)) and not argmin and n < S * B)
            own[n] = (ph["valid"] > 0.5) & ((ph["diff"] < ph["auto_err"]) if am else True)
        if argmin and S > 1:
            if refine and np.any(ls0 != 0):
                own[:S * B] = (bits[0, :S * B] & 1) > 0      # (the select helper has no depth-scale argument)
            else:
                own[:S * B] = orc.window_select(w["target"], w["sources"], w["depth_t"][:, 0], w["depth_s"][:, :, 0], w["K"],
                                                w["first"][:S * B], oopts) > 0.5
        flip = ((bits[0] & 1) > 0) != own
        flips = int(flip.sum())
        _flip_report("window", "first_lin_vs_own", flips / flip.size, max_flip_frac)
        assert flips <= 2 * N + max_flip_frac * flip.size, (flips, flip.sum((1, 2)))
    return dict(pose=pose, stats=st, bits=bits, decide=dec, depth=depth, ref_pose=rp, ref_stats=rst, ref_depth=rd, log_scale=ls,
                mask_flips=flips, lm_flips=lm_flips, flips_all_lin=flips_all)


def replay_dense_pairs(e, orc, b, d0, o, oopts, tdev, pose_key="pose_init", poses=None):
    """N directed pairs through Engine.refine_dense (initial target depth d0 [N,1,H,W]) with the trace on + oracle replay"""
    N = b["tgt"].shape[0]
    nl, nit = n_lin(o), int(o.n_iters)
    p0 = b[pose_key] if poses is None else poses
    (pose, depth, st), bits, dec = traced_and_production(
        e, nl, N, lambda: e.refine_dense(tdev(b["tgt"]), tdev(b["src"]), tdev(d0), tdev(b["depth_s"]), tdev(b["K"]), tdev(p0), o, stats=True))
    pose, depth, st = pose.cpu().numpy().astype(np.float64), depth.cpu().numpy()[:, 0], st.cpu().numpy()
    rows = nit + (1 if int(o.solver) == 1 and nit > 0 else 0)
    out = dict(pose=pose, depth=depth, stats=st, bits=bits, decide=dec, ref_pose=[], ref_depth=[], ref_stats=[], mask_flips=0, lm_flips=0)
    orc.flip_stats_reset()
    for n in range(N):
        rp, rd, rst = orc.refine_dense(b["tgt"][n], b["src"][n], d0[n, 0], b["depth_s"][n, 0], p0[n], b["K"][n], oopts,
                                       lambda_depth=float(o.lambda_depth), w_prior=float(o.prior_depth), min_depth=float(o.min_depth),
                                       max_depth=float(o.max_depth), bits=bits[:, n], decide=dec[:, n])
        assert_pose(pose[n], rp, ("dense pair", n))
        assert_depth(depth[n], rd, ("dense pair", n))                                          # per-pixel depth
        assert np.max(np.abs(st[n, :rows, 0] - rst[:rows, 0]) / rst[:rows, 0]) < 5e-5, (n, st[n, :rows, 0], rst[:rows, 0])
        assert np.array_equal(st[n, :nit, 2], rst[:nit, 2])
        out["lm_flips"] += check_lm_decisions(rst, dec[:, n], o, ("dense pair", n))
        if nit > 0:
            ph = orc.photometric(b["tgt"][n], b["src"][n], d0[n, 0], b["depth_s"][n, 0], p0[n], b["K"][n], w_l1=float(o.w_l1), w_ssim=float(o.w_ssim))
            out["mask_flips"] += check_first_masks(bits[0, n], ph, int(o.automask), ("dense pair", n))
        out["ref_pose"].append(rp); out["ref_depth"].append(rd); out["ref_stats"].append(rst)
    out["flips_all_lin"] = check_flips_every_linearisation(orc, nit, N * bits.shape[-1] * bits.shape[-2], "dense pairs")
    return out
