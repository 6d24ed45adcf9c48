#!/usr/bin/env python3
"""Run every pose entry point once at two tiny shapes and print a SHA-256 of each output: two builds whose lines agree compute the same bits.
    python scripts/pose_bits.py > bits.txt
Modes: tcsfm_refine (Gauss-Newton and LM, pose and pose + scale, with and without the depth-consistency term, no iteration),
tcsfm_refine_window at S = 1, 2, 4 with and without the min over the sources under both window rules, tcsfm_linearize,
tcsfm_linearize_window, tcsfm_loss_surface, host-pointer calls (host_ptrs = 1, and 2 through the _async form), a merged pair of pose
calls and of pose + scale calls, the _async form on lane 1, and one call under graph replay (three sightings: plain run, capture,
replay).  One refinement and one linearisation run at 208 x 640: 260 tiles, above the 256 tiles up to which the solve kernel sums the
workgroup records itself, so the two-level reduction is covered too."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tightly_coupled_sfm_amd import _lib, synth
from tightly_coupled_sfm_amd.engine import Engine, default_opts

MAX_PAIRS, B = 16, 2
BASE = dict(n_iters=2)


def sha(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def window(H, W, S, nb=B, seed=3):
    """host arrays of a window call: tgt [nb], srcs [S, nb], depth_t [nb, 1], depth_s [S, nb, 1], K [nb], pose [2 S nb]"""
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(nb):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0, -1.0, 1.6, -1.6)[s]
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return (f32(np.stack(tg)), f32(np.stack([np.stack(x) for x in sr])), f32(np.stack(dt)[:, None]), f32(np.stack([np.stack(x) for x in ds])[:, :, None]), f32(np.stack(K)),
            f32(np.concatenate([fwd, -fwd])))


def dev(arrays):
    return tuple(torch.as_tensor(a).cuda() for a in arrays)


def pairs_of(w):
    """the pair form of an S = 1 window's forward pairs"""
    tgt, srcs, dt, ds, K, pose = w
    c = (lambda a: a.contiguous()) if isinstance(tgt, torch.Tensor) else np.ascontiguousarray
    return tgt, c(srcs[0]), dt, c(ds[0]), K, c(pose[:tgt.shape[0]])


def lin_outs(r):
    return dict(H=r["H"], g=r["g"], stats=np.stack([r["cost"], r["cost_photo"], r["cost_dc"], r["n_mask"]]))


def main():
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    P = lambda t: C.c_void_p(t.data_ptr())
    for H, W in ((17, 33), (37, 53)):
        eng = Engine(H, W, MAX_PAIRS, lanes=2)
        host = {S: window(H, W, S) for S in (1, 2, 4)}
        wins = {S: dev(host[S]) for S in host}

        def show(name, **outs):
            for k, v in outs.items():
                if v is not None:
                    print(f"{H}x{W} {name} {k} {sha(v)}")

        pr = pairs_of(wins[1])
        ls = torch.full((B,), 0.03, device="cuda")
        for solver, sn in ((_lib.SOLVER_GN, "GN"), (_lib.SOLVER_LM, "LM")):
            for refine, rn in ((_lib.REFINE_POSE, "pose"), (_lib.REFINE_POSE_SCALE, "pose+scale")):
                for w_dc in (0.0, 0.15):
                    o = default_opts(solver=solver, refine=refine, w_dc=w_dc, **BASE)
                    pose, lso, st = eng.refine(*pr, o, log_scale=ls if refine else None, stats=True)
                    torch.cuda.synchronize()
                    show(f"refine {sn} {rn} w_dc={w_dc}", pose=pose, log_scale=lso, stats=st)
                o = default_opts(solver=solver, refine=refine, n_iters=0)
                pose, lso, st = eng.refine(*pr, o, log_scale=ls if refine else None, stats=True)
                torch.cuda.synchronize()
                show(f"refine {sn} {rn} no iteration", pose=pose, log_scale=lso, stats=st)
        for S in (1, 2, 4):
            for rule, rname in ((_lib.WINDOW_PAIR, "pair rule"), (_lib.WINDOW_REFERENCE, "reference rule")):
                for am in (0, 1):
                    o = default_opts(window_rule=rule, argmin=am, w_dc=0.15, **BASE)
                    pose, _, st = eng.refine_window(*wins[S], o, stats=True)
                    torch.cuda.synchronize()
                    show(f"refine_window S={S} {rname} argmin={am}", pose=pose, stats=st)
                    show(f"linearize_window S={S} {rname} argmin={am}", **lin_outs(eng.linearize_window(*wins[S], o)))
            o = default_opts(refine=_lib.REFINE_POSE_SCALE, solver=_lib.SOLVER_LM, argmin=1, **BASE)
            ls_w = torch.full((2 * S * B,), -0.02, device="cuda")
            pose, lso, _ = eng.refine_window(*wins[S], o, log_scale=ls_w)
            torch.cuda.synchronize()
            show(f"refine_window S={S} LM pose+scale", pose=pose, log_scale=lso)
            show(f"linearize_window S={S} pose+scale", **lin_outs(eng.linearize_window(*wins[S], o, log_scale=ls_w)))
        for refine, rn in ((_lib.REFINE_POSE, "pose"), (_lib.REFINE_POSE_SCALE, "pose+scale")):
            for w_dc in (0.0, 0.15):
                o = default_opts(refine=refine, w_dc=w_dc)
                show(f"linearize {rn} w_dc={w_dc}", **lin_outs(eng.linearize(*pr, o, log_scale=ls if refine else None)))
        poses = torch.as_tensor(np.float32(host[1][5][:1] + np.linspace(-0.01, 0.01, 5)[:, None] * np.float32([1, 0, 0, 0, 0.5, 0]))).cuda()
        show("loss_surface", cost=eng.loss_surface(pr[0][:1], pr[1][:1], pr[2][:1], pr[3][:1], pr[4][:1], poses, default_opts(w_dc=0.15)))

        # host pointers: staged by the library (1), and pinned + asynchronous through the _async form on a lane (2)
        tg, sr, dt, ds, K, p0 = host[2]
        o = default_opts(host_ptrs=1, argmin=1, **BASE)
        out, st = np.zeros((2 * 2 * B, 6), np.float32), np.zeros((2 * 2 * B, 3, _lib.NSTAT), np.float32)
        eng._call(eng.lib.tcsfm_refine_window(eng._h, C.byref(o), B, 2, ptr(tg), ptr(sr), ptr(dt), ptr(ds), ptr(K), ptr(p0), None, ptr(out), None, ptr(st)))
        show("host_ptrs=1 refine_window S=2", pose=out, stats=st)
        tg, sr, dt, ds, K, p0 = pairs_of(host[1])
        out = np.zeros((B, 6), np.float32)
        eng._call(eng.lib.tcsfm_refine(eng._h, C.byref(o), B, ptr(tg), ptr(sr), ptr(dt), ptr(ds), ptr(K), ptr(p0), None, ptr(out), None, None))
        show("host_ptrs=1 refine", pose=out)
        pinned = [torch.as_tensor(a).pin_memory() for a in host[1]]
        out = torch.zeros(2 * B, 6).pin_memory()
        o2 = default_opts(host_ptrs=2, **BASE)
        eng._call(eng.lib.tcsfm_refine_window_async(eng._h, 1, C.byref(o2), B, 1, *(P(t) for t in pinned), None, P(out), None, None))
        eng.lane_synchronize(1)
        show("host_ptrs=2 refine_window_async lane 1", pose=out)

        # the _async form on lane 1, device pointers
        o = default_opts(w_dc=0.15, **BASE)
        out = torch.zeros(2 * 2 * B, 6, device="cuda")
        eng.refine_window_async(1, *wins[2], out, o)
        eng.lane_synchronize(1); torch.cuda.synchronize()
        show("refine_window_async lane 1 S=2", pose=out)

        # a merged pair of calls: two one-target windows of one shape queued, run as one launch sequence
        for name, refine in (("pose", _lib.REFINE_POSE), ("pose+scale", _lib.REFINE_POSE_SCALE)):
            for S in (1, 2):
                o = default_opts(refine=refine, argmin=1, **BASE)
                tgt, srcs, dt, ds, K, pose = wins[S]
                calls = []
                for b in range(B):
                    idx = [s * B + b for s in range(S)] + [S * B + s * B + b for s in range(S)]
                    calls.append((tgt[b:b + 1].contiguous(), srcs[:, b:b + 1].contiguous(), dt[b:b + 1].contiguous(), ds[:, b:b + 1].contiguous(), K[b:b + 1].contiguous(),
                                  pose[idx].contiguous(), torch.full((2 * S,), 0.01 * (b + 1), device="cuda"), torch.zeros(2 * S, 6, device="cuda"), torch.zeros(2 * S, device="cuda")))
                eng.set_coalesce(B)
                for c in calls:
                    if refine:
                        eng.refine_window_scale_queued(*c, o)
                    else:
                        eng.refine_window_queued(*c[:6], c[7], o)
                eng.flush(); torch.cuda.synchronize()
                eng.set_coalesce(0)
                for b, c in enumerate(calls):
                    show(f"merged {name} S={S} call {b}", pose=c[7], log_scale=c[8] if refine else None)
                print(f"{H}x{W} merged {name} S={S} sequences/calls so far {'/'.join(map(str, eng.coalesce_counts()))}")

        # one call under graph replay: the same tensors three times
        eng.use_own_stream()          # (a capture needs a stream of its own, not the default stream)
        eng.set_graph_replay(4)
        for name, S, o in (("pose S=2", 2, default_opts(argmin=1, w_dc=0.15, **BASE)), ("pose+scale S=1 LM", 1, default_opts(refine=_lib.REFINE_POSE_SCALE, solver=_lib.SOLVER_LM, **BASE))):
            po, lo = torch.zeros(2 * S * B, 6, device="cuda"), torch.zeros(2 * S * B, device="cuda")
            li = torch.full((2 * S * B,), 0.02, device="cuda")
            for sighting in range(3):
                po.zero_(); lo.zero_(); torch.cuda.synchronize()
                eng.refine_window_async(0, *wins[S], po, o, log_scale=li if o.refine else None, log_scale_out=lo if o.refine else None)
                eng.synchronize(); torch.cuda.synchronize()
                show(f"graph replay {name} sighting {sighting}", pose=po, log_scale=lo if o.refine else None)
        print(f"{H}x{W} graph replay captures/replays {'/'.join(map(str, eng.graph_replay_counts()))}")
        eng.set_graph_replay(0)
        eng.close()

    H, W = 208, 640                   # 260 tiles: the two-level reduction of the workgroup records
    eng = Engine(H, W, 2)
    pr = pairs_of(dev(window(H, W, 1, nb=1)))
    o = default_opts(w_dc=0.15, **BASE)
    pose, _, st = eng.refine(*pr, o, stats=True)
    torch.cuda.synchronize()
    print(f"{H}x{W} refine GN pose w_dc=0.15 pose {sha(pose)}")
    print(f"{H}x{W} refine GN pose w_dc=0.15 stats {sha(st)}")
    for k, v in lin_outs(eng.linearize(*pr, o)).items():
        print(f"{H}x{W} linearize pose w_dc=0.15 {k} {sha(v)}")
    eng.close()


if __name__ == "__main__":
    main()
