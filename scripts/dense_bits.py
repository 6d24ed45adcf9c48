#!/usr/bin/env python3
"""Run every dense mode once at two tiny shapes and print a SHA-256 of each output: two builds whose lines agree compute the same bits.
    python scripts/dense_bits.py > bits.txt
Modes: the pair form (Gauss-Newton and LM, with and without the min over the sources), the library's joint mode (S = 2, 3), the
reference's loss at S = 1 .. 4 with and without the quarter-resolution unknown, free source maps, l_smooth and l_pose_consist, both
exports, a merged pair of calls of either kind, and one call under graph replay (three sightings: plain run, capture, replay)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tightly_coupled_sfm_amd import _lib, synth
from tightly_coupled_sfm_amd.engine import Engine, default_opts

MAX_PAIRS, B = 16, 2
BASE = dict(n_iters=2, min_depth=0.06, max_depth=2.67)


def sha(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def window(H, W, S, seed=3):
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0, -1.0, 1.6, -1.6)[s]
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return (dev(np.stack(tg)), dev(np.stack([np.stack(x) for x in sr])), dev(np.stack(dt)[:, None]), dev(np.stack([np.stack(x) for x in ds])[:, :, None]), dev(np.stack(K)),
            dev(np.concatenate([fwd, -fwd])))


def main():
    for H, W in ((16, 48), (28, 48)):
        eng = Engine(H, W, MAX_PAIRS)
        wins = {S: window(H, W, S) for S in (1, 2, 3, 4)}

        def show(name, **outs):
            for k, v in outs.items():
                print(f"{H}x{W} {name} {k} {sha(v)}")

        def refine(name, S, o, stats=False):
            pose, depth, st = eng.refine_dense_window(*wins[S], o, stats=stats)
            torch.cuda.synchronize()
            show(name, pose=pose, depth=depth, **({"stats": st} if stats else {}))

        w1 = wins[1]
        pose, depth, _ = eng.refine_dense(w1[0], w1[1][0], w1[2], w1[3][0], w1[4], w1[5][:B], default_opts(**BASE))
        show("pair form, no window, GN", pose=pose, depth=depth)
        for solver, sn in ((_lib.SOLVER_GN, "GN"), (_lib.SOLVER_LM, "LM")):
            for am in (0, 1):
                refine(f"pair form S=2 {sn} argmin={am}", 2, default_opts(dense_joint=0, solver=solver, argmin=am, **BASE), stats=bool(am))
            refine(f"pair form S=4 {sn} argmin=1", 4, default_opts(dense_joint=1, solver=solver, argmin=1, **BASE))      # (wider than the joint mode takes)
            for S in (2, 3):
                for am in (0, 1):
                    refine(f"joint mode S={S} {sn} argmin={am}", S, default_opts(dense_joint=1, solver=solver, argmin=am, **BASE), stats=S == 2)
        ref = dict(window_rule=_lib.WINDOW_REFERENCE, w_dc=0.5, **BASE)
        for S in (1, 2, 3, 4):
            refine(f"reference loss S={S} plain argmin=1", S, default_opts(argmin=1, **ref), stats=True)
            refine(f"reference loss S={S} plain argmin=0", S, default_opts(argmin=0, **ref))
            refine(f"reference loss S={S} quarter", S, default_opts(depth_param=_lib.DEPTH_QUARTER, **ref))
            refine(f"reference loss S={S} free sources", S, default_opts(free_source_depths=1, **ref), stats=True)
            refine(f"reference loss S={S} smooth", S, default_opts(w_smooth=2.0, **ref))
            refine(f"reference loss S={S} pose consistency", S, default_opts(w_pose_consist=0.5, **ref))
            refine(f"reference loss S={S} quarter + free sources", S, default_opts(depth_param=_lib.DEPTH_QUARTER, free_source_depths=1, **ref))
            refine(f"reference loss S={S} free sources + smooth + pose consistency", S, default_opts(free_source_depths=1, w_smooth=2.0, w_pose_consist=0.5, **ref))
            refine(f"reference loss S={S} all four, no iteration", S, default_opts(depth_param=_lib.DEPTH_QUARTER, free_source_depths=1, w_smooth=2.0, w_pose_consist=0.5,
                                                                                  window_rule=_lib.WINDOW_REFERENCE, n_iters=0, min_depth=0.06, max_depth=2.67))
            for sources in (False, True):
                r = eng.linearize_dense_window(*wins[S], default_opts(w_pose_consist=0.5, **ref), sources=sources)
                scal = np.array([r[k] for k in ("loss", "fwd", "inv_photo", "inv_dc", "K_f", "K_i", "a_f", "pose_consist")])
                show(f"reference loss S={S} export sources={int(sources)}", scalars=scal, g_pose=r["g_pose"], g_rho=r["g_rho"], **({"g_rho_src": r["g_rho_src"]} if sources else {}))
            refine(f"reference loss S={S} plain argmin=1 after the export", S, default_opts(argmin=1, **ref))
        # a merged pair of calls: two one-target windows of one shape queued, run as one launch sequence
        for name, S, o in (("pair form", 1, default_opts(**BASE)), ("reference loss", 2, default_opts(**ref))):
            tgt, srcs, dt, ds, K, pose = wins[S]
            calls = []
            for b in range(B):
                idx = [s * B + b for s in range(S)] + [S * B + s * B + b for s in range(S)]
                calls.append((tgt[b:b + 1].contiguous(), srcs[:, b:b + 1].contiguous(), dt[b:b + 1].contiguous(), ds[:, b:b + 1].contiguous(), K[b:b + 1].contiguous(),
                              pose[idx].contiguous(), torch.empty(2 * S, 6, device="cuda"), torch.empty(2 * S, 1, H, W, device="cuda")))
            eng.set_coalesce(B)
            for c in calls:
                eng.refine_dense_window_queued(*c, o)
            eng.flush(); torch.cuda.synchronize()
            eng.set_coalesce(0)
            batches, ncalls = eng.coalesce_counts()
            for b, c in enumerate(calls):
                show(f"merged {name} S={S} call {b}", pose=c[6], depth=c[7])
            print(f"{H}x{W} merged {name} S={S} sequences/calls so far {batches}/{ncalls}")
        # one call under graph replay: the same tensors three times
        eng.use_own_stream()          # (a capture needs a stream of its own, not the default stream)
        eng.set_graph_replay(4)
        for name, S, o in (("joint mode S=2", 2, default_opts(dense_joint=1, argmin=1, **BASE)), ("reference loss S=2", 2, default_opts(**ref))):
            po, do = torch.empty(2 * S * B, 6, device="cuda"), torch.empty(2 * S * B, 1, H, W, device="cuda")
            for sighting in range(3):
                eng.refine_dense_window_async(0, *wins[S], po, do, o)
                eng.synchronize(); torch.cuda.synchronize()
                show(f"graph replay {name} sighting {sighting}", pose=po, depth=do)
        print(f"{H}x{W} graph replay captures/replays {'/'.join(map(str, eng.graph_replay_counts()))}")
        eng.set_graph_replay(0)
        eng.close()


if __name__ == "__main__":
    main()
