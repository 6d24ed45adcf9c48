"""Frames in, poses out: tcsfm_odometry_sequence with the depth network inside the call against the two-step path
(PCIe-inclusive, 200 pinned frames of 640x192, 4 PoseNet iterations, 2 lanes, 8 windows per call), S = 1 and S = 2.

    arm A  two-step: the depth network over all frames in calls of 8 (frames uploaded for it), tcsfm_disp_to_depth, the depths
           copied to pinned host memory, then the sequence call with host depths
    arm B  frames-only: Engine.attach_depthnet + depths=None (skipped where the library has no tcsfm_sequence_depthnet)
    arm C  the depth network alone over the 200 frames, resident on the device (B's floor)

The arms alternate (A, B, C, A, B, C, ...) after a warm-up of each, so drift hits them alike; a row carries the median, the extremes
and the quartiles of the wall time per sequence.  --package-root runs the same arms on another build of the package (the parent
commit's, for the acceptance comparison); --out appends the rows to a .jsonl file."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, args.package_root)
import numpy as np, torch
import standins, depthnet_twin
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process: HIP_FORCE_DEV_KERNARG / GPU_MAX_HW_QUEUES when absent)
from tightly_coupled_sfm_amd import _lib, synth
from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
from tightly_coupled_sfm_amd.engine import Engine, default_opts
from tightly_coupled_sfm_amd.posenet import PoseNetHIP
H, W, T, WPC, GROUP = 192, 640, args.frames, 8, 8
seq = synth.make_sequence(T, H, W, seed=5)
frames = torch.as_tensor(seq["frames"]).pin_memory()
depths = torch.empty((T, 1, H, W), dtype=torch.float32).pin_memory()
K = seq["K"]
has_b = "tcsfm_sequence_depthnet" in _lib.EXPORTS


def stats(ts):
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return {"median_ms": round(q[2] * 1e3, 3), "min_ms": round(q[0] * 1e3, 3), "q1_ms": round(q[1] * 1e3, 3), "q3_ms": round(q[3] * 1e3, 3),
            "max_ms": round(q[4] * 1e3, 3), "frames_per_s": round(T / q[2], 1), "reps": len(ts)}


rows = []
for S, o in ((1, default_opts(n_iters=4)), (2, default_opts(n_iters=4, argmin=1, w_dc=0.15))):
    e = Engine(H, W, 2 * S * WPC, lanes=2)
    dn = DepthNetHIP(e, GROUP, depthnet_twin.depthnet_params(0))
    pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
    kw = dict(sources=S, iterations=4, windows_per_call=WPC, target_pos=-1 if S == 2 else 0)
    dev_frames = frames.cuda()

    def net_over(src):
        for i0 in range(0, T, GROUP):
            yield i0, e.disp_to_depth(dn.forward(src[i0:i0 + GROUP].cuda(non_blocking=True)), o.min_depth, o.max_depth)[1]

    def arm_a():
        for i0, d in net_over(frames):
            depths[i0:i0 + GROUP].copy_(d, non_blocking=True)
        torch.cuda.synchronize()
        return pn.odometry_sequence(frames, depths, K, o, **kw)

    def arm_b():
        return pn.odometry_sequence(frames, None, K, o, **kw)

    def arm_c():
        for _ in net_over(dev_frames):
            pass
        torch.cuda.synchronize()

    arms = [("A two-step (host depths)", arm_a), ("C depth network alone", arm_c)]
    if has_b:
        e.attach_depthnet(dn)
        arms.insert(1, ("B frames-only", arm_b))
    for _, f in arms:                         # warm-up: allocations, the ring, the lanes' PoseNet clones
        f(); f()
    if has_b:
        a, b = arm_a(), arm_b()
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "frames-only and two-step poses differ"
    ts = {name: [] for name, _ in arms}
    for _ in range(args.reps):
        for name, f in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); ts[name].append(time.perf_counter() - t0)
    for name, _ in arms:
        row = dict({"build": args.label, "S": S, "arm": name, "T": T, "H": H, "W": W, "windows_per_call": WPC, "lanes": 2, "posenet_iterations": 4}, **stats(ts[name]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    del dev_frames
    pn.close(); dn.close(); e.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
