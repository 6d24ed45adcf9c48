"""The disparity stage of the sequence calls (tcsfm_sequence_disparity) against the same call without it and against what a user did
before it existed (PCIe-inclusive, 200 pinned frames of 640x192, 2 lanes, 8 windows per call): frames-only tcsfm_odometry_sequence,
S = 1, the depth network attached.  Arms:

    stage off          the call as it was
    plain              disparity="plain": one more store in the depth stage's head
    post               disparity="post": a second, mirrored pass of the network and the blend per group of frames, on the pack stream
    off + host loop    the stage-off call followed by helpers.get_disp_for_eigen(DepthNetHIP, ...) over the frames in calls of 8, results
                       back on the host: today's way to the same planes (runs on any build: it needs no new symbol)

The arms alternate after a warm-up of each, every timed call follows an untimed call of its own arm, and a row carries the median, the
extremes and the quartiles of the wall time per sequence.  --runs 2 repeats the whole measurement in the same process.  The stage's arms
are checked to return the poses of the stage-off arm, bit for bit, first.  --package-root runs the arms that build has (the parent
commit's: stage off, off + host loop); --out appends the rows to a .jsonl file.
Also, on a build with the stage: the fetch of the T float64 planes (tcsfm_sequence_disparities), and tcsfm_depthnet_disp_for_eigen on 8
device-resident frames against helpers.get_disp_for_eigen on the same 8 (the latter returns host arrays, the former a device tensor: a
third arm adds the copy to the host)."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--op-reps", type=int, default=50)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, args.package_root)
import numpy as np, torch
import standins, depthnet_twin
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process: HIP_FORCE_DEV_KERNARG / GPU_MAX_HW_QUEUES when absent)
from tightly_coupled_sfm_amd import _lib, helpers, synth
from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
from tightly_coupled_sfm_amd.engine import Engine, default_opts
from tightly_coupled_sfm_amd.posenet import PoseNetHIP
H, W, T, WPC, S = 192, 640, args.frames, 8, 1
seq = synth.make_sequence(T, H, W, seed=5)
frames = torch.as_tensor(np.ascontiguousarray(seq["frames"], dtype=np.float32)).pin_memory()
K = seq["K"]
has_stage = "tcsfm_sequence_disparity" in _lib.EXPORTS
o = default_opts(n_iters=4)
config = {"min_depth": float(o.min_depth), "max_depth": float(o.max_depth)}


def stats(ts, unit=1e3, name="ms"):
    p = np.percentile(ts, [0, 25, 50, 75, 100])
    return {f"median_{name}": round(p[2] * unit, 3), f"min_{name}": round(p[0] * unit, 3), f"q1_{name}": round(p[1] * unit, 3),
            f"q3_{name}": round(p[3] * unit, 3), f"max_{name}": round(p[4] * unit, 3), "reps": len(ts)}


e = Engine(H, W, 2 * S * WPC, lanes=2)
dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
e.attach_depthnet(dn)
run = lambda **kw: pn.odometry_sequence(frames, None, K, o, sources=S, iterations=4, windows_per_call=WPC, **kw)[1]


def host_loop():
    """what a user of the parent build does for the planes: the frames-only call, then get_disp_for_eigen over the frames, 8 per call"""
    poses = run()
    disps = [helpers.get_disp_for_eigen(dn, frames[i:i + 8].cuda(non_blocking=True), config) for i in range(0, T, 8)]
    return poses, np.concatenate(disps)


arms = [("stage off", lambda: run())]
if has_stage:
    arms += [("plain", lambda: run(disparity="plain")), ("post", lambda: run(disparity="post"))]
arms.append(("off + host loop", host_loop))
for _, f in arms:                             # warm-up: allocations, the rings, the lanes' PoseNet clones
    f(); f()
if has_stage:
    a = run()
    for mode in ("plain", "post"):
        assert torch.equal(a.view(torch.int32), run(disparity=mode).view(torch.int32)), "the stage changed the poses"
    planes = e.sequence_disparities()
    mirror = host_loop()[1]
    print(json.dumps({"note": "post planes against the host loop (optimizer.batch_post_process_disparity keeps its own ramp form)",
                      "max_abs_diff": float(np.abs(planes - mirror.reshape(planes.shape)).max())}), flush=True)
rows = []
for r in range(args.runs):
    ts = {name: [] for name, _ in arms}
    for _ in range(args.reps):
        for name, f in arms:
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); ts[name].append(time.perf_counter() - t0)
    for name, _ in arms:
        row = dict({"build": args.label, "leg": "odometry S=1, frames only (depth network attached)", "arm": name, "run": r, "T": T, "H": H, "W": W,
                    "windows_per_call": WPC, "lanes": 2}, **stats(ts[name]))
        row["windows_per_s"] = round((T - S) / (row["median_ms"] * 1e-3), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)

if has_stage:
    run(disparity="post")
    for r in range(args.runs):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); e.sequence_disparities(); ts.append(time.perf_counter() - t0)
        row = dict({"build": args.label, "leg": f"fetch of {T} float64 planes (tcsfm_sequence_disparities, pageable destination)", "arm": "fetch", "run": r,
                    "T": T, "H": H, "W": W, "MB": round(T * H * W * 8 / 1e6, 1)}, **stats(ts))
        rows.append(row)
        print(json.dumps(row), flush=True)
    f8 = frames[:8].cuda()
    ops = [("tcsfm_depthnet_disp_for_eigen (device tensor out)", lambda: dn.disp_for_eigen(f8, o.min_depth, o.max_depth)),
           ("tcsfm_depthnet_disp_for_eigen + copy to the host", lambda: dn.disp_for_eigen(f8, o.min_depth, o.max_depth).cpu()),
           ("helpers.get_disp_for_eigen (host arrays out)", lambda: helpers.get_disp_for_eigen(dn, f8, config))]
    for r in range(args.runs):
        ts = {name: [] for name, _ in ops}
        for _ in range(args.op_reps):
            for name, f in ops:
                f(); e.synchronize()
                t0 = time.perf_counter(); f(); e.synchronize(); ts[name].append(time.perf_counter() - t0)
        for name, v in ts.items():
            row = dict({"build": args.label, "leg": "operator, 8 frames", "arm": name, "run": r, "N": 8, "H": H, "W": W}, **stats(v, 1e6, "us"))
            rows.append(row)
            print(json.dumps(row), flush=True)
for n in (pn, dn):
    n.close()
e.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
