"""The depth evaluation on the device (tcsfm_depth_eval, tcsfm_sequence_depth_eval) against what a user of the parent commit does for
the same numbers: tcsfm_sequence_disparities to the host, then the NumPy evaluation per frame (tests/depth_eval_inputs.py's twin: the
reference's script with its cv2.resize restated in NumPy).

  operator   192 x 640 float64 planes against 375 x 1242 ground truth, N = 8 and 64 frames per call, ground truth sparse (about 5 % of
             the plane survives the Eigen crop and range test, KITTI's density) and dense (every pixel valid); HIP events around blocks of
             --block calls, per call and per frame, median / quartiles / extremes over --reps blocks after a warm-up block.  lds_pairs = 0
             (no list: every pass scans the crop) beside the default shows what the list is worth.
  sequence   a frames-only tcsfm_odometry_sequence over --frames frames with disparity="post" leaves the store; then, alternating after a
             warm-up of each: (a) Engine.sequence_depth_eval over the whole store, the upload of the ground truth (1.86 MB per frame,
             pageable) included; (b) Engine.sequence_disparities to the host and the twin per frame on one core.  Wall time per sequence.
--out appends the rows to a .jsonl file."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--block", type=int, default=10)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--out", default="")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np, torch
import standins, depthnet_twin
import depth_eval_inputs as D
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process: HIP_FORCE_DEV_KERNARG / GPU_MAX_HW_QUEUES when absent)
from tightly_coupled_sfm_amd import synth
from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
from tightly_coupled_sfm_amd.engine import Engine, default_opts
from tightly_coupled_sfm_amd.posenet import PoseNetHIP
H, W, GH, GW, T, WPC, S = 192, 640, 375, 1242, args.frames, 8, 1


def stats(ts, unit, name):
    p = np.percentile(ts, [0, 25, 50, 75, 100])
    return {f"median_{name}": round(p[2] * unit, 3), f"min_{name}": round(p[0] * unit, 3), f"q1_{name}": round(p[1] * unit, 3),
            f"q3_{name}": round(p[3] * unit, 3), f"max_{name}": round(p[4] * unit, 3), "reps": len(ts)}


def ground_truth(n, valid, seed):
    """n float32 planes: uniform in [1, 79) on a fraction `valid` of the pixels, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(1.0, 79.0, size=(n, GH, GW)).astype(np.float32)
    if valid < 1.0:
        g[rng.uniform(size=g.shape) >= valid] = 0
    return g


rows = []
e = Engine(H, W, 2 * S * WPC, lanes=2)
y0, y1, x0, x1 = D.crop(D.EIGEN, GH, GW)
crop_share = (y1 - y0) * (x1 - x0) / (GH * GW)

# ---- the operator
rng = np.random.default_rng(1)
base = {"sparse": ground_truth(8, 0.05 / crop_share, 2), "dense": ground_truth(8, 1.0, 3)}
for n in (8, 64):
    planes = torch.from_numpy(rng.uniform(D.MIN_DISP, D.MAX_DISP, size=(n, H, W))).cuda()
    for density, g8 in base.items():
        gt = torch.from_numpy(np.concatenate([g8] * (n // 8))).cuda()
        for lds_pairs in (-1, 0):
            call = lambda: e.depth_eval(planes, gt, lds_pairs=lds_pairs)
            m = call().cpu().numpy()
            for _ in range(args.block):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.block):
                    call()
                b.record(); b.synchronize()
                ts.append(a.elapsed_time(b) * 1e-3 / args.block)
            row = dict({"leg": "operator", "N": n, "gt": density, "lds_pairs": "default" if lds_pairs < 0 else lds_pairs, "H": H, "W": W, "gt_h": GH,
                        "gt_w": GW, "masked_per_frame": float(m[:, 8].mean()), "block": args.block}, **stats(ts, 1e6, "us_per_call"))
            row["median_us_per_frame"] = round(row["median_us_per_call"] / n, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)

# ---- the sequence form
dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
e.attach_depthnet(dn)
seq = synth.make_sequence(T, H, W, seed=5)
frames = torch.as_tensor(np.ascontiguousarray(seq["frames"], dtype=np.float32)).pin_memory()
pn.odometry_sequence(frames, None, seq["K"], default_opts(n_iters=4), sources=S, iterations=4, windows_per_call=WPC, disparity="post")
gts = np.concatenate([base["sparse"]] * ((T + 7) // 8))[:T]


def device_arm():
    return e.sequence_depth_eval(gts)


def host_arm():
    planes = e.sequence_disparities()
    return np.stack([D.evaluate_frame(planes[t], gts[t]) for t in range(T)])


got, want = device_arm(), host_arm()
exact = all(np.array_equal(got[:, j], want[:, j]) for j in D.EXACT)
rel = float(np.max(np.abs(got[:, :4] - want[:, :4]) / np.abs(want[:, :4])))
print(json.dumps({"note": "device against the host loop", "exact_fields_equal": bool(exact), "max_rel_diff_summed": rel}), flush=True)
device_arm()
ts = {"device": [], "host": []}
for r in range(max(args.reps, args.host_reps)):
    if r < args.reps:
        t0 = time.perf_counter(); device_arm(); ts["device"].append(time.perf_counter() - t0)
    if r < args.host_reps:
        t0 = time.perf_counter(); host_arm(); ts["host"].append(time.perf_counter() - t0)
for arm, what in (("device", "Engine.sequence_depth_eval, ground-truth upload included"),
                  ("host", "Engine.sequence_disparities + the NumPy evaluation per frame (the parent commit's way)")):
    row = dict({"leg": "sequence", "arm": what, "T": T, "H": H, "W": W, "gt_h": GH, "gt_w": GW, "gt_MB": round(gts.nbytes / 1e6, 1),
                "planes_MB": round(T * H * W * 8 / 1e6, 1)}, **stats(ts[arm], 1e3, "ms"))
    row["median_ms_per_frame"] = round(row["median_ms"] / T, 4)
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
