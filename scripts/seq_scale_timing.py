"""The per-frame scale stage of the sequence calls (tcsfm_sequence_scale) against the same calls without it (PCIe-inclusive, 200
pinned frames of 640x192, 2 lanes, 8 windows per call).  Three legs:

    refine S=1      tcsfm_refine_sequence, one source, depths given        (the PCIe-bound leg)
    refine S=2      tcsfm_refine_sequence, KITTI windows, depths given
    odometry        tcsfm_odometry_sequence, S = 1, frames only, the depth network attached

and per leg two arms:

    stage off       the call as it was
    stage on        cam_height=1.65 / 30: k_ground + k_median_frames per chunk on the pack stream, one copy of the results at the end
                    (skipped where the library has no tcsfm_sequence_scale: the parent build)

The arms alternate after a warm-up of each, every timed call follows an untimed call of its own arm, and a row carries the median, the
extremes and the quartiles of the wall time per sequence.  --runs 2 repeats the whole measurement in the same process: the two medians
of an arm are its run-to-run spread.  The stage-on arm is checked to return the poses of the stage-off arm, bit for bit, first.
--package-root runs the stage-off arm on another build of the package (the parent commit's: the baseline); --out appends the rows
to a .jsonl file.
--operator adds the operator's own timing at 192x640 for N = 4 and 8: tcsfm_scale_recovery_frames (two launches) against N calls of
tcsfm_scale_recovery on the same depths (nine launches and a memset each), both on the engine's stream, wall time per batch with a
synchronisation at the end, median of --op-reps."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--operator", action="store_true")
ap.add_argument("--op-reps", type=int, default=200)
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
H, W, T, WPC = 192, 640, args.frames, 8
CAM = 1.65 / 30.0
seq = synth.make_sequence(T, H, W, seed=5)
frames = torch.as_tensor(np.ascontiguousarray(seq["frames"], dtype=np.float32)).pin_memory()
depths = torch.as_tensor(seq["depths"]).pin_memory()
K = seq["K"]
has_scale = "tcsfm_sequence_scale" in _lib.EXPORTS
init1 = torch.as_tensor(seq["init"])
step = seq["init"][:, 0]
init2 = torch.as_tensor(np.stack([np.stack([-step[w], step[w + 1], step[w], -step[w + 1]]) for w in range(T - 2)]).astype(np.float32))


def stats(ts, nwin):
    p = np.percentile(ts, [0, 25, 50, 75, 100])
    return {"median_ms": round(p[2] * 1e3, 3), "min_ms": round(p[0] * 1e3, 3), "q1_ms": round(p[1] * 1e3, 3), "q3_ms": round(p[3] * 1e3, 3),
            "max_ms": round(p[4] * 1e3, 3), "windows_per_s": round(nwin / p[2], 1), "reps": len(ts)}


o1, o2 = default_opts(n_iters=4), default_opts(n_iters=4, argmin=1, w_dc=0.15)
LEGS = [("refine S=1, depths given", 1, o1, "refine"), ("refine S=2 (KITTI windows), depths given", 2, o2, "refine"),
        ("odometry S=1, frames only (depth network attached)", 1, o1, "odometry")]
rows = []
for leg, S, o, kind in LEGS:
    e = Engine(H, W, 2 * S * WPC, lanes=2)
    nets = []
    if kind == "refine":
        init = init1 if S == 1 else init2
        run = lambda **kw: e.refine_sequence(frames, depths, K, init, o, sources=S, windows_per_call=WPC, target_pos=-1 if S == 2 else 0, **kw)
    else:
        dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
        pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
        e.attach_depthnet(dn)
        nets = [pn, dn]
        run = lambda **kw: pn.odometry_sequence(frames, None, K, o, sources=S, iterations=4, windows_per_call=WPC, **kw)[1]
    arms = [("stage off", lambda: run())]
    if has_scale:
        arms.append(("stage on", lambda: run(cam_height=CAM)))
    for _, f in arms:                         # warm-up: allocations, the rings, the lanes' PoseNet clones
        f(); f()
    extra = {}
    if has_scale:
        a, b = run(), run(cam_height=CAM)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the stage changed the poses"
        sc = e.sequence_scales()
        extra = {"frames_with_ground": int((sc["count"] > 0).sum()), "median_scale": round(float(sc["scale"].nanmedian()), 6)}
    for r in range(args.runs):
        ts = {name: [] for name, _ in arms}
        for _ in range(args.reps):
            for name, f in arms:
                f()
                torch.cuda.synchronize()
                t0 = time.perf_counter(); f(); ts[name].append(time.perf_counter() - t0)
        for name, _ in arms:
            row = dict({"build": args.label, "leg": leg, "arm": name, "run": r, "T": T, "H": H, "W": W, "windows_per_call": WPC, "lanes": 2},
                       **stats(ts[name], T - S))
            if name == "stage on":
                row.update(extra)
            rows.append(row)
            print(json.dumps(row), flush=True)
    for n in nets:
        n.close()
    e.close()

if args.operator and has_scale:
    for N in (4, 8):
        e = Engine(H, W, N)
        d = depths[:N].cuda()
        Kn = torch.as_tensor(np.repeat(K[None], N, 0).astype(np.float32)).cuda()
        one = lambda: e.scale_recovery_frames(d, Kn, CAM)
        chain = lambda: [e.scale_recovery(d[n:n + 1], Kn[n:n + 1], CAM) for n in range(N)]
        got, want = one()[0], torch.cat(chain())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the operator and the chain disagree"
        for r in range(args.runs):
            ts = {"tcsfm_scale_recovery_frames": [], "N x tcsfm_scale_recovery": []}
            for _ in range(args.op_reps):
                for name, f in (("tcsfm_scale_recovery_frames", one), ("N x tcsfm_scale_recovery", chain)):
                    f(); e.synchronize()
                    t0 = time.perf_counter(); f(); e.synchronize(); ts[name].append(time.perf_counter() - t0)
            for name, v in ts.items():
                p = np.percentile(v, [0, 25, 50, 75, 100])
                row = {"build": args.label, "leg": f"operator N={N}", "arm": name, "run": r, "N": N, "H": H, "W": W, "median_us": round(p[2] * 1e6, 1),
                       "min_us": round(p[0] * 1e6, 1), "q1_us": round(p[1] * 1e6, 1), "q3_us": round(p[3] * 1e6, 1), "max_us": round(p[4] * 1e6, 1),
                       "reps": len(v)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        e.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
