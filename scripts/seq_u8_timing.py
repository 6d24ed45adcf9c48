"""8-bit frames in the sequence calls against float frames (PCIe-inclusive, 200 pinned frames of 640x192, 2 lanes, 8 windows per
call).  Three legs:

    refine S=1      tcsfm_refine_sequence, one source, depths given        (the PCIe-bound leg: 16 B/pixel as floats, 7 as bytes)
    refine S=2      tcsfm_refine_sequence, KITTI windows, depths given
    odometry        tcsfm_odometry_sequence, S = 1, frames only, the depth network attached (12 B/pixel as floats, 3 as bytes)

and per leg three arms:

    u8 hwc          the frames as interleaved uint8 [T,H,W,3], converted on the device (skipped where the library has no
                    tcsfm_sequence_frame_format: the parent build)
    f32             the frames as float32 [T,3,H,W]
    host convert    what the float arm needs before it can start when the camera delivers bytes: the host's own
                    uint8 HWC -> float32 CHW / 255 of the whole sequence into pinned memory (torch, the machine's threads)

The arms alternate (u8, f32, host, u8, f32, host, ...) after a warm-up of each, so drift hits them alike; a row carries the median,
the extremes and the quartiles of the wall time per sequence.  The two frame arms are checked to return the same bits first.
Every timed sequence call follows an untimed call of its own arm (--lead 1, the default): the host conversion leaves the device idle
for some 60 ms, and the first call after such a pause runs slower (about 2 ms on the S = 2 leg), which --lead 0 charges to whichever
arm comes after the conversion in the rotation.
--package-root runs the same arms on another build of the package (the parent commit's, the baseline of the float arms); --out
appends the rows to a .jsonl file."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--lead", type=int, default=1, help="1: an untimed call of the same arm right before every timed sequence call; 0: none")
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
seq = synth.make_sequence(T, H, W, seed=5)
q = np.round(np.asarray(seq["frames"], dtype=np.float64) * 255).astype(np.uint8)
u8 = torch.from_numpy(np.ascontiguousarray(q.transpose(0, 2, 3, 1))).pin_memory()           # [T,H,W,3]: the camera's bytes
f32 = torch.empty((T, 3, H, W), dtype=torch.float32).pin_memory()
depths = torch.as_tensor(seq["depths"]).pin_memory()
K = seq["K"]
has_u8 = "tcsfm_sequence_frame_format" in _lib.EXPORTS


def host_convert():
    """ArrayToTensor over the sequence: transpose to C x H x W, .float() / 255, into the pinned buffer the float arm reads"""
    torch.div(u8.permute(0, 3, 1, 2), 255, out=f32)


host_convert()
assert torch.equal(f32, torch.from_numpy(q).float() / 255)
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
        run = lambda fr: e.refine_sequence(fr, depths, K, init, o, sources=S, windows_per_call=WPC, target_pos=-1 if S == 2 else 0)
    else:
        dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
        pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
        e.attach_depthnet(dn)
        nets = [pn, dn]
        run = lambda fr: pn.odometry_sequence(fr, None, K, o, sources=S, iterations=4, windows_per_call=WPC)[1]
    arms = [("f32", lambda: run(f32)), ("host convert", host_convert)]
    if has_u8:
        arms.insert(0, ("u8 hwc", lambda: run(u8)))
    for _, f in arms:                         # warm-up: allocations, the rings, the lanes' PoseNet clones
        f(); f()
    if has_u8:
        a, b = run(u8), run(f32)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "byte frames and float frames give different poses"
    ts = {name: [] for name, _ in arms}
    for _ in range(args.reps):
        for name, f in arms:
            if args.lead and name != "host convert":
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); ts[name].append(time.perf_counter() - t0)
    for name, _ in arms:
        row = dict({"build": args.label, "leg": leg, "arm": name, "T": T, "H": H, "W": W, "windows_per_call": WPC, "lanes": 2,
                    "lead_call": bool(args.lead)}, **stats(ts[name], T - S))
        if name == "host convert":
            row.pop("windows_per_s")
        rows.append(row)
        print(json.dumps(row), flush=True)
    for n in nets:
        n.close()
    e.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
