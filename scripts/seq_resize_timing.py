"""Camera-size frames in the sequence calls (tcsfm_sequence_frame_source) against frames resized on the host first (PCIe-inclusive, 200
pinned frames of 1241x376 -> 640x192, 2 lanes, 8 windows per call).  Three legs:

    refine S=1      tcsfm_refine_sequence, one source, depths given        (the PCIe-bound leg)
    refine S=2      tcsfm_refine_sequence, KITTI windows, depths given
    odometry        tcsfm_odometry_sequence, S = 1, frames only, the depth network attached

and per leg three arms:

    camera u8       (a) the camera's bytes, interleaved uint8 [T,376,1241,3], with source_size: resized on the device by k_resize_u8
                    (skipped where the library has no tcsfm_sequence_frame_source: the parent build)
    resized u8      (b) the floor: uint8 [T,192,640,3] that somebody resized before, converted on the device
    host resize     what (b) needs before it can start when the camera delivers 1241x376: the reference's per-frame
                    Image.resize((640, 192), Image.LANCZOS) of the whole sequence into the pinned buffer (b) reads.  Without Pillow: the
                    same integer arithmetic in torch with the library's coefficient tables (labelled in the row).
    (c) = host resize + (b) is what a user of the parent build runs; the script prints (a) / (c).

The arms alternate after a warm-up of each, so drift hits them alike; a row carries the median, the extremes and the quartiles of the
wall time per sequence.  Every timed sequence call follows an untimed call of its own arm (--lead 1, the default; see
scripts/seq_u8_timing.py).  (a) and (b) are checked to return the same bits first.
The camera frames are the synthetic 640x192 sequence enlarged bilinearly to 1241x376 (rendering 200 frames at that size takes minutes
on the host and the timings do not depend on the content); the 640x192 frames (b) reads are the host resize of those.
--profile-only: the kernel alone on one chunk, for rocprofv3 --kernel-trace --stats (profiles/README.md names the command).
--package-root runs the arms on another build of the package (the parent commit's); --out appends the rows to a .jsonl file."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--lead", type=int, default=1, help="1: an untimed call of the same arm right before every timed sequence call; 0: none")
ap.add_argument("--out", default="")
ap.add_argument("--profile-only", action="store_true",
                help="20 launches of k_resize_u8 on one chunk (4 interleaved frames -> the float ring's planar floats) and nothing else: the "
                     "workload of rocprofv3 --kernel-trace --stats")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, args.package_root)
import numpy as np, torch
import standins, depthnet_twin, resize_inputs
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process)
from tightly_coupled_sfm_amd import _lib, synth
from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
from tightly_coupled_sfm_amd.engine import Engine, default_opts
from tightly_coupled_sfm_amd.posenet import PoseNetHIP
try:
    from PIL import Image
except ImportError:
    Image = None
H, W, h, w, T, WPC = 192, 640, 376, 1241, args.frames, 8
if args.profile_only:
    e = Engine(H, W, 2)
    chunk = torch.randint(0, 256, (4, h, w, 3), dtype=torch.uint8, device="cuda")
    for _ in range(20):
        out = e.resize_u8(chunk, "hwc", out="f32")
    torch.cuda.synchronize()
    print("k_resize_u8: 20 launches, 4 frames of %dx%d -> %dx%d; bytes per launch: %d read + %d written" % (w, h, W, H, chunk.numel(), out.numel() * 4))
    sys.exit(0)
seq = synth.make_sequence(T, H, W, seed=5)
big = torch.nn.functional.interpolate(torch.as_tensor(np.asarray(seq["frames"], dtype=np.float32)), size=(h, w), mode="bilinear", align_corners=False)
cam = (big * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()       # [T,h,w,3]: the camera's bytes
del big
small = torch.empty((T, H, W, 3), dtype=torch.uint8).pin_memory()                                          # what (b) reads
depths = torch.as_tensor(seq["depths"]).pin_memory()
K = seq["K"]
has_source = "tcsfm_sequence_frame_source" in _lib.EXPORTS


def _torch_pass(img, axis, out):
    """one pass of resize_inputs' restatement on an int32 tensor [h, w, 3], along axis 0 or 1"""
    _, bounds, kk = resize_inputs.coeffs(img.shape[axis], out)
    idx = torch.as_tensor(bounds[:, :1].astype(np.int64) + np.minimum(np.arange(kk.shape[1])[None, :], bounds[:, 1:] - 1))      # [out, ksize] (taps beyond n: weight 0)
    k = torch.as_tensor(kk)
    g = img.movedim(axis, 0)[idx]                                                                          # [out, ksize, other, 3]
    acc = (g * k[:, :, None, None]).sum(1) + (1 << 21)
    return (acc >> 22).clamp(0, 255).movedim(0, axis)


def host_resize():
    """the reference's loader over the sequence: one Lanczos resize per frame into the pinned buffer the resized arm reads"""
    dst = small.numpy()
    if Image is not None:
        for t in range(T):
            dst[t] = np.asarray(Image.fromarray(cam[t].numpy(), "RGB").resize((W, H), resample=Image.LANCZOS))
    else:
        for t in range(T):
            small[t] = _torch_pass(_torch_pass(cam[t].to(torch.int32), 1, W), 0, H).to(torch.uint8)


HOST = "host resize (Pillow %s)" % Image.__version__ if Image is not None else "host resize (torch, the library's tables; no Pillow here)"
host_resize()
chk, _ = resize_inputs.resize(cam[:1].numpy(), H, W)
assert np.array_equal(chk[0], small[0].numpy()), "the host resize is not the restatement's"
init1 = torch.as_tensor(seq["init"])
step = seq["init"][:, 0]
init2 = torch.as_tensor(np.stack([np.stack([-step[i], step[i + 1], step[i], -step[i + 1]]) for i in range(T - 2)]).astype(np.float32))


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
        run = lambda fr, **kw: e.refine_sequence(fr, depths, K, init, o, sources=S, windows_per_call=WPC, target_pos=-1 if S == 2 else 0, **kw)
    else:
        dn = DepthNetHIP(e, 8, depthnet_twin.depthnet_params(0))
        pn = PoseNetHIP(e, 2 * S * WPC, standins.posenet_params(0))
        e.attach_depthnet(dn)
        nets = [pn, dn]
        run = lambda fr, **kw: pn.odometry_sequence(fr, None, K, o, sources=S, iterations=4, windows_per_call=WPC, **kw)[1]
    arms = [("resized u8", lambda: run(small)), (HOST, host_resize)]
    if has_source:
        arms.insert(0, ("camera u8", lambda: run(cam, source_size=(h, w))))
    for _, f in arms:                         # warm-up: allocations, the rings, the lanes' PoseNet clones
        f(); f()
    if has_source:
        a, b = run(cam, source_size=(h, w)), run(small)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "camera-size frames and host-resized frames give different poses"
    ts = {name: [] for name, _ in arms}
    for _ in range(args.reps):
        for name, f in arms:
            if args.lead and name != HOST:
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); ts[name].append(time.perf_counter() - t0)
    med = {}
    for name, _ in arms:
        row = dict({"build": args.label, "leg": leg, "arm": name, "T": T, "source": [h, w], "H": H, "W": W, "windows_per_call": WPC, "lanes": 2,
                    "lead_call": bool(args.lead)}, **stats(ts[name], T - S))
        if name == HOST:
            row.pop("windows_per_s")
        med[name] = row["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if has_source:
        c = med[HOST] + med["resized u8"]
        row = {"build": args.label, "leg": leg, "arm": "(a) camera u8 / (c) host resize + resized u8", "a_ms": med["camera u8"], "c_ms": round(c, 3),
               "a_over_c": round(med["camera u8"] / c, 4)}
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
