"""One backward pass of compute_photometric_error at 192x640, N = 4 (the directed pairs of a KITTI window): tcsfm_photometric_backward
(all three cotangents, all three outputs; Engine.compute_photometric_error_backward: warp forward into scratch, the assembly's backward,
the warp's backward) against PyTorch-ROCm autograd through the fp32 twin (oracle.torch_twin.photometric: forward + backward, and the
backward alone with the graph retained), alternating in one process.  HIP events on the stream, a warm-up, the median.  One JSON line.
    python scripts/photo_grad_timing.py            # -> stdout (profiles/r09_photo_grad_timing.jsonl)
    python scripts/photo_grad_timing.py --profile-only   # 20 HIP backward calls and nothing else (rocprofv3 --kernel-trace --stats)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import operator_inputs as OI
from oracle import torch_twin as tw
from tightly_coupled_sfm_amd.engine import Engine

H, W, N = 192, 640, 4


def timed(f, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    c = OI.make_case(H, W, N, 1.0)
    d = {k: torch.as_tensor(v).cuda() for k, v in c.items()}
    gen = torch.Generator().manual_seed(5)
    g_diff, g_weight, g_rec = (torch.randn(s, generator=gen).cuda() for s in ((N, 1, H, W), (N, 1, H, W), (N, 3, H, W)))
    e = Engine(H, W, N)
    hip = lambda: e.compute_photometric_error_backward(d["tgt"], d["src"], d["depth_t"], d["depth_s"], d["pose"], d["K"], g_diff, g_weight, g_rec)
    if "--profile-only" in sys.argv:
        for _ in range(20):
            hip()
        torch.cuda.synchronize()
        return
    leaves = [d[k].clone().requires_grad_() for k in ("depth_t", "depth_s", "pose")]

    def loss():
        r = tw.photometric(d["tgt"], d["src"], leaves[0], leaves[1], leaves[2], d["K"])
        return (r["diff"] * g_diff).sum() + (r["weight"] * g_weight).sum() + (r["rec"] * g_rec).sum()

    twin_fb = lambda: torch.autograd.grad(loss(), leaves)
    L = loss()
    twin_b = lambda: torch.autograd.grad(L, leaves, retain_graph=True)
    fs = {"hip_backward": hip, "torch_fp32_twin_forward_backward": twin_fb, "torch_fp32_twin_backward_only": twin_b}
    for f in fs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fs}
    for rep in range(10):                 # alternating blocks of 20 calls
        for k, f in fs.items():
            t[k] += timed(f, 20)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    print(json.dumps({"size": f"{W}x{H}", "items": N, "method": "hip events per call, 10 alternating blocks of 20, median",
                      "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(min(v), 4) for k, v in t.items()},
                      "speedup_vs_twin_backward_only": round(med["torch_fp32_twin_backward_only"] / med["hip_backward"], 2)}), flush=True)


if __name__ == "__main__":
    main()
