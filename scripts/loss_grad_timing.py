"""The loss-side backward passes at 192x640, N = 4: tcsfm_disp_to_depth_backward (both cotangents), tcsfm_ssim_backward (one plane per
item, both outputs), tcsfm_smooth_loss_device and tcsfm_smooth_loss_backward, each against PyTorch-ROCm autograd through the reference
expression in float32 on the same GPU (the backward alone with the graph retained; for the smooth loss also the forward), and the plain
Engine.smooth_loss with its host round trip.  Alternating in one process, HIP events on the stream, a warm-up, the median.  One JSON line.
    python scripts/loss_grad_timing.py            # -> stdout (profiles/r10_loss_grad_timing.jsonl)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from oracle import torch_twin as tw
from tightly_coupled_sfm_amd import losses
from tightly_coupled_sfm_amd.engine import Engine

H, W, N = 192, 640, 4
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0


def timed(f, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def torch_smooth(disp, img):          # the torch body of losses.get_smooth_loss (losses.py:43-61)
    mean_disp = disp.mean(2, True).mean(3, True)
    disp = disp / (mean_disp + 1e-7)
    gdx = torch.abs(disp[:, :, :, :-1] - disp[:, :, :, 1:]); gdy = torch.abs(disp[:, :, :-1, :] - disp[:, :, 1:, :])
    gix = torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1, keepdim=True)
    giy = torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1, keepdim=True)
    return (gdx * torch.exp(-gix)).mean() + (gdy * torch.exp(-giy)).mean()


def main():
    rng = np.random.default_rng(3)
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
    disp, img = cu(rng.uniform(0.05, 0.95, (N, 1, H, W))), cu(rng.uniform(0, 1, (N, 3, H, W)))
    y = cu(np.clip(disp.cpu().numpy() + rng.uniform(-0.1, 0.1, (N, 1, H, W)), 0.01, 0.99))
    g1, g2, g3 = (cu(rng.standard_normal((N, 1, H, W))) for _ in range(3))
    gl = torch.tensor(1.7, device="cuda")
    e = Engine(H, W, N)
    _, stats = e.smooth_loss_device(disp, img)
    lo, hi = 1 / MAX_DEPTH, 1 / MIN_DEPTH
    leaf, xl, yl, dl = (t.clone().requires_grad_() for t in (disp, disp, y, disp))
    s = lo + (hi - lo) * leaf
    L_d2d = (s * g1).sum() + ((1 / s) * g2).sum()
    L_ssim = (tw.ssim(xl, yl) * g3).sum()
    L_smooth = torch_smooth(dl, img) * gl
    fs = {
        "hip_disp_to_depth_backward": lambda: e.disp_to_depth_backward(disp, MIN_DEPTH, MAX_DEPTH, g1, g2),
        "torch_disp_to_depth_backward": lambda: torch.autograd.grad(L_d2d, [leaf], retain_graph=True),
        "hip_ssim_backward": lambda: e.ssim_loss_backward(disp, y, g3),
        "torch_ssim_backward": lambda: torch.autograd.grad(L_ssim, [xl, yl], retain_graph=True),
        "hip_smooth_loss_device": lambda: e.smooth_loss_device(disp, img),
        "hip_smooth_loss_plain_host_round_trip": lambda: e.smooth_loss(disp, img),
        "torch_smooth_forward": lambda: torch_smooth(disp, img),
        "hip_smooth_loss_backward": lambda: e.smooth_loss_backward(disp, img, stats, gl),
        "torch_smooth_backward": lambda: torch.autograd.grad(L_smooth, [dl], retain_graph=True),
    }
    for f in fs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fs}
    for rep in range(10):                 # alternating blocks of 20 calls
        for k, f in fs.items():
            t[k] += timed(f, 20)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    ratio = lambda a, b: round(med[a] / med[b], 2)
    print(json.dumps({"size": f"{W}x{H}", "items": N, "method": "hip events per call, 10 alternating blocks of 20, median",
                      "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(min(v), 4) for k, v in t.items()},
                      "torch_over_hip": {"disp_to_depth_backward": ratio("torch_disp_to_depth_backward", "hip_disp_to_depth_backward"),
                                         "ssim_backward": ratio("torch_ssim_backward", "hip_ssim_backward"),
                                         "smooth_forward": ratio("torch_smooth_forward", "hip_smooth_loss_device"),
                                         "smooth_backward": ratio("torch_smooth_backward", "hip_smooth_loss_backward"),
                                         "smooth_plain_over_device": ratio("hip_smooth_loss_plain_host_round_trip", "hip_smooth_loss_device")}}), flush=True)


if __name__ == "__main__":
    main()
