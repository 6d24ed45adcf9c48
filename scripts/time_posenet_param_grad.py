"""PoseNet forward_train + param_backward (all 30 parameter gradients and the input gradient, csrc/posenet_wgrad_kernel.h) at 640x192
against the same step in PyTorch autograd on MIOpen (tests/standins.PoseNetTwin, fp32, its parameters requiring grad), for N = 4 and
N = 24 images (24 = the reference's minibatch of 6 windows with S = 2).  The two alternate in one process in blocks of steps that
end in a device synchronise; medians over the blocks, and each side's spread (min .. max of its blocks).  One JSON line per N.
    python scripts/time_posenet_param_grad.py                  # -> stdout (profiles/r12_posenet_param_grad_timing.jsonl)
    python scripts/time_posenet_param_grad.py --profile-only   # 5 library steps at N = 24 and nothing else (rocprofv3 --kernel-trace --stats)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import posenet_layers as PL
import standins
from tightly_coupled_sfm_amd.engine import Engine
from tightly_coupled_sfm_amd.posenet import PoseNetHIP

H, W = 192, 640
BLOCKS, STEPS = 10, 10


def setup(N):
    sd = standins.posenet_params(0)
    net = PoseNetHIP(Engine(H, W, N), N, sd)
    twin = standins.PoseNetTwin(sd).cuda().eval()
    params = list(twin.parameters())
    x = PL.images(H, W, N, seed=1).cuda()
    d = torch.randn((N, 6), generator=torch.Generator().manual_seed(N)).cuda()

    def hip():
        _, tape = net.forward_train(x)
        return net.param_backward(x, tape, d)

    def torch_step():
        xr = x.detach().requires_grad_(True)
        return torch.autograd.grad(twin(xr), [xr] + params, d)

    return hip, torch_step, [k for k, _ in twin.named_parameters()]


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if "--profile-only" in sys.argv:
        hip, _, _ = setup(24)
        for _ in range(5):
            hip()
        torch.cuda.synchronize()
        return
    for N in (4, 24):
        fh, ft, names = setup(N)
        for _ in range(5):
            (gi, gh), gt = fh(), ft()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-30))
        worst = max((rel(gh[k], g), k) for k, g in zip(names, gt[1:]) if k != "conv1.0.bias")
        th, tt = [], []
        for rep in range(BLOCKS):          # alternating blocks
            for f, acc in ((fh, th), (ft, tt)) if rep % 2 == 0 else ((ft, tt), (fh, th)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(STEPS):
                    f()
                torch.cuda.synchronize(); acc.append((time.perf_counter() - t0) / STEPS * 1e3)
        med = lambda v: sorted(v)[len(v) // 2]
        print(json.dumps({"images": N, "size": f"{W}x{H}", "blocks": BLOCKS, "steps_per_block": STEPS,
                          "step_ms_median": {"hip": round(med(th), 3), "torch_miopen_autograd": round(med(tt), 3)},
                          "step_ms_min_max": {"hip": [round(min(th), 3), round(max(th), 3)], "torch_miopen_autograd": [round(min(tt), 3), round(max(tt), 3)]},
                          "torch_over_hip": round(med(tt) / med(th), 2), "input_gradient_rel_l2_hip_vs_torch": float(f"{rel(gi, gt[0]):.3e}"),
                          "worst_parameter_gradient_rel_l2_hip_vs_torch": [float(f"{worst[0]:.3e}"), worst[1]]}), flush=True)
        del fh, ft
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
