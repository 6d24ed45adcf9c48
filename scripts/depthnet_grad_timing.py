"""Weight-tuning step timings of the depth network at 640x192: one training forward + backward on the library's kernels
(depthnet_train.DepthNetModule) against the same step in PyTorch autograd on MIOpen (tests/depthnet_twin.forward, fp32), alternating
in one process with device synchronisation, for N = 6 and 18 images (18 = the driver's minibatch of 6 three-frame windows), in three
modes: `encoder` (encoder weights require grad, decoder frozen), `all` (every weight), `bottleneck` (weights frozen, skips 3 and 4 are
leaves: a decoder forward + backward from fixed skips).  Loss (disp * R).sum() with a seeded R.  One JSON line per (mode, N).
    python scripts/depthnet_grad_timing.py                  # -> stdout (profiles/r07_depthnet_grad_timing.jsonl)
    python scripts/depthnet_grad_timing.py --profile-only   # 5 `all` steps at N = 6 and nothing else (rocprofv3 --kernel-trace --stats)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import depthnet_twin as dt
from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule

H, W = 192, 640
MODES = ("encoder", "all", "bottleneck")


def _stat(k):
    return k.endswith(("running_mean", "running_var"))


def hip_step(mod, mode, x, R, sk):
    def f():
        mod.zero_grad(set_to_none=True)
        if mode == "bottleneck":
            leaves = [s if k < 3 else s.detach().requires_grad_(True) for k, s in enumerate(sk)]
            disp = mod(None, skips=leaves)[0][0]
        else:
            disp = mod(x)[0][0]
        (disp * R).sum().backward()
    return f


def twin_step(sd, mode, x, R, sk):
    for k, v in sd.items():
        if not _stat(k):
            v.requires_grad_(mode == "all" or (mode == "encoder" and k.startswith(dt.ENC)))

    def f():
        for v in sd.values():
            v.grad = None
        if mode == "bottleneck":
            leaves = [s if k < 3 else s.detach().requires_grad_(True) for k, s in enumerate(sk)]
            disp = dt._decode(sd, leaves)
        else:
            disp = dt.forward(sd, x)
        (disp * R).sum().backward()
    return f


def setup(mode, N):
    params = dt.depthnet_params(0)
    mod = DepthNetModule(params, max_images=18).cuda()
    for k, p in mod.named_parameters():
        p.requires_grad_(mode == "all" or (mode == "encoder" and k.startswith(dt.ENC)))
    sd = {k: v.cuda() for k, v in params.items()}
    x = torch.from_numpy(dt.sample_images(N, N, H, W)).cuda()
    R = torch.randn((N, 1, H, W), generator=torch.Generator().manual_seed(N)).cuda()
    with torch.no_grad():
        _, sk = mod(x, return_disp=False)
        _, skt = dt.forward(sd, x, return_skips=True)
    return mod, sd, x, R, sk, skt


def main():
    if "--profile-only" in sys.argv:
        mod, sd, x, R, sk, _ = setup("all", 6)
        f = hip_step(mod, "all", x, R, sk)
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        return
    for N in (6, 18):
        for mode in MODES:
            mod, sd, x, R, sk, skt = setup(mode, N)
            fh, ft = hip_step(mod, mode, x, R, sk), twin_step(sd, mode, x, R, skt)
            for _ in range(3):
                fh(); ft()
            th, tt = [], []
            for rep in range(8):          # alternating blocks of 5 steps
                for f, acc in ((fh, th), (ft, tt)) if rep % 2 == 0 else ((ft, tt), (fh, th)):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    for _ in range(5):
                        f()
                    torch.cuda.synchronize(); acc.append((time.perf_counter() - t0) / 5 * 1e3)
            mh, mt = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
            print(json.dumps({"mode": mode, "images": N, "size": f"{W}x{H}",
                              "step_ms_median": {"hip": round(mh, 3), "torch_miopen_autograd": round(mt, 3)},
                              "step_ms_min": {"hip": round(min(th), 3), "torch_miopen_autograd": round(min(tt), 3)},
                              "speedup_vs_torch": round(mt / mh, 2)}), flush=True)
            del mod, sd, fh, ft
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
