"""Depth-network timings at 640x192: the library's gfx950 kernels (DepthNetHIP.forward) vs the same network in PyTorch
(tests/depthnet_twin.DepthNetTwin: MIOpen convolutions) on the same GPU, alternating in one process, for N = 1, 2, 5 and 18 images
(18 = a minibatch of 6 three-frame windows).  TF/s and the fraction of the 157.3 TF fp32 matrix peak are on the DIRECT FLOP count
(2 x multiply-adds of every convolution, 25.9 GFLOP per image).  One JSON line per N.
    python scripts/depthnet_timing.py                 # -> stdout (profiles/r06_depthnet_timing.jsonl)
    python scripts/depthnet_timing.py --profile-only  # a few N = 5 forwards and nothing else (for rocprofv3 --kernel-trace --stats)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import depthnet_twin as dt
from tightly_coupled_sfm_amd.engine import Engine
from tightly_coupled_sfm_amd.depthnet import DepthNetHIP

H, W = 192, 640
PEAK_TF = 157.3


def direct_flop(H, W):
    """2 x multiply-adds of every convolution of the network for one H x W image"""
    f = 2 * 64 * 3 * 49 * (H // 2) * (W // 2)
    for p, ci, co, s, ds in dt._blocks():
        scale = {64: 4, 128: 8, 256: 16, 512: 32}[co]
        hw = (H // scale) * (W // scale)
        f += 2 * hw * co * 9 * (ci + co) + (2 * hw * co * ci if ds else 0)
    for i in range(5):
        hw = (H >> (4 - i)) * (W >> (4 - i))
        f += 2 * hw * 9 * dt.PLANES[i + 1] * (dt.PLANES[i] + dt.PLANES[i + 1])
    return f + 2 * H * W * 9 * (32 * 8 + 8 * 1)


def main():
    sd = dt.depthnet_params(0)
    e = Engine(H, W, 2)
    net = DepthNetHIP(e, 18, sd)
    if "--profile-only" in sys.argv:
        x = torch.from_numpy(dt.sample_images(1, 5, H, W)).cuda()
        for _ in range(10):
            net.forward(x)
        torch.cuda.synchronize()
        return
    twin = dt.DepthNetTwin(sd, device="cuda")
    gf = direct_flop(H, W) / 1e9
    for N in (1, 2, 5, 18):
        x = torch.from_numpy(dt.sample_images(N, N, H, W)).cuda()
        fh = lambda: net.forward(x)
        def ft():
            with torch.no_grad():
                return twin(x=x)
        for _ in range(5):
            fh(); ft()
        th, tt = [], []
        for rep in range(8):          # alternating blocks of 10 calls
            for f, acc in ((fh, th), (ft, tt)) if rep % 2 == 0 else ((ft, tt), (fh, th)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(10):
                    f()
                torch.cuda.synchronize(); acc.append((time.perf_counter() - t0) / 10 * 1e3)
        mh, mt = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
        tf = lambda ms: gf * N / ms                  # GFLOP per ms = TFLOP/s
        print(json.dumps({"images": N, "size": f"{W}x{H}", "GFLOP_direct_per_image": round(gf, 2),
                          "forward_ms_median": {"hip": round(mh, 4), "torch_miopen": round(mt, 4)},
                          "forward_ms_min": {"hip": round(min(th), 4), "torch_miopen": round(min(tt), 4)},
                          "speedup_vs_torch": round(mt / mh, 2),
                          "TFLOPs": {"hip": round(tf(mh), 1), "torch_miopen": round(tf(mt), 1)},
                          "fraction_of_fp32_matrix_peak": {"hip": round(tf(mh) / PEAK_TF, 3), "torch_miopen": round(tf(mt) / PEAK_TF, 3)}}), flush=True)


if __name__ == "__main__":
    main()
