"""The window loss (optimizer.py:47-86) at 192x640, (B, S) = (1, 2) and (6, 2), the reference's default switches (diff_img_argmin,
automasking, l_inverse_reconstruction, l_depth_consist 0.15): forward plus backward of losses.compute_optimization_loss as the torch
expression (fused=False) against the fused HIP reduction (fused=True: tcsfm_window_loss, tcsfm_window_loss_backward), with diff_img and
weight_mask of both sides as leaves; and one optimize_depth_encoder epoch of DepthOptimizer(weight_tuning=True) both ways.

Loss: HIP events around blocks of 20 forward + backward calls (the span the stream is busy or waits for the host's launches), 10
alternating blocks per variant after a warm-up, the median per call.  Epoch: the wall time of optimize_window (it ends in a
synchronisation) at 6 and at 2 epochs, alternating fused / unfused, medians of 5; the epoch is (t6 - t2) / 4, which leaves the first pass
and the result assembly out.  Two JSON lines.
    python scripts/window_loss_timing.py [--out profiles/r13_window_loss_timing.jsonl]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from tightly_coupled_sfm_amd import losses

H, W = 192, 640
OPTIONS = dict(num_source_imgs=2, diff_img_argmin=True, automasking=True, l_inverse_reconstruction=True, l_depth_consist=True,
               l_depth_consist_weight=0.15, l_depth_init=False, l_depth_init_weight=0.1, l_smooth=False, l_smooth_weight=2, l_pose_consist=False)


def loss_case(B, S):
    rng = np.random.default_rng(13 + B)
    shape = (S * B, 1, H, W)
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
    leaf = lambda: cu(rng.uniform(0, 1, shape)).requires_grad_()
    fwd = dict(diff_img=leaf(), weight_mask=leaf(), valid_mask=cu(rng.uniform(0, 1, shape) < 0.8), auto_mask_error=cu(rng.uniform(0, 1, shape)))
    inv = dict(diff_img=leaf(), weight_mask=leaf(), valid_mask=cu(rng.uniform(0, 1, shape) < 0.8), auto_mask=cu(rng.uniform(0, 1, shape) < 0.7))
    leaves = [fwd["diff_img"], fwd["weight_mask"], inv["diff_img"], inv["weight_mask"]]
    target = torch.zeros((B, 3, H, W), device="cuda")

    def run(fused):
        L = losses.compute_optimization_loss(OPTIONS, target, None, None, fwd, inv, None, fused=fused)
        return L, torch.autograd.grad(L.sum(), leaves)
    return run


def block_ms(f, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def time_loss():
    out = {}
    for B, S in ((1, 2), (6, 2)):
        run = loss_case(B, S)
        (L0, g0), (L1, g1) = run(False), run(True)
        agree = {"loss_rel": abs(float(L0) - float(L1)) / abs(float(L0)),
                 "grad_rel_l2": max(float((a - b).norm() / a.norm()) for a, b in zip(g0, g1))}
        fs = {"torch": lambda: run(False), "fused": lambda: run(True)}
        for f in fs.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fs}
        for _ in range(10):
            for k, f in fs.items():
                t[k].append(block_ms(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        out[f"B{B}_S{S}"] = {"ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(min(v), 4) for k, v in t.items()},
                             "ms_max": {k: round(max(v), 4) for k, v in t.items()}, "torch_over_fused": round(med["torch"] / med["fused"], 2),
                             "agreement": agree}
    return {"what": "forward + backward of optimizer.py:47-86", "size": f"{W}x{H}", "switches": "argmin, automasking, inverse, l_depth_consist 0.15",
            "method": "hip events around blocks of 20 calls, 10 alternating blocks, median per call", "cases": out}


def time_epoch():
    import depthnet_twin as dt
    import pose_loop_grad_inputs as LI
    import standins
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    from tightly_coupled_sfm_amd.optimizer import DepthOptimizer
    B, S = 1, 2
    im = torch.as_tensor(dt.sample_images(300 + H + W, S + 1, H, W)).float().cuda()
    K = torch.tensor([[[0.58 * W, 0, (W - 1) / 2], [0, 0.58 * W, (H - 1) / 2], [0, 0, 1]]], device="cuda")
    gts = [torch.zeros((B, 6), device="cuda") for _ in range(S)]
    data = (im[:1].contiguous(), [im[1:2].contiguous(), im[2:3].contiguous()], gts, gts, None, K, None, None, None, None, None)
    depth = DepthNetModule(dt.depthnet_params(0), max_images=S + 1).cuda()
    pose = standins.PoseNetTwin(LI.params()).cuda().eval()
    config = {"minibatch": B, "device": "cuda", "min_depth": 0.1, "max_depth": 100.0, "iterations": 2, "camera_height": 1.65}
    base = dict(OPTIONS, l_depth_init=True, lr=2e-4, optimizer="adam", mode="scaled", avg_final_epochs=2, weight_tuning=True, optimize_depth_encoder=True)

    def window(fused, epochs):
        opt = DepthOptimizer(dict(base, epochs=epochs, fused_loss=fused), config, pose, depth, "timing")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = opt.optimize_window(0, data)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r["losses"].tolist()
    for fused in (True, False):
        window(fused, 2)                 # warm-up
    t = {(f, e): [] for f in (True, False) for e in (6, 2)}
    losses_seen = {}
    for _ in range(5):
        for key in t:
            ms, ls = window(*key)
            t[key].append(ms)
            losses_seen[key] = ls
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    epoch = {("fused" if f else "torch"): (med[(f, 6)] - med[(f, 2)]) / 4 for f in (True, False)}
    return {"what": "one optimize_depth_encoder epoch of DepthOptimizer(weight_tuning=True)", "size": f"{W}x{H}", "B": B, "S": S, "iterations": 2,
            "method": "wall time of optimize_window at 6 and 2 epochs, alternating, medians of 5; epoch = (t6 - t2) / 4",
            "ms_window_median": {f"{'fused' if f else 'torch'}_{e}_epochs": round(v, 3) for (f, e), v in med.items()},
            "ms_epoch": {k: round(v, 3) for k, v in epoch.items()}, "saving_us_per_epoch": round((epoch["torch"] - epoch["fused"]) * 1e3, 1),
            "losses_6_epochs": {("fused" if f else "torch"): losses_seen[(f, 6)] for f in (True, False)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_window_loss_timing.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_loss_timing.py needs a GPU: nothing is measured without one")
    lines = [json.dumps(time_loss()), json.dumps(time_epoch())]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
