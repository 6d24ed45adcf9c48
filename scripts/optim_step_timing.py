"""The optimiser step and the per-window weight restore of the weight-tuning loop (csrc/optim_kernel.h, optim.LibraryOptimizer,
DepthOptimizer options['fused_step']), three measurements:

1. one Adam step over the reference depth network's encoder parameters, and over all of its parameters (shapes of
   depthnet_train._shapes()): LibraryOptimizer.step() against torch.optim.Adam with torch's defaults -- the reference's optimiser --
   and the C ABI's tcsfm_optim_step with its tables prebuilt (the launch without Python's per-tensor work).  HIP events around blocks
   of 20 steps, 10 alternating blocks in one process after a warm-up of every variant, the median per step.  The algorithmic bytes
   (28 B per element: read p, g, m, v, write p, m, v) over the C ABI figure, and that as a share of the 8 TB/s HBM peak.
2. one optimize_depth_encoder epoch of DepthOptimizer(weight_tuning=True) at 640x192, B = 1, S = 2 with fused_step on and off: wall
   time of optimize_window at 6 and at 2 epochs, alternating, medians of 5; the epoch is (t6 - t2) / 4 (the method of row 2 of
   profiles/r13_window_loss_timing.jsonl).
3. wall time from the start of a window to the start of the next over 4 consecutive windows of ONE DepthOptimizer (after a first
   window that builds everything), 3 epochs each, fused_step on and off: restore against deep copy.
Three JSON lines.
    python scripts/optim_step_timing.py [--out profiles/r14_optim_step_timing.jsonl]
--profile-only runs nothing but 5 + 50 tcsfm_optim_step calls over the encoder set, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/optim_step_timing.py --profile-only
(k_optim<0>'s average duration there is the kernel time proper: profiles/r14_optim_kernel_stats.csv)."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

H, W = 192, 640
HBM_PEAK = 8.0e12
OPTIONS = dict(num_source_imgs=2, diff_img_argmin=True, automasking=True, l_inverse_reconstruction=True, l_depth_consist=True,
               l_depth_consist_weight=0.15, l_depth_init=True, l_depth_init_weight=0.1, l_smooth=False, l_smooth_weight=2, l_pose_consist=False)


def block_ms(f, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def median(v):
    return sorted(v)[len(v) // 2]


def time_step(profile_only=False):
    from tightly_coupled_sfm_amd.depthnet_train import _is_buffer, _shapes
    from tightly_coupled_sfm_amd.optim import LibraryOptimizer
    shapes = {k: s for k, s in _shapes().items() if not _is_buffer(k)}
    out = {}
    for name, keys in (("encoder", [k for k in shapes if k.startswith("encoder.")]), ("all", list(shapes)))[:1 if profile_only else 2]:
        gen = torch.Generator(device="cuda").manual_seed(14)
        mk = lambda: [torch.randn(shapes[k], device="cuda", generator=gen) * 0.05 for k in keys]
        sets = {v: [torch.nn.Parameter(t) for t in mk()] for v in ("library", "abi", "torch")}
        for ps in sets.values():
            for p in ps:
                p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
        lib_opt, abi_opt = LibraryOptimizer(sets["library"], kind="adam", lr=2e-4), LibraryOptimizer(sets["abi"], kind="adam", lr=2e-4)
        torch_opt = torch.optim.Adam(sets["torch"], lr=2e-4)
        n = len(keys)
        grads = (C.c_void_p * n)(*[p.grad.data_ptr() for p in sets["abi"]])
        lr = (C.c_double * n)(*[2e-4] * n)
        abi_opt.eng._bind()
        fs = {"library": lib_opt.step, "torch": torch_opt.step,
              "abi": lambda: abi_opt.lib.tcsfm_optim_step(abi_opt._o, grads, lr, 0.9, 0.999, 1e-8)}
        if profile_only:
            for _ in range(55):
                fs["abi"]()
            torch.cuda.synchronize()
            return {"profile_only": name, "elements": sum(p.numel() for p in sets["abi"]), "steps": 55}
        for f in fs.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fs}
        for _ in range(10):
            for k, f in fs.items():
                t[k].append(block_ms(f))
        med = {k: median(v) for k, v in t.items()}
        numel = sum(p.numel() for p in sets["abi"])
        rate = 28.0 * numel / (med["abi"] * 1e-3)
        out[name] = {"tensors": n, "elements": numel, "ms_median": {k: round(v, 4) for k, v in med.items()},
                     "ms_min": {k: round(min(v), 4) for k, v in t.items()}, "ms_max": {k: round(max(v), 4) for k, v in t.items()},
                     "torch_over_library": round(med["torch"] / med["library"], 2), "algorithmic_bytes": 28 * numel,
                     "abi_algorithmic_TBps": round(rate / 1e12, 3), "abi_share_of_8TBps_hbm_peak": round(rate / HBM_PEAK, 3)}
    return {"what": "one Adam step over the reference depth network's parameters", "variants": "library = LibraryOptimizer.step(), torch = "
            "torch.optim.Adam defaults, abi = tcsfm_optim_step with prebuilt tables", "method": "hip events around blocks of 20 steps, 10 "
            "alternating blocks, median per step (the span covers the host's launches as well as the kernel)", "sets": out}


def _window_inputs():
    import depthnet_twin as dt
    import pose_loop_grad_inputs as LI
    import standins
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    B, S = 1, 2
    im = torch.as_tensor(dt.sample_images(300 + H + W, S + 1, H, W)).float().cuda()
    K = torch.tensor([[[0.58 * W, 0, (W - 1) / 2], [0, 0.58 * W, (H - 1) / 2], [0, 0, 1]]], device="cuda")
    gts = [torch.zeros((B, 6), device="cuda") for _ in range(S)]
    data = (im[:1].contiguous(), [im[1:2].contiguous(), im[2:3].contiguous()], gts, gts, None, K, None, None, None, None, None)
    depth = DepthNetModule(dt.depthnet_params(0), max_images=S + 1).cuda()
    pose = standins.PoseNetTwin(LI.params()).cuda().eval()
    config = {"minibatch": B, "device": "cuda", "min_depth": 0.1, "max_depth": 100.0, "iterations": 2, "camera_height": 1.65}
    base = dict(OPTIONS, lr=2e-4, optimizer="adam", mode="scaled", avg_final_epochs=2, weight_tuning=True, optimize_depth_encoder=True)
    return data, depth, pose, config, base


def time_epoch():
    from tightly_coupled_sfm_amd.optimizer import DepthOptimizer
    data, depth, pose, config, base = _window_inputs()

    def window(fused_step, epochs):
        opt = DepthOptimizer(dict(base, epochs=epochs, fused_step=fused_step), config, pose, depth, "timing")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = opt.optimize_window(0, data)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r["losses"].tolist()
    for fs in (True, False):
        window(fs, 2)                 # warm-up
    t = {(f, e): [] for f in (True, False) for e in (6, 2)}
    seen = {}
    for _ in range(5):
        for key in t:
            ms, ls = window(*key)
            t[key].append(ms)
            seen[key] = ls
    med = {k: median(v) for k, v in t.items()}
    name = lambda f: "fused_step" if f else "torch_step"
    epoch = {name(f): (med[(f, 6)] - med[(f, 2)]) / 4 for f in (True, False)}
    return {"what": "one optimize_depth_encoder epoch of DepthOptimizer(weight_tuning=True)", "size": f"{W}x{H}", "B": 1, "S": 2, "iterations": 2,
            "method": "wall time of optimize_window at 6 and 2 epochs, alternating, medians of 5; epoch = (t6 - t2) / 4",
            "ms_window_median": {f"{name(f)}_{e}_epochs": round(v, 3) for (f, e), v in med.items()},
            "ms_epoch": {k: round(v, 3) for k, v in epoch.items()},
            "saving_us_per_epoch": round((epoch["torch_step"] - epoch["fused_step"]) * 1e3, 1),
            "losses_6_epochs": {name(f): seen[(f, 6)] for f in (True, False)}}


def time_windows():
    from tightly_coupled_sfm_amd.optimizer import DepthOptimizer
    data, depth, pose, config, base = _window_inputs()
    out = {}
    for fused_step in (True, False, True, False):
        opt = DepthOptimizer(dict(base, epochs=3, fused_step=fused_step), config, pose, depth, "timing")
        opt.optimize_window(0, data)          # the first window builds the copies, their native networks and the optimiser
        torch.cuda.synchronize()
        stamps = [time.perf_counter()]
        for w in range(4):
            opt.optimize_window(w + 1, data)   # (ends in the staged copy's synchronisation: the next window starts here)
            stamps.append(time.perf_counter())
        out.setdefault("fused_step" if fused_step else "deep_copy", []).append([round((b - a) * 1e3, 3) for a, b in zip(stamps, stamps[1:])])
    med = {k: median([x for run in v for x in run]) for k, v in out.items()}
    return {"what": "wall time from the start of a window to the start of the next, 4 consecutive windows of one DepthOptimizer, 3 epochs each",
            "size": f"{W}x{H}", "B": 1, "S": 2, "iterations": 2, "mode": "optimize_depth_encoder", "method": "two runs per variant, alternating; "
            "every window's time listed, median over the 8", "ms_windows": out, "ms_window_median": {k: round(v, 3) for k, v in med.items()},
            "saving_ms_per_window": round(med["deep_copy"] - med["fused_step"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_optim_step_timing.jsonl"))
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_timing.py needs a GPU: nothing is measured without one")
    if a.profile_only:
        print(json.dumps(time_step(profile_only=True)))
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []
    for f in (time_step, time_epoch, time_windows):
        lines.append(json.dumps(f()))
        print(lines[-1], flush=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
