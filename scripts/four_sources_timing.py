#!/usr/bin/env python3
"""Dense window mode on the reference's loss at S = 2 and S = 4 sources per target (the three- and five-frame windows) at 192 x 640:
time per call of a B = 1 window and of the reference driver's minibatch of six windows (one call in flight, device pointers, 4 Gauss-Newton
iterations, w_dc 0.15, prior_init 0.1) -> one JSON line per case (profiles/r06_four_sources_timing.jsonl).  Run under
`rocprofv3 --kernel-trace --stats` with `--reps 3` for the per-kernel split (profiles/r06_four_sources_kernel_stats.csv).
    python scripts/four_sources_timing.py [--reps N]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, torch
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process: HIP_FORCE_DEV_KERNARG / GPU_MAX_HW_QUEUES when absent)
from tightly_coupled_sfm_amd import _lib
from tightly_coupled_sfm_amd.engine import Engine, default_opts
import test_gpu_four_sources as T

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
H, W, mind, maxd = 192, 640, 0.06, 2.67
for S in (2, 4):
    for B in (1, 6):
        w = T._window(B, S, H, W, seed=31)
        t = {k: T._dev(v) for k, v in w.items()}
        dt4, ds5 = t["depth_t"][:, None].contiguous(), t["depth_s"][:, :, None].contiguous()
        e = Engine(H, W, 2 * S * B)
        o = default_opts(n_iters=4, w_dc=0.15, prior_init=0.1, min_depth=mind, max_depth=maxd, window_rule=_lib.WINDOW_REFERENCE)
        run = lambda: e.refine_dense_window(t["tgt"], t["srcs"], dt4, ds5, t["K"], t["pose"], o, argmin=True)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run(); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        ms = np.array(ms)
        print(json.dumps(dict(H=H, W=W, S=S, B=B, n_iters=4, reps=args.reps, us_per_call_median=float(np.median(ms) * 1e3),
                              us_per_call_min=float(ms.min() * 1e3), us_per_window=float(np.median(ms) * 1e3 / B))), flush=True)
        e.close()
