"""Drop-in for the reference's paper_plots_and_data/evaluate_depth_eigen.py: the Eigen depth table from disparity planes.

compute_errors has the reference's signature and runs on the host in NumPy.  evaluate does the script's loop (lines 131-177) on the
device through Engine.depth_eval / Engine.sequence_depth_eval: the resize to the ground truth's size, 30 / disp, mask and crop, median
scaling, clip and the seven metrics of every frame in one launch per group of frames (include/tcsfm.h "Evaluation").  KITTI's ground
truth has a handful of sizes, one call takes one size: the frames are grouped by size."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def compute_errors(gt, pred):
    """The seven Eigen metrics of masked depth vectors, in the order of NAMES (the reference function's signature and result; host
    NumPy, in the inputs' own types: a float32 `gt` gets a float32 log, as there).  The device path is Engine.depth_eval."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    diff = gt - pred
    sq = diff * diff
    log_diff = np.log(gt) - np.log(pred)
    worse = np.maximum(gt / pred, pred / gt)                     # how far off, whichever way: >= 1
    within = [np.mean(worse < 1.25 ** k) for k in (1, 2, 3)]
    return (np.mean(np.abs(diff) / gt), np.mean(sq / gt), np.sqrt(np.mean(sq)), np.sqrt(np.mean(log_diff * log_diff)), *within)


def load_gt_depths(path: str):
    """the `data` entry of a gt_depths.npz as the KITTI export writes it -> list of float32 planes, one per frame (sizes may differ).
    The file holds a pickled object array, written under Python 2 in the published splits: hence allow_pickle and latin1."""
    with np.load(path, allow_pickle=True, encoding="latin1") as archive:
        return list(archive["data"])


def _by_size(gt_depths):
    groups = {}
    for i, g in enumerate(gt_depths):
        groups.setdefault(tuple(np.asarray(g).shape[:2]), []).append(i)
    return groups


def evaluate(pred_disps, gt_depths: Sequence[np.ndarray], engine, benchmark: str = "eigen", median_scaling: bool = True,
             min_depth: float = 1e-3, max_depth: float = 80.0, depth_unit: float = 30.0, first: int = 0, batch: int = 32) -> dict:
    """pred_disps: [n,H,W] disparity planes at the engine's size (NumPy or CUDA tensor, float32 or float64), or None for the planes the
    engine's last sequence call kept (disparity="plain" / "post"): frame first + i against gt_depths[i].  gt_depths: n float32 planes,
    sizes may differ.  -> dict(errors [n,7], mean_errors [7], ratios [n], med, std: the reference's printed median of the ratios and
    std(ratios / med), metrics [n,10]: the engine's rows)"""
    import torch
    n = len(gt_depths)
    if n < 1:
        raise ValueError("evaluate: no ground truth")
    if pred_disps is not None and len(pred_disps) != n:
        raise ValueError(f"evaluate: {len(pred_disps)} disparity planes for {n} ground-truth planes")
    metrics = np.empty((n, 10), dtype=np.float64)
    kw = dict(protocol=benchmark, median_scaling=median_scaling, min_depth=min_depth, max_depth=max_depth, depth_unit=depth_unit)
    for _, idx in sorted(_by_size(gt_depths).items()):
        # runs of consecutive frames of one size go up together
        runs, start = [], 0
        for k in range(1, len(idx) + 1):
            if k == len(idx) or idx[k] != idx[k - 1] + 1 or k - start >= batch:
                runs.append(idx[start:k]); start = k
        for run in runs:
            gt = np.stack([np.asarray(gt_depths[i], dtype=np.float32) for i in run])
            if pred_disps is None:
                metrics[run] = engine.sequence_depth_eval(gt, first=first + run[0], **kw)
            else:
                d = pred_disps[run[0]:run[-1] + 1]
                d = d if isinstance(d, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(d))
                metrics[run] = engine.depth_eval(d.to(engine.dev), torch.from_numpy(gt).to(engine.dev), **kw).cpu().numpy()
    ratios = metrics[:, 7].copy()
    med: Optional[float] = float(np.median(ratios)) if median_scaling else None
    std = float(np.std(ratios / med)) if median_scaling else None
    return dict(errors=metrics[:, :7].copy(), mean_errors=metrics[:, :7].mean(0), ratios=ratios, med=med, std=std, metrics=metrics)


def format_table(result: dict) -> str:
    """the table as the reference's script prints it, so that outputs can be compared line by line: the scaling ratios' median and
    spread (with median scaling), a blank line, the metric names right-aligned in columns of eight, the means as LaTeX cells"""
    out = []
    if result["med"] is not None:
        out.append(f" Scaling ratios | med: {result['med']:.3f} | std: {result['std']:.3f}")
    out.append("")
    out.append("  " + "".join(f"{name:>8} | " for name in NAMES))
    out.append("".join(f"&{float(v): 5.3f} " for v in result["mean_errors"]))
    return "\n".join(out)
