"""Generate tests/golden/golden_depth_eval.npz: the reference's own per-frame evaluation (paper_plots_and_data/evaluate_depth_eigen.py)
on already-resized predictions.

Run where make_golden.py runs (it needs the reference checkout, imported as make_golden.py imports it):
    python tests/golden/make_golden_depth_eval.py
The script's loop body lives under `if __name__ == '__main__'`, so lines 143-166 (mask, crop, median scaling, clip: no cv2 in them) are
read from the reference's file and executed as they stand around the module's own compute_errors; nothing of them is copied here.
Inputs: pred_depth = 30 / disparity with the disparity uniform in [1 / 2.67, 1 / 0.06] at the ground truth's size (float64, what
cv2.resize would have returned), gt float32 with holes.  Stored per case k: gt{k}, pred{k} (the inputs), bench{k} (0: eigen,
1: eigen_benchmark), errors{k} (the seven metrics), ratio{k}, n_valid{k}, n_median{k}.  Data only."""
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

#        gt_h gt_w benchmark         valid  far   (far: fraction of the valid pixels at or beyond 80 m)
CASES = [(16, 40, "eigen", 0.45, 0.05),
         (17, 41, "eigen", 0.45, 0.0),
         (9, 23, "eigen_benchmark", 0.30, 0.10),
         (10, 22, "eigen_benchmark", 0.50, 0.0)]


def import_script():
    """the reference's evaluate_depth_eigen as a module (its __main__ block does not run) and its source lines"""
    import make_golden
    make_golden.import_reference()
    import types
    for name in ("matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = types.ModuleType(name); m.use = lambda *a, **k: None
                sys.modules[name] = m
    ref = make_golden.REF
    for name, attrs in (("models.depth_models", ["depth_model"]), ("models.pose_models", ["pose_model"]),
                        ("data.kitti_loader_eigen", ["KittiLoaderPytorch"]), ("utils.custom_transforms", [])):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = types.ModuleType(name)
                for a in attrs:
                    setattr(m, a, None)
                sys.modules[name] = m
    path = os.path.join(ref, "paper_plots_and_data", "evaluate_depth_eigen.py")
    sys.path.insert(0, os.path.dirname(path))
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_evaluate_depth_eigen", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(path) as f:
        lines = f.read().split("\n")
    return mod, lines


def main():
    import depth_eval_inputs as D
    mod, lines = import_script()
    body = textwrap.dedent("\n".join(lines[142:166]))            # lines 143-166
    assert body.lstrip().startswith('if benchmark == "eigen":') and "pred_depth[pred_depth > MAX_DEPTH] = MAX_DEPTH" in body
    code = compile(body, "evaluate_depth_eigen.py:143-166", "exec")
    out = {}
    for k, (gh, gw, bench, valid, far) in enumerate(CASES):
        disp = D.disparity(gh, gw, seed=100 + k)
        gt = D.ground_truth(disp, gh, gw, seed=200 + k, valid=valid, far=far)      # (same size: its resize is the identity)
        pred = 30 / disp
        ns = dict(np=np, benchmark=bench, MIN_DEPTH=1e-3, MAX_DEPTH=80, median_scaling=True, ratios=[], gt_depth=gt.copy(),
                  pred_depth=pred.copy(), gt_height=gh, gt_width=gw)
        exec(code, ns)
        errors = mod.compute_errors(ns["gt_depth"], ns["pred_depth"])
        out[f"gt{k}"], out[f"pred{k}"], out[f"bench{k}"] = gt, pred, np.int32(bench == "eigen_benchmark")
        out[f"errors{k}"] = np.array(errors, dtype=np.float64)
        out[f"ratio{k}"] = np.float64(ns["ratios"][0])
        out[f"n_valid{k}"] = np.int64(ns["gt_depth"].size)
        out[f"n_median{k}"] = np.int64((ns["gt_depth"] < 80).sum())
        print(k, bench, out[f"n_valid{k}"], out[f"n_median{k}"], out[f"ratio{k}"], out[f"errors{k}"])
    out["n_cases"] = np.int32(len(CASES))
    path = os.path.join(HERE, "golden_depth_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
