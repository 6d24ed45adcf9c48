#!/usr/bin/env python3
"""ms per tcsfm_create and per tcsfm_destroy of a 192x640 handle with max_pairs = 4 through the C ABI (guard bands off): 5 warm-up pairs,
then the medians over 40.  One JSON line.
    python scripts/diag/create_destroy_timing.py [ROOT]      # ROOT: the tree whose package is measured (default: this one)"""
import ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tightly_coupled_sfm_amd import _lib
lib = _lib.load()
torch.cuda.init(); torch.cuda.synchronize()


def once():
    h = C.c_void_p()
    t0 = time.perf_counter()
    assert lib.tcsfm_create(C.byref(h), 0, 192, 640, 4) == 0
    t1 = time.perf_counter()
    lib.tcsfm_destroy(h)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


for _ in range(5):
    once()
v = [once() for _ in range(40)]
print(json.dumps({"script": "create_destroy", "HxW": "192x640", "max_pairs": 4, "create_ms_median": round(statistics.median(a for a, _ in v), 4),
                  "destroy_ms_median": round(statistics.median(b for _, b in v), 4), "n": len(v)}))
