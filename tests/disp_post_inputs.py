"""Shared by the disparity post-processing tests: the golden vectors, the NumPy restatement of the reference's blend and the frames.

post_process restates utils/learning_helpers.py:115-123 (batch_post_process_disparity) on float32 planes with np.linspace: the same
operations in the same order; tests/test_disp_post_cpu.py pins it to the reference's own output (golden_disp_post.npz) bit for bit, so the GPU tests
may use it at sizes the golden file does not hold."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SHAPES = [(2, 8, 64), (1, 4, 96), (1, 3, 33)]


@functools.lru_cache(maxsize=None)
def golden():
    """[(l float32, r float32 -- already un-flipped --, post float64)] at GOLDEN_SHAPES"""
    g = np.load(os.path.join(HERE, "golden", "golden_disp_post.npz"))
    return [(g[f"l{k}"], g[f"r{k}"], g[f"post{k}"]) for k in range(len(GOLDEN_SHAPES))]


def ramp(w):
    """l_mask of the blend for width w, float64 [w]"""
    return 1.0 - np.clip(20 * (np.linspace(0, 1, w) - 0.05), 0, 1)


def post_process(l_disp, r_disp):
    """l_disp, r_disp [n,h,w] float32 (r_disp un-flipped) -> float64 [n,h,w]"""
    assert l_disp.dtype == np.float32 and r_disp.dtype == np.float32
    lm = ramp(l_disp.shape[2])                     # float64 [w], broadcast over the rows: the meshgrid's values
    rm = lm[::-1]
    mean = 0.5 * (l_disp + r_disp)                 # float32
    return rm * l_disp + lm * r_disp + (1.0 - lm - rm) * mean


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(view), b.view(view))


def frames(n, h, w, seed=7):
    """n deterministic float32 frames [n,3,h,w] in [0,1]: smooth gradients plus texture, not symmetric under a horizontal flip"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, 3, h, w), np.float32)
    for i in range(n):
        for c in range(3):
            base = 0.5 + 0.3 * np.sin(2 * np.pi * ((1 + c) * x * (1 + 0.3 * i) + 0.7 * y + 0.1 * i)) * (0.4 + 0.6 * x)
            out[i, c] = np.clip(base + 0.15 * rng.uniform(-1, 1, size=(h, w)), 0, 1)
    return out
