"""Shared by tests/test_resize_cpu.py, tests/test_gpu_resize.py and tests/golden/make_golden_resize.py: a NumPy restatement of Pillow's
8-bit Lanczos resize (Image.resize((W, H), Image.LANCZOS), which Image.ANTIALIAS named), the table of cases, and the input generator.

The algorithm (Pillow's Resample.c, restated; include/tcsfm.h: tcsfm_resize_coeffs): per axis, input length `in` -> output length `out`

    scale = in / out;  fs = max(scale, 1.0);  support = 3.0 * fs;  ksize = (int)ceil(support) * 2 + 1
    for xx in 0 .. out-1:
        center = (xx + 0.5) * scale
        xmin = max((int)(center - support + 0.5), 0);   n = min((int)(center + support + 0.5), in) - xmin          (C truncation)
        w[x] = lanczos((x + xmin - center + 0.5) / fs), x = 0 .. n-1;   ww = w[0] + w[1] + ... (in this order);   w[x] /= ww
        k[x] = (int)(w[x] < 0 ? -0.5 + w[x] * 4194304.0 : 0.5 + w[x] * 4194304.0)
    lanczos(t) = sinc(t) * sinc(t / 3) for -3 <= t < 3, else 0;  sinc(0) = 1, sinc(t) = sin(pi t) / (pi t)

and a pass is acc = (1 << 21) + sum byte[xmin + x] * k[x] in int32, byte = clamp(acc >> 22, 0, 255); horizontal first, then vertical on
the horizontal pass's BYTES; a pass with in == out is skipped.  Python floats are C doubles and math.sin is the C library's sin, so the
table is the one a C program computes.

Nothing here imports PIL or torch: the fixture tests/golden/golden_resize.npz carries Pillow's bytes."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_resize.npz")

PRECISION_BITS = 22
TILE = 32                    # the kernel's output tile (csrc/resize_u8_kernel.h: RZ_TW = RZ_TH)

#         name             source h, w   H, W     frames
CASES = [("kitti_ratio",    (47, 79),  (24, 40), 3),      # KITTI's ratio, both passes; 47 * 79 * 3 is odd: frames 1 and 2 sit at other alignments
         ("vertical_only",  (91, 40),  (24, 40), 1),      # 3.79x
         ("horizontal_only", (24, 157), (24, 40), 1),     # 3.9x
         ("upscale",        (5, 7),    (8, 16), 1),       # windows cut at both borders
         ("same_size",      (24, 40),  (24, 40), 1),      # both passes skipped
         ("two_tiles",      (95, 161), (48, 40), 2)]      # 32 x 32 tiles: two per axis, the last one partial in each (16 rows, 8 columns); 4.03x horizontally
CASE = {c[0]: c for c in CASES}
assert all(-(-c[2][0] // TILE) >= 2 and -(-c[2][1] // TILE) >= 2 and c[2][0] % TILE and c[2][1] % TILE for c in CASES if c[0] == "two_tiles")

# sequences for the sequence calls: T camera-size frames (synth.make_sequence at the source size, quantised), resized by Pillow
#          name        source h, w   H, W      T
SEQUENCES = [("seq",     (47, 79),  (24, 40), 20),
             ("seq_net", (63, 125), (32, 64), 8)]         # the depth network takes multiples of 32 only
SEQUENCE = {s[0]: s for s in SEQUENCES}

# camera sizes of the reference's datasets -> the sizes its networks read
REAL = [((376, 1241), (192, 640)), ((968, 1296), (256, 448))]


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    return _sinc(t) * _sinc(t / 3.0) if -3.0 <= t < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(inn, out):
    """-> (ksize, bounds int32 [out,2] = (xmin, n), kk int32 [out,ksize], zero beyond n)"""
    scale = inn / out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out, 2), dtype=np.int32)
    kk = np.zeros((out, ksize), dtype=np.int32)
    for xx in range(out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), inn) - xmin
        w = [_lanczos((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, n)
    return ksize, bounds, kk


def _pass(img, axis, out):
    """one pass along `axis` of uint8 img -> (uint8 result, smallest and largest sum BEFORE the clip)"""
    inn = img.shape[axis]
    _, bounds, kk = coeffs(inn, out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    acc = np.empty((out,) + src.shape[1:], dtype=np.int64)
    for xx in range(out):
        xmin, n = (int(v) for v in bounds[xx])
        acc[xx] = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
    assert int(np.abs(acc).max()) < 2 ** 31                 # (Pillow's int32 sums do not wrap)
    res = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(res, 0, axis), (int(acc.min()), int(acc.max()))


def resize(img, H, W):
    """uint8 [N,h,w,3] -> (uint8 [N,H,W,3], {"h": (min, max) sums of the horizontal pass, "v": ... of the vertical}; a skipped pass: None)"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 4 and img.shape[3] == 3
    stats = {"h": None, "v": None}
    if img.shape[2] != W:
        img, stats["h"] = _pass(img, 2, W)
    if img.shape[1] != H:
        img, stats["v"] = _pass(img, 1, H)
    return np.ascontiguousarray(img), stats


def clips_both_ways(stats):
    """a pass that ran saw a sum below 0 AND one above 255 * 2^22 before its clip"""
    return all(s is None or (s[0] < 0 and s[1] >= (256 << PRECISION_BITS)) for s in stats.values())


def make_input(name):
    """uint8 [N,h,w,3]: random bytes with blocks of 0 / 255 bands along rows and along columns -- hard edges, whose Lanczos overshoot
    leaves [0, 255] on both sides in both passes.  The fixture stores the result: tests read it from there."""
    _, (h, w), _, N = CASE[name]
    rng = np.random.default_rng(sum(ord(ch) for ch in name) * 1000 + h * w)
    img = rng.integers(0, 256, size=(N, h, w, 3), dtype=np.uint8)
    bh, bw = max(2, h // 10), max(2, w // 10)                # band thickness: wider than the filter's inner lobe at the case's ratio
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    rows = (((y // bh) % 2) * 255 + 0 * x).astype(np.uint8)  # bands along rows: edges for the vertical pass
    cols = (((x // bw) % 2) * 255 + 0 * y).astype(np.uint8)  # bands along columns: edges for the horizontal pass
    checks = ((((y // bh) + (x // bw)) % 2) * 255).astype(np.uint8)
    for f in range(N):
        if h < 16 or w < 16:                                 # (the upscaling case: all of it)
            img[f, :, :, :] = checks[:, :, None]
            img[f, f % h, :, 1] = rng.integers(0, 256, size=w, dtype=np.uint8)
            continue
        img[f, : h // 2, : w // 2, :] = rows[: h // 2, : w // 2, None]
        img[f, h // 2:, w // 2:, :] = cols[h // 2:, w // 2:, None]
        img[f, : h // 3, w - w // 3:, f % 3] = checks[: h // 3, w - w // 3:]
    return img


def make_sequence_input(name):
    """uint8 [T,h,w,3]: the synthetic corridor at the camera's size, quantised to bytes"""
    from tightly_coupled_sfm_amd import synth
    _, (h, w), _, T = SEQUENCE[name]
    seq = synth.make_sequence(T, h, w, seed=4)
    q = np.round(np.asarray(seq["frames"], dtype=np.float64) * 255).clip(0, 255).astype(np.uint8)
    return np.ascontiguousarray(q.transpose(0, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def golden():
    """{in_<name>, out_<name>: uint8 [N,h,w,3] / [N,H,W,3]} for every case and sequence: the inputs and PILLOW's bytes"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
