"""Inputs and judging rules shared by tests/test_operators_inputs_cpu.py and tests/test_gpu_operators.py: the drop-in operators
(warp, PoseNet input, photometric maps, SSIM, smoothness, disparity to depth, loss surface, DNet scale recovery) against float64.

INPUTS.  synth.make_batch pairs in which every item differs in images, both depth maps, intrinsics and pose: item n gets its own
focal lengths and principal point and its own scaling of both depth maps (make_batch renders every target depth from the same
room, so without this all target depth maps of a batch would be equal).  Every case is run at the ground-truth poses and at 30
times those, where most samples leave the frame (out-of-bounds sentinel, zero-pad border blend, Z clamp).

JUDGING.  A discrete output (warp validity, auto-mask, ground mask) may differ from the float64 oracle at a few near-tie pixels.
Those DECISION PIXELS are left out of the value comparison, but their number per item is capped (decision_cap: 0.1 % of the frame,
one pixel below 1000 pixels); above the cap the test fails.  The cap is asserted for the oracle's own fp32 build as well, so an
input that breaks it without any kernel involved is caught as a bad input.  An auto-mask flip inside the 3 x 3 neighbourhood of a
validity flip is a consequence of that flip (the SSIM window of the neighbour reads the flipped reconstruction; one such pixel
at 100 x 333 moves a neighbour's diff by 9e-3) and is not counted a second time.
Every other pixel is held to   bound = max(existing absolute bound of that map, MARGIN * max |oracle32 - oracle64|)   on the same
inputs: the bound rests on the reference's two builds only, never on what the kernels return.  MARGIN = 4 grants two bits for the
kernels' different contraction and ordering of the same fp32 operations (fused multiply-adds, __expf, the summation order over
the 3 x 3 window).
"""
import functools

import numpy as np

from tightly_coupled_sfm_amd import synth

MARGIN = 4.0
# (H, W, N): less than one 256-thread block (the smallest frames of the engine's own tests) / ragged last block, odd widths / the
# two production sizes
SHAPES = [(5, 9, 3), (17, 33, 3), (37, 53, 3), (100, 333, 2), (192, 640, 2), (256, 448, 2)]
MANY = (37, 53, 19)                      # one call with many items, on an Engine whose max_pairs (MANY_MAX_PAIRS) is larger
MANY_MAX_PAIRS = 24
POSE_SCALES = (1.0, 30.0)
SSIM_SHAPES = [(37, 53), (100, 333), (192, 640), (256, 448)]
SURFACE_SHAPES = [(100, 333), (192, 640)]
CAM_HEIGHT = 1.65

# the absolute bounds the suite already uses for these maps (tests/test_gpu_parity.py, tests/test_gpu_options.py): the floors
FLOOR = dict(rec=1e-4, proj_depth=2e-4, comp_depth=1e-5, diff=3e-5, weight=1e-4, auto_err=2e-5, ssim=2e-6, height=2e-5)


def decision_cap(hw):
    return 1 if hw < 1000 else int(1e-3 * hw)


def dilate3(m):
    """3 x 3 neighbourhood of a boolean map (no wrap-around)"""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dv in range(3):
        for du in range(3):
            out |= p[dv:dv + m.shape[0], du:du + m.shape[1]]
    return out


def bound(floor, e32):
    return max(floor, MARGIN * e32)


def _maxabs(a, b, sel=None):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    if sel is not None:
        d = d[..., sel]
    return float(d.max()) if d.size else 0.0


@functools.lru_cache(maxsize=None)
def make_case(H, W, N, pose_scale):
    """-> dict of float32 arrays: tgt, src [N,3,H,W]; depth_t, depth_s [N,1,H,W]; K [N,3,3]; pose [N,6]"""
    b = synth.make_batch(N, H, W, seed0=700 + 3 * H + W)
    K = b["K"].copy()
    depth_t, depth_s = b["depth_t"].copy(), b["depth_s"].copy()
    for n in range(N):
        K[n, 0, 0] *= 1 + 0.004 * (n + 1); K[n, 1, 1] *= 1 - 0.003 * (n + 1)
        K[n, 0, 2] += 0.37 * (n + 1) * W / 640.0; K[n, 1, 2] -= 0.21 * (n + 1) * H / 192.0
        depth_t[n] *= np.float32(1 + 0.011 * (n + 1)); depth_s[n] *= np.float32(1 - 0.007 * (n + 1))
    pose = (b["pose_gt"].astype(np.float64) * pose_scale).astype(np.float32)
    return dict(tgt=b["tgt"], src=b["src"], depth_t=depth_t, depth_s=depth_s, K=K, pose=pose)


PAIR_CASES = [(H, W, N, s) for (H, W, N) in SHAPES + [MANY] for s in POSE_SCALES]
PAIR_IDS = [f"{H}x{W}-N{N}-pose_x{s:g}" for (H, W, N, s) in PAIR_CASES]


def items_differ(c):
    """every item of the batch differs from every other in every input"""
    N = c["tgt"].shape[0]
    return all(not np.array_equal(c[k][i], c[k][j]) for k in c for i in range(N) for j in range(i))


# ---------------------------------------------------------------------------------------------------------------------------------
# warp
WARP_MAPS = ("rec", "proj_depth", "comp_depth")


def oracle_warp(orc, c, n):
    rec, valid, pd, cd = orc.warp(c["src"][n], c["depth_t"][n, 0], c["depth_s"][n, 0], c["pose"][n], c["K"][n])
    return dict(rec=rec, valid=valid, proj_depth=pd, comp_depth=cd)


def judge_warp(got, ref, tag):
    """one item's warp maps (dict as oracle_warp) against the float64 ones -> {map: max error outside the decision pixels};
    asserts the cap on the decision pixels"""
    flip = got["valid"] != ref["valid"]
    assert flip.sum() <= decision_cap(flip.size), (tag, "validity decisions", int(flip.sum()), flip.size)
    ok = ~flip
    scale = max(1.0, float(np.abs(ref["comp_depth"]).max()))
    # the computed depth is a smooth function of the pixel, validity or not: every pixel is compared
    return dict(rec=_maxabs(got["rec"], ref["rec"], ok), proj_depth=_maxabs(got["proj_depth"], ref["proj_depth"], ok),
                comp_depth=_maxabs(got["comp_depth"], ref["comp_depth"]) / scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# photometric maps
PHOTO_MAPS = ("diff", "weight", "auto_err", "rec")
PHOTO_WEIGHTS = [(0.15, 0.85), (0.4, 0.6)]


def oracle_photometric(orc, c, n, w_l1, w_ssim):
    return orc.photometric(c["tgt"][n], c["src"][n], c["depth_t"][n, 0], c["depth_s"][n, 0], c["pose"][n], c["K"][n],
                           w_l1=w_l1, w_ssim=w_ssim)


def judge_photometric(got, ref, tag):
    """one item's six maps (dict with the oracle's keys) against the float64 ones -> {map: max error outside the decision pixels}"""
    vflip = got["valid"] != ref["valid"]
    near = dilate3(vflip)
    aflip = (got["auto_mask"] != ref["auto_mask"]) & ~near
    n_dec = int(vflip.sum() + aflip.sum())
    assert n_dec <= decision_cap(vflip.size), (tag, "validity / auto-mask decisions", int(vflip.sum()), int(aflip.sum()), vflip.size)
    ok = ~near
    # the auto-mask error compares the target with the UNWARPED source: no warp decision enters it, every pixel is compared
    return dict(diff=_maxabs(got["diff"], ref["diff"], ok), weight=_maxabs(got["weight"], ref["weight"], ok),
                auto_err=_maxabs(got["auto_err"], ref["auto_err"]), rec=_maxabs(got["rec"], ref["rec"], ~vflip))


# ---------------------------------------------------------------------------------------------------------------------------------
# SSIM
@functools.lru_cache(maxsize=None)
def make_ssim_planes(H, W):
    """x, y [N=3, C=3, H, W] float32: textured planes, constant planes (variance exactly zero), planes of zeros and ones"""
    b = synth.make_batch(2, H, W, seed0=40 + H)
    rng = np.random.default_rng(H * 1000 + W)
    x = np.concatenate([b["tgt"], np.empty((1, 3, H, W), np.float32)])
    y = np.concatenate([b["src"], np.empty((1, 3, H, W), np.float32)])
    x[1, 1] = 0.625; y[1, 1] = 0.625                     # both constant and equal
    x[1, 2] = 0.25                                       # constant against texture
    x[2, 0] = rng.integers(0, 2, (H, W)); y[2, 0] = rng.integers(0, 2, (H, W))      # values exactly 0 and 1
    x[2, 1] = 1.0; y[2, 1] = 0.0
    x[2, 2] = rng.uniform(0, 1, (H, W)); y[2, 2] = rng.uniform(0, 1, (H, W))       # no spatial correlation at all
    x[2, 2, :, -1] = 1.0; y[2, 2, -1, :] = 0.0
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def ssim_regions(H, W):
    """the first and last rows and columns separately (a reflection error must not hide in the interior's statistics)"""
    r = {k: np.zeros((H, W), bool) for k in ("first_row", "last_row", "first_col", "last_col")}
    r["first_row"][0] = True; r["last_row"][-1] = True; r["first_col"][:, 0] = True; r["last_col"][:, -1] = True
    r["interior"] = np.zeros((H, W), bool); r["interior"][1:-1, 1:-1] = True
    return r


def oracle_ssim(orc, x, y):
    return np.stack([orc.ssim(x[n], y[n]) for n in range(x.shape[0])])


# ---------------------------------------------------------------------------------------------------------------------------------
# smoothness
@functools.lru_cache(maxsize=None)
def make_smooth(H, W, N):
    """disp [N,1,H,W], img [N,3,H,W] float32 with a different mean disparity per item"""
    rng = np.random.default_rng(H * 7 + W + N)
    disp = np.stack([rng.uniform(0.05, 0.9, (1, H, W)) * (0.25 + 0.45 * n) for n in range(N)])
    img = rng.uniform(0, 1, (N, 3, H, W))
    return disp.astype(np.float32), img.astype(np.float32)


def smooth_reference(disp, img, dtype):
    """the reference expression (losses.get_smooth_loss on CPU tensors takes the torch path) in the given torch dtype"""
    import torch
    from tightly_coupled_sfm_amd import losses
    return float(losses.get_smooth_loss(torch.tensor(disp, dtype=dtype), torch.tensor(img, dtype=dtype)))


# ---------------------------------------------------------------------------------------------------------------------------------
# disparity to depth
DISP_N = 65536 * 256 + 77        # more blocks of 256 than fit one grid row of 65535, ragged last block
MIN_DEPTH, MAX_DEPTH = 0.06, 2.67


@functools.lru_cache(maxsize=None)
def make_disp():
    d = np.random.default_rng(11).uniform(0, 1, DISP_N).astype(np.float32)
    d[0] = 0.0; d[1] = 1.0; d[-1] = 1.0; d[-2] = 0.0; d[65535 * 256] = 0.0; d[65535 * 256 + 1] = 1.0
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# loss surface
@functools.lru_cache(maxsize=None)
def make_surface(H, W):
    """one pair (item 1 of a two-item case: own intrinsics) and two sweeps of 21 poses: along z and in yaw"""
    c = make_case(H, W, 2, 1.0)
    one = {k: v[1:2] for k, v in c.items()}
    sweeps = []
    for idx, step in ((2, 2e-3), (4, 2e-4)):
        poses = np.repeat(one["pose"].astype(np.float32), 21, 0)
        poses[:, idx] += (np.arange(21, dtype=np.float32) - 10) * np.float32(step)
        sweeps.append(poses)
    return one, sweeps


def oracle_surface(orc, one, poses):
    return np.array([orc.cost(one["tgt"][0], one["src"][0], one["depth_t"][0, 0], one["depth_s"][0, 0], p, one["K"][0]) for p in poses])


# ---------------------------------------------------------------------------------------------------------------------------------
# scale recovery: heights and masks
@functools.lru_cache(maxsize=None)
def make_ground(H, W, N):
    """depth [N,1,H,W], K [N,3,3]: the synthetic room's depth with 0.2 % noise, so that the normals are not axis-aligned"""
    c = make_case(H, W, N, 1.0)
    rng = np.random.default_rng(H + W)
    depth, K = c["depth_t"], c["K"]
    if H < 8:        # the room has no ground in a frame of a few rows: ground planes of different heights under cameras that look down
        K = K.copy(); K[:, 1, 2] = -1.5 - 0.3 * np.arange(N)
        depth = np.stack([plane(H, W, K[n], 0.3 + 0.1 * n) for n in range(N)])[:, None]
    depth = (depth * (1 + 0.002 * rng.standard_normal(depth.shape))).astype(np.float32)
    return depth, K


def judge_ground(h, m, h64, m64, tag):
    flip = m != m64
    assert flip.sum() <= decision_cap(flip.size), (tag, "ground-mask decisions", int(flip.sum()), flip.size)
    return _maxabs(h, h64, ~flip) / float(h64.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# scale recovery: the median, exactly
def lower_median(heights, masks, pad_to_batch=0):
    """torch.median of the masked heights of a batch [N,H,W] that the reference pads to `pad_to_batch` images with copies of image 0
    (dnet_layers.py:307-311): sorted[(count - 1) // 2] -> (median as np.float32 or NaN, count, the padded float32 array)"""
    N = heights.shape[0]
    order = list(range(N)) + [0] * max(0, pad_to_batch - N)
    v = np.concatenate([heights[n][masks[n] > 0.5].astype(np.float32).ravel() for n in order]) if order else np.zeros(0, np.float32)
    if v.size == 0:
        return np.float32(np.nan), 0, v
    return np.sort(v)[(v.size - 1) // 2], int(v.size), v


def pinhole(H, W):
    """the synthetic camera; for a frame of a few rows with the principal point above the frame, so that every row looks down at
    the ground (with it inside, no 3 x 3 neighbourhood of a 5-row frame lies below the horizon)"""
    K = synth.scaled_K(H, W).astype(np.float32)
    if H < 8:
        K[1, 2] = -1.5
    return K


def wall(H, W, seed, depth=1.0):
    """a fronto-parallel wall with 0.1 % noise: normals along z, no ground anywhere"""
    return (depth * (1 + 0.001 * np.random.default_rng(seed).standard_normal((H, W)))).astype(np.float32)


def plane(H, W, K, cam_height):
    """the noiseless ground plane Y = cam_height below the principal point, the wall (depth 1) above it"""
    v = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    y = (v - float(K[1, 2])) / float(K[1, 1])
    d = np.ones((H, W))
    d[y > 1e-3] = cam_height / y[y > 1e-3]
    return np.minimum(d, 50.0).astype(np.float32)


def few_ground_pixels(orc32, orc64, H, W, count):
    """search for a depth map with exactly `count` ground pixels: a noisy wall with a small patch of the ground plane set into it.
    The normal of a pixel reads its 8 neighbours and border pixels take the normal of a reflected interior pixel, so which patch
    gives which count is found by trying patches with both builds of the oracle (they must agree) -> depth [H,W] float32"""
    K = pinhole(H, W)
    for seed in range(300):
        rng = np.random.default_rng(100 + seed)
        d = wall(H, W, seed)
        ground = plane(H, W, K, float(rng.uniform(0.2, 0.6)))
        ph, pw = int(rng.integers(2, 5)), int(rng.integers(2, 6))
        v0, u0 = int(rng.integers(0, H - ph + 1)), int(rng.integers(0, W - pw + 1))
        d[v0:v0 + ph, u0:u0 + pw] = ground[v0:v0 + ph, u0:u0 + pw]
        m32, m64 = orc32.ground_height(d, K)[1], orc64.ground_height(d, K)[1]
        if m32.sum() == count and m64.sum() == count and np.array_equal(m32, m64):
            return d
    raise AssertionError(f"no {H}x{W} depth map with {count} ground pixels found")


def median_cases(orc32, orc64):
    """-> list of (name, depth [N,1,H,W], K [N,3,3], pad_to_batch, expect) where expect is a dict of the structure the name claims:
    count (exact number of masked heights before padding) and / or parity, ties, byte ('low' / 'high')"""
    H, W = 37, 53
    K1 = pinhole(H, W)[None]
    rep = lambda K, n: np.ascontiguousarray(np.repeat(K, n, 0))
    noisy = make_ground(H, W, 3)
    one = few_ground_pixels(orc32, orc64, H, W, 1)
    two = few_ground_pixels(orc32, orc64, H, W, 2)
    flat = plane(H, W, K1[0], CAM_HEIGHT)
    cases = [("noisy-N3", noisy[0], noisy[1], 0, {}),
             ("noisy-N1", noisy[0][:1], noisy[1][:1], 0, {}),
             ("count1", one[None, None], K1, 0, dict(count=1)),
             ("count2", two[None, None], K1, 0, dict(count=2)),
             ("count3-odd", np.stack([one, two])[:, None], rep(K1, 2), 0, dict(count=3)),
             ("count4-even", np.stack([two, wall(H, W, 7), two * np.float32(1.5)])[:, None], rep(K1, 3), 0, dict(count=4)),
             ("ties-plane", np.stack([flat, flat])[:, None], rep(K1, 2), 0, dict(ties=True, byte="low")),
             # a power of two scales every height exactly: 4^n moves the top byte of the bit pattern and nothing else
             ("high-byte-3", np.stack([one * np.float32(4.0 ** n) for n in range(3)])[:, None], rep(K1, 3), 0, dict(count=3, byte="high")),
             ("high-byte-4", np.stack([one * np.float32(4.0 ** n) for n in (2, 0, 3, 1)])[:, None], rep(K1, 4), 0, dict(count=4, byte="high"))]
    for pad in (4, 9):                                   # N + 1 and 3 N for N = 3: image 0 counts 2 and 7 times
        cases.append((f"noisy-N3-pad{pad}", noisy[0], noisy[1], pad, {}))
        cases.append((f"count-2-0-1-pad{pad}", np.stack([two, wall(H, W, 8), one * np.float32(3.0)])[:, None], rep(K1, 3), pad, dict(count=3)))
    cases.append(("count-1-2-pad3", np.stack([one, two * np.float32(0.5)])[:, None], rep(K1, 2), 3, dict(count=3)))
    cases.append(("count1-pad2-N1", one[None, None], K1, 2, dict(count=1)))
    cases.append(("no-ground", wall(H, W, 9)[None, None], K1, 0, dict(count=0)))
    # frames smaller than one block, 5 x 9 the smallest the call accepts
    for (h, w) in ((5, 9), (17, 33)):
        g = make_ground(h, w, 3)
        k1 = pinhole(h, w)[None]
        cases.append((f"noisy-{h}x{w}", g[0], g[1], 0, {}))
        cases.append((f"plane-{h}x{w}-pad4", np.stack([plane(h, w, k1[0], CAM_HEIGHT), plane(h, w, k1[0], 0.7)])[:, None], rep(k1, 2), 4, dict(ties=True)))
    cases.append(("count1-5x9", few_ground_pixels(orc32, orc64, 5, 9, 1)[None, None], pinhole(5, 9)[None], 0, dict(count=1)))
    cases.append(("count2-5x9-pad3", few_ground_pixels(orc32, orc64, 5, 9, 2)[None, None], pinhole(5, 9)[None], 3, dict(count=2)))
    g = make_ground(192, 640, 2)
    cases.append(("noisy-192x640", g[0], g[1], 0, {}))
    cases.append(("noisy-192x640-pad3", g[0], g[1], 3, {}))
    return [(name, np.ascontiguousarray(d, np.float32), np.ascontiguousarray(K, np.float32), pad, ex) for name, d, K, pad, ex in cases]


def check_median_structure(name, heights, masks, pad, expect):
    """the masked heights [N,H,W] of a case have the structure its name claims -> (median, count with padding)"""
    _, count0, v0 = lower_median(heights, masks, 0)
    med, count, v = lower_median(heights, masks, pad)
    if "count" in expect:
        assert count0 == expect["count"], (name, count0, expect)
    if expect.get("ties"):
        assert count0 >= 8 and np.unique(v0).size <= count0 // 4, (name, count0, np.unique(v0).size)
        assert (v == med).sum() >= 2, (name, "the median itself is a tied value")
    bits = v0.view(np.uint32)
    if expect.get("byte") == "low":
        assert np.unique(bits >> 8).size == 1 and np.unique(bits & 0xFF).size >= 2, (name, np.unique(bits))
    if expect.get("byte") == "high":
        assert np.unique(bits & 0xFFFFFF).size == 1 and np.unique(bits >> 24).size == count0, (name, np.unique(bits))
    return med, count
