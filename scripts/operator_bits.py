#!/usr/bin/env python3
"""Run every operator, evaluation and frame-preparation entry of the C ABI at three tiny shapes and print a SHA-256 of each output: two
builds whose lines agree compute the same bits.
    python scripts/operator_bits.py > bits.txt
Shapes: 5 x 7 (hw & 3 == 3, one block), 17 x 33 (partial tiles both ways, hw & 3 == 1, three blocks), 37 x 53.  Every entry runs on
device pointers at every shape and (where it takes them) with host_ptrs = 1 at 17 x 33.  At 17 x 33 the three backward entries run
over every NULL / wanted combination their plan (csrc/operator_plan.h) distinguishes and the window loss over every combination of
argmin, automask and the inverse direction at S = 1, 2, 4; the other shapes and the host run take every S with all switches on and
with argmin and the inverse direction off, and the backward entries with every cotangent given and without g_proj_depth.  Everywhere:
disp_to_depth_backward also on a pointer offset by one float (the scalar path), scale_recovery with and without pad_to_batch and the
optional maps, and its _frames form.  One line per call, a SHA-256 per output.  The calls go through the raw ABI so that a NULL is a NULL."""
import ctypes as C
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tightly_coupled_sfm_amd import _lib, synth
from tightly_coupled_sfm_amd.engine import Engine

MAX_PAIRS, N = 16, 2
f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Out:
    """an output array of the call: name, shape, dtype; host: written on the host in every mode (the float64 results)"""
    def __init__(self, name, shape, dtype=np.float32, host=False):
        self.name, self.shape, self.dtype, self.host = name, shape, dtype, host


class Runner:
    def __init__(self, H, W, host):
        self.H, self.W, self.host = H, W, host
        self.e = Engine(H, W, MAX_PAIRS)
        self.e._bind()
        self.lib = self.e.lib
        self.tag = f"{H}x{W} {'host' if host else 'dev'}"

    def call(self, label, entry, opts, *args, offset=0):
        """args: scalars pass through; a numpy array is an input; an Out an output; None a NULL.  offset: floats every device array is
        shifted by inside a larger allocation"""
        o = _lib.default_opts(**opts)
        o.host_ptrs = 1 if self.host else 0
        keep, outs, cargs = [], [], []
        for a in args:
            if isinstance(a, Out):
                buf = np.zeros(a.shape, a.dtype)
                if self.host or a.host:
                    keep.append(buf); cargs.append(buf.ctypes.data); outs.append((a, buf))
                else:
                    t = torch.zeros(buf.size + offset, dtype=getattr(torch, buf.dtype.name), device="cuda")[offset:]
                    keep.append(t); cargs.append(t.data_ptr()); outs.append((a, t))
            elif isinstance(a, np.ndarray):
                if self.host:
                    keep.append(a); cargs.append(a.ctypes.data)
                else:
                    t = torch.zeros(a.size + offset, dtype=getattr(torch, a.dtype.name), device="cuda")
                    t[offset:] = torch.from_numpy(a.reshape(-1))
                    keep.append(t); cargs.append(t[offset:].data_ptr())
            else:
                cargs.append(a)
        torch.cuda.synchronize()
        rc = getattr(self.lib, entry)(self.e._h, C.byref(o), *cargs)
        rc = rc or self.lib.tcsfm_synchronize(self.e._h)
        torch.cuda.synchronize()
        if rc:
            print(f"{self.tag} {entry} {label} rc {rc} {self.lib.tcsfm_last_error(self.e._h).decode()}")
            return {}
        res, line = {}, []
        for a, buf in outs:
            v = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
            res[a.name] = v.reshape(a.shape)
            line.append(f"{a.name} {sha(v)}")
        print(f"{self.tag} {entry} {label}: {' '.join(line)}")
        return res


def window(H, W, S, nb, seed=3):
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(nb):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0, -1.0, 1.6, -1.6)[s]
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    return (f32(np.stack(tg)), f32(np.stack([np.stack(x) for x in sr])), f32(np.stack(dt)[:, None]), f32(np.stack([np.stack(x) for x in ds])[:, :, None]), f32(np.stack(K)),
            f32(np.concatenate([fwd, -fwd])))


def bits(n):
    return list(itertools.product((0, 1), repeat=n))


def run_shape(H, W, host, full):
    """full: every combination; otherwise the combinations that take another launch or grid at this shape"""
    r = Runner(H, W, host)
    rng = np.random.default_rng(H * 1000 + W)
    hw = H * W
    u = lambda *s, lo=0.0, hi=1.0: f32(rng.uniform(lo, hi, size=s))
    g = lambda *s: f32(rng.normal(size=s))
    b = synth.make_batch(N, H, W, seed0=5, both_directions=True)
    tgt, src, dt, ds, K, pose = (f32(b[k]) for k in ("tgt", "src", "depth_t", "depth_s", "K", "pose_init"))
    m1, m3 = (N, 1, H, W), (N, 3, H, W)

    # -- per-plane operators
    n = N * hw
    disp = u(n, lo=0.05, hi=0.95)
    r.call("", "tcsfm_disp_to_depth", {}, n, disp, Out("scaled_disp", (n,)), Out("depth", (n,)))
    gs, gd = g(n), g(n)
    for label, a, c in (("both", gs, gd), ("g_scaled", gs, None), ("g_depth", None, gd)):
        r.call(label, "tcsfm_disp_to_depth_backward", {}, n, disp, a, c, Out("g_disp", (n,)))
    if not host:          # a pointer offset by one float: no 16-byte alignment, the scalar path takes every element
        r.call("offset by one float", "tcsfm_disp_to_depth_backward", {}, n, disp, gs, gd, Out("g_disp", (n,)), offset=1)
    x, y, go = u(3 * N, H, W), u(3 * N, H, W), g(3 * N, H, W)
    r.call("", "tcsfm_ssim", {}, 3 * N, x, y, Out("out", (3 * N, H, W)))
    for wx, wy in ((1, 1), (1, 0), (0, 1)):
        r.call(f"want {wx}{wy}", "tcsfm_ssim_backward", {}, 3 * N, x, y, go, Out("g_x", (3 * N, H, W)) if wx else None, Out("g_y", (3 * N, H, W)) if wy else None)
    sdisp, img = u(*m1, lo=0.05, hi=0.95), u(*m3)
    r.call("", "tcsfm_smooth_loss", {}, N, sdisp, img, Out("loss_out", (1,), np.float64, host=True))
    st = r.call("", "tcsfm_smooth_loss_device", {}, N, sdisp, img, Out("loss_out", (1,)), Out("stats_out", (N, 3), np.float64))
    if st:
        r.call("", "tcsfm_smooth_loss_backward", {}, N, sdisp, img, st["stats_out"], f32([1.25]), Out("g_disp", m1))

    # -- the window loss and its backward
    for S in (1, 2, 4):
        Bw = 2
        m = (S * Bw, 1, H, W)
        maps = [u(*m), f32(rng.uniform(size=m) > 0.3), u(*m, lo=0.2), u(*m), u(*m), f32(rng.uniform(size=m) > 0.3), u(*m, lo=0.2), f32(rng.uniform(size=m) > 0.3)]
        for argmin, automask, inverse in (bits(3) if full else ((1, 1, 1), (0, 1, 0))):
            label = f"S={S} argmin={argmin} automask={automask} inverse={inverse}"
            o = dict(w_dc=0.15, automask=automask)
            st = r.call(label, "tcsfm_window_loss", o, Bw, S, argmin, inverse, *maps, Out("loss_out", (1,)), Out("stats_out", (7,), np.float64))
            if st:
                r.call(label, "tcsfm_window_loss_backward", o, Bw, S, argmin, inverse, *maps, st["stats_out"], f32([0.75]),
                       Out("g_fwd_diff", m), Out("g_fwd_weight", m), Out("g_inv_diff", m) if inverse else None, Out("g_inv_weight", m) if inverse else None)

    # -- warp, photometric
    w = r.call("", "tcsfm_warp", {}, N, src, dt, ds, pose, K, Out("img_rec", m3), Out("valid", m1), Out("proj_depth", m1), Out("comp_depth", m1))
    r.call("", "tcsfm_warp_posenet_input", {}, N, tgt, src, dt, ds, pose, K, Out("posenet_in", (N, 6, H, W)), Out("valid", m1))
    for am in (0, 1):
        r.call(f"automask={am}", "tcsfm_photometric", dict(automask=am), N, tgt, src, dt, ds, pose, K,
               *(Out(k, m1) for k in ("diff", "valid", "weight", "auto_err", "auto_mask")), Out("img_rec", m3))
    g_rec, g_pd, g_cd, g_diff, g_weight = g(*m3), g(*m1), g(*m1), g(*m1), g(*m1)
    # warp backward: g_proj_depth x the three outputs (g_rec and g_comp_depth change no decision: given, and once absent)
    for gpd, wdt, wds, wp in bits(4):
        if (wdt or wds or wp) and (full or wdt + wds + wp == 3):
            r.call(f"g_pd={gpd} want={wdt}{wds}{wp}", "tcsfm_warp_backward", {}, N, src, dt, ds, pose, K, g_rec, g_pd if gpd else None, g_cd,
                   Out("d_depth_t", m1) if wdt else None, Out("d_depth_s", m1) if wds else None, Out("d_pose", (N, 6)) if wp else None)
    r.call("g_pd only", "tcsfm_warp_backward", {}, N, src, dt, ds, pose, K, None, g_pd, None, Out("d_depth_t", m1), Out("d_depth_s", m1), Out("d_pose", (N, 6)))
    if w:
        for gdf, gw, wr, wpd, wcd in bits(5):
            if (wr or wpd or wcd) and (full or (gdf and gw and wr + wpd + wcd == 3)):
                r.call(f"g={gdf}{gw} want={wr}{wpd}{wcd}", "tcsfm_photometric_maps_backward", {}, N, tgt, w["img_rec"], w["proj_depth"], w["comp_depth"],
                       g_diff if gdf else None, g_weight if gw else None, Out("g_rec", m3) if wr else None, Out("g_proj_depth", m1) if wpd else None,
                       Out("g_comp_depth", m1) if wcd else None)
    for gdf, gw, gi in (bits(3) if full else ((1, 1, 1),)):      # (which outputs are wanted decides in the warp's backward alone: above)
        for want in ((1, 1, 1), (0, 1, 0)):
            r.call(f"g={gdf}{gw}{gi} want={''.join(map(str, want))}", "tcsfm_photometric_backward", {}, N, tgt, src, dt, ds, pose, K,
                   g_diff if gdf else None, g_weight if gw else None, g_rec if gi else None,
                   Out("d_depth_t", m1) if want[0] else None, Out("d_depth_s", m1) if want[1] else None, Out("d_pose", (N, 6)) if want[2] else None)

    # -- evaluation entries
    ls = f32(np.linspace(-0.03, 0.02, N))
    for refine, w_dc in ((0, 0.0), (0, 0.15), (1, 0.15)):
        np_ = 7 if refine else 6
        r.call(f"refine={refine} w_dc={w_dc}", "tcsfm_linearize", dict(refine=refine, w_dc=w_dc), N, tgt, src, dt, ds, pose, ls if refine else None, K,
               Out("Hmat", (N, np_, np_), np.float64, host=True), Out("g", (N, np_), np.float64, host=True), Out("stats", (N, 4), np.float64, host=True))
    poses = f32(pose[:1] + np.linspace(-0.01, 0.01, 5)[:, None] * np.float32([1, 0, 0, 0, 0.5, 0]))
    r.call("", "tcsfm_loss_surface", dict(w_dc=0.15), tgt[0], src[0], dt[0], ds[0], K[0], 5, poses, Out("cost_out", (5,), np.float64, host=True))
    for S in (1, 2):
        Bw = 2
        Nw = 2 * Bw * S
        wt, ws, wdt, wds, wK, wp = window(H, W, S, Bw)
        lsw = f32(np.linspace(-0.03, 0.02, Nw))
        for refine, argmin, rule in ((0, 1, 0), (1, 1, 0), (0, 0, 1)):
            np_ = 7 if refine else 6
            r.call(f"S={S} refine={refine} argmin={argmin} rule={rule}", "tcsfm_linearize_window", dict(refine=refine, argmin=argmin, window_rule=rule, w_dc=0.15), Bw, S,
                   wt, ws, wdt, wds, wK, wp, lsw if refine else None, Out("Hmat", (Nw, np_, np_), np.float64, host=True), Out("g", (Nw, np_), np.float64, host=True),
                   Out("stats", (Nw, 4), np.float64, host=True))
        o = dict(window_rule=1, w_dc=0.15, argmin=1)
        d0 = f32(wdt * 0.97)
        tail = [Out("scal_out", (8,), np.float64, host=True), Out("g_pose_out", (Nw, 6), np.float64, host=True), Out("g_rho_out", (Bw, hw))]
        r.call(f"S={S}", "tcsfm_linearize_dense_window", o, Bw, S, wt, ws, wdt, wds, wK, wp, d0, *tail)
        r.call(f"S={S} no depth0", "tcsfm_linearize_dense_window", o, Bw, S, wt, ws, wdt, wds, wK, wp, None, *tail)
        r.call(f"S={S}", "tcsfm_linearize_dense_window_sources", o, Bw, S, wt, ws, wdt, wds, wK, wp, d0, *tail, Out("g_rho_src_out", (S, Bw, hw)))

    # -- scale recovery
    for pad, maps in ((0, 0), (4, 0), (0, 1), (4, 1)):
        r.call(f"pad_to_batch={pad} maps={maps}", "tcsfm_scale_recovery", {}, N, dt, K, C.c_float(1.65), pad, Out("scale_out", (1,)), Out("median_out", (1,)),
               Out("height_out", m1) if maps else None, Out("mask_out", m1) if maps else None)
    if not host:
        r.call("", "tcsfm_scale_recovery_frames", {}, N, dt, K, C.c_float(1.65), Out("scale_out", (N,)), Out("median_out", (N,)), Out("count_out", (N,), np.int32))
        r.call("no median, no count", "tcsfm_scale_recovery_frames", {}, N, dt, K, C.c_float(1.65), Out("scale_out", (N,)), None, None)

    # -- frame preparation (device pointers only; the host forms take no handle)
    if not host:
        r.call("", "tcsfm_disp_post_process", {}, N, u(N, H, W), u(N, H, W), Out("out", (N, H, W), np.float64))
        r.call("offset by one float", "tcsfm_disp_post_process", {}, N, u(N, H, W), u(N, H, W), Out("out", (N, H, W), np.float64), offset=1)
        u8 = np.ascontiguousarray(rng.integers(0, 256, size=(N, 3, H, W), dtype=np.uint8))
        for fmt, fname in ((_lib.FRAMES_U8_CHW, "chw"), (_lib.FRAMES_U8_HWC, "hwc")):
            r.call(fname, "tcsfm_frames_from_u8", {}, fmt, N, u8, Out("dst", m3))
            for sh, sw in ((2 * H + 1, 2 * W + 3), (H, W), (3 * H, W + 5)):
                big = np.ascontiguousarray(rng.integers(0, 256, size=(N, 3 * sh * sw), dtype=np.uint8))
                r.call(f"{fname} {sh}x{sw} f32", "tcsfm_resize_u8", {}, fmt, N, sh, sw, big, _lib.FRAMES_F32_CHW, Out("dst", m3))
                r.call(f"{fname} {sh}x{sw} u8", "tcsfm_resize_u8", {}, fmt, N, sh, sw, big, fmt, Out("dst", m3, np.uint8))
        print(f"{r.tag} tcsfm_flip_ramp l_mask {sha(r.e.flip_ramp())}")
        print(f"{r.tag} tcsfm_scale_intrinsics K {sha(r.e.scale_intrinsics(K[0], (2 * H + 1, 2 * W + 3)))}")
        for a, c in ((2 * W + 3, W), (W, W), (W, 2 * W)):
            ks, bounds, kk = C.c_int(0), np.zeros(2 * c, np.int32), np.zeros(c * 64, np.int32)
            rc = r.lib.tcsfm_resize_coeffs(a, c, C.byref(ks), bounds.ctypes.data, kk.ctypes.data)
            print(f"{r.tag} tcsfm_resize_coeffs {a}->{c} rc {rc} ksize {ks.value} bounds {sha(bounds)} kk {sha(kk[:c * max(ks.value, 0)])}")
    r.e.close()


def main():
    for H, W in ((5, 7), (17, 33), (37, 53)):
        run_shape(H, W, False, full=(H, W) == (17, 33))
    run_shape(17, 33, True, full=False)


if __name__ == "__main__":
    main()
