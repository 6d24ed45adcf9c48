"""References, cotangents, the judge and planted faults of the PoseNet input-gradient tests (tests/test_posenet_grad_inputs_cpu.py,
tests/test_gpu_posenet_grad.py).  No GPU in here.

REFERENCE: standins.PoseNetTwin(...).double() stepped layer by layer with the ReLU decisions SUPPLIED by the caller
(forward_pinned): a_l = GroupNorm(z_l) * mask_l.  Pinned to the decisions the library took (act_out > 0 of
tcsfm_debug_posenet_tape_layer) the float64 gradient is the gradient of the very piecewise-linear function the library
differentiated; an activation that sits within an ulp of zero cannot turn a rounding difference into a whole term.

YARDSTICK: the same pinned twin in float32 (CPU torch autograd).

JUDGE: relative L2 and max error / RMS of the reference, each <= max(floor, posenet_layers.MARGIN x the yardstick's own figure), the
floors posenet_layers.FLOOR_REL_L2 / FLOOR_MAX_RMS -- the project's operator rule, not a measurement of the code under test.

COTANGENTS are exact in fp32 (multiples of 1/8 in [-1, 1]; one-hot).

PLANTED FAULTS (backward_manual, a float64 restatement of the backward's formulas at torch level; without a fault it reproduces
autograd): the S1 term dropped, the S2 term dropped, layer l's mask taken from layer l - 1 (its stride-2 subsample, channels wrapped;
layer 1: no mask), the transposed convolution's result shifted by one pixel, 0.01 / npix missing, 1 / 0.22 missing.
"""
import numpy as np
import torch
import torch.nn.functional as F

import posenet_layers as PL
import standins

# (H, W, N, max_images)
CASES = [(5, 9, 1, 1), (17, 33, 2, 2), (17, 33, 5, 5), (37, 53, 4, 4), (37, 53, 7, 12), (64, 64, 5, 5), (192, 640, 2, 2)]
CASE_IDS = [f"{H}x{W}-N{N}of{M}" for H, W, N, M in CASES]
FAULTS = ["no_s1", "no_s2", "mask_prev", "shifted", "no_head_scale", "no_input_scale"]
C045 = float(np.float32(0.45))


def constant_frames(H, W, N):
    """every pixel 0.45f: the normalised image is exactly zero, layer 1's groups (one channel each) have zero variance, rstd = 316"""
    return torch.full((N, 6, H, W), C045, dtype=torch.float32)


def cotangent_dense(N, seed):
    rng = np.random.default_rng(4200 + seed)
    return torch.tensor(rng.integers(-8, 9, size=(N, 6)).astype(np.float32) / 8.0)


def cotangent_onehot(N, n, j):
    d = torch.zeros((N, 6), dtype=torch.float32)
    d[n, j] = 1.0
    return d


def _normalised(imgs, dtype):
    return PL.operand64(1, imgs) if dtype == torch.float64 else (imgs.to(dtype) - 0.45) / 0.22


def forward_pinned(sd, imgs, masks=None, dtype=torch.float64):
    """PoseNetTwin in `dtype`, layer by layer, ReLU replaced by the multiplication with masks[l] (bool [N,C,h,w]); masks None: the
    twin's own decisions.  Differentiable with respect to imgs.  -> (pose [N,6], the masks used)"""
    net = standins.PoseNetTwin(sd).to(dtype).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    x = _normalised(imgs, dtype)
    used = []
    for i in range(7):
        seq = getattr(net, f"conv{i + 1}")
        y = seq[1](seq[0](x))
        m = (y > 0) if masks is None else masks[i]
        used.append(m.detach())
        x = y * m.to(dtype)
    return 0.01 * net.pose_pred(x).mean(3).mean(2).view(-1, 6), used


def grad_pinned(sd, imgs, masks, d_pose, dtype=torch.float64):
    """d_imgs [N,6,H,W] in `dtype`: autograd through forward_pinned"""
    x = imgs.clone().to(dtype).requires_grad_(True)
    pose, _ = forward_pinned(sd, x, masks, dtype)
    g, = torch.autograd.grad(pose, x, d_pose.to(dtype))
    return g


def grad_plain64(sd, imgs, d_pose):
    """plain float64 autograd of PoseNetTwin (its own ReLU)"""
    net = standins.PoseNetTwin(sd).double().eval()
    # the twin subtracts the double 0.45 where forward_pinned subtracts 0.45f (posenet_layers.operand64): hand it the same operand
    x = (imgs.double() + (0.45 - C045)).requires_grad_(True)
    g, = torch.autograd.grad(net(x), x, d_pose.double())
    return g


def backward_manual(sd, imgs, masks, d_pose, fault=None):
    """the backward's formulas in float64 at torch level (module docstring); fault: None or one of FAULTS"""
    assert fault is None or fault in FAULTS
    with torch.no_grad():
        a = PL.operand64(1, imgs)
        N = a.shape[0]
        tape = []
        for l in range(1, 8):
            w = PL.ws64(sd[f"conv{l}.0.weight"])
            k = w.shape[-1]
            z = F.conv2d(a, w, torch.as_tensor(sd[f"conv{l}.0.bias"]).double(), 2, (k - 1) // 2)
            zg = z.reshape(N, 16, -1)
            mean, var = zg.mean(2, keepdim=True), zg.var(2, unbiased=False, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + PL.EPS)
            xh = ((zg - mean) * rstd).reshape(z.shape)
            gam = torch.as_tensor(sd[f"conv{l}.1.weight"]).double().view(1, -1, 1, 1)
            bet = torch.as_tensor(sd[f"conv{l}.1.bias"]).double().view(1, -1, 1, 1)
            tape.append((w, a.shape, xh, rstd, gam))
            a = (xh * gam + bet) * masks[l - 1].double()
        h7, w7 = a.shape[2:]
        wh = torch.as_tensor(sd["pose_pred.weight"]).double().reshape(6, 256)
        scale = 1.0 if fault == "no_head_scale" else 0.01 / (h7 * w7)
        da = (scale * (d_pose.double() @ wh))[:, :, None, None].expand(N, 256, h7, w7)
        for l in range(7, 0, -1):
            w, ishape, xh, rstd, gam = tape[l - 1]
            m = masks[l - 1]
            if fault == "mask_prev":
                if l == 1:
                    m = torch.ones_like(m)
                else:
                    p = masks[l - 2][:, :, ::2, ::2]
                    ci = torch.arange(m.shape[1]) % p.shape[1]
                    m = p[:, ci][:, :, :m.shape[2], :m.shape[3]]
            t = gam * (da * m.double())
            tg, xg = t.reshape(N, 16, -1), xh.reshape(N, 16, -1)
            s1 = tg.mean(2, keepdim=True) * (0.0 if fault == "no_s1" else 1.0)
            s2 = (tg * xg).mean(2, keepdim=True) * (0.0 if fault == "no_s2" else 1.0)
            dz = (rstd * (tg - s1 - xg * s2)).reshape(t.shape)
            k, pad = w.shape[-1], (w.shape[-1] - 1) // 2
            op = tuple(ishape[2 + d] - ((dz.shape[2 + d] - 1) * 2 - 2 * pad + k) for d in range(2))
            da = F.conv_transpose2d(dz, w, None, 2, pad, op)
            if fault == "shifted":
                da = F.pad(da, (1, 0))[:, :, :, :-1]
        return da * (1.0 if fault == "no_input_scale" else 1.0 / 0.22)


def figures(got, ref):
    return PL.rel_l2(got, ref), PL.max_over_rms(got, ref)


def judge(got, ref64, yard32):
    """-> (ok, dict of figures): both figures of `got` within max(floor, MARGIN x the float32 yardstick's)"""
    e, y = figures(got, ref64), figures(yard32, ref64)
    bounds = (PL.hold(PL.FLOOR_REL_L2, y[0]), PL.hold(PL.FLOOR_MAX_RMS, y[1]))
    ok = bool(torch.isfinite(torch.as_tensor(got)).all()) and e[0] <= bounds[0] and e[1] <= bounds[1]
    return ok, dict(rel_l2=e[0], max_rms=e[1], f32_rel_l2=y[0], f32_max_rms=y[1], bound_rel_l2=bounds[0], bound_max_rms=bounds[1],
                    ratio_rel_l2=e[0] / y[0] if y[0] > 0 else float("nan"), ratio_max_rms=e[1] / y[1] if y[1] > 0 else float("nan"))
