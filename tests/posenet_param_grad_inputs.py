"""References, the judge and planted faults of the PoseNet parameter-gradient tests (tests/test_posenet_param_grad_inputs_cpu.py,
tests/test_gpu_posenet_param_grad.py, tests/test_gpu_pose_loop_param_grad.py).  No GPU in here.

REFERENCE: standins.PoseNetTwin(...).double() with its parameters requiring grad, stepped layer by layer with the ReLU decisions
SUPPLIED by the caller (posenet_grad_inputs' pinning: a_l = GroupNorm(z_l) * mask_l), so that the float64 gradient is the gradient of
the very piecewise-linear function the library differentiated.  YARDSTICK: the same pinned twin in float32.  JUDGE, per parameter
tensor: posenet_grad_inputs.judge -- relative L2 and max error / RMS within max(floor, MARGIN x the yardstick's own figure).

conv1.0.bias is DEGENERATE: layer 1 has one channel per GroupNorm group, the group mean removes any per-channel constant and the
gradient is identically zero (float64 gives 1e-19); a relative figure means nothing.  It is judged by a derived bound,
    |g_c| <= n u D_c,   n = N oh ow,  u = 2^-24,  D_c = sum_{n,p} rstd (|t| + |s1| + |x^ s2|)   (from the float64 twin),
the standard any-order bound of a sum of n terms whose cancellation-free magnitude is D_c (Higham, 4.2): dz = rstd (t - s1 - x^ s2).

PLANTED FAULTS (param_backward_manual, a float64 restatement of the backward's parameter formulas at torch level; without a fault it
reproduces autograd): see FAULTS; FAULT_TENSORS names, per fault, the tensors on which the judge must fail at every shape.
"""
import numpy as np
import torch
import torch.nn.functional as F

import posenet_grad_inputs as GI
import posenet_layers as PL
import standins

NAMES = [f"conv{l}.{k}" for l in range(1, 8) for k in ("0.weight", "0.bias", "1.weight", "1.bias")] + ["pose_pred.weight", "pose_pred.bias"]
DEGENERATE = "conv1.0.bias"
# (H, W, N, max_images)
CASES = [(5, 9, 1, 1), (17, 33, 2, 2), (17, 33, 5, 5), (37, 53, 7, 12), (64, 64, 5, 5), (96, 100, 2, 2), (192, 640, 2, 2)]
CASE_IDS = [f"{H}x{W}-N{N}of{M}" for H, W, N, M in CASES]
CPU_SHAPES = [(5, 9, 1), (17, 33, 2), (37, 53, 2), (64, 64, 2), (96, 100, 2)]

FAULTS = ["no_gmean", "no_gw_term", "n_for_nm1", "no_eps", "unmasked_affine", "bias_from_t", "prerelu_input", "kykx_swapped", "no_head_scale"]
_W = lambda ls: [f"conv{l}.0.weight" for l in ls]
FAULT_TENSORS = {
    "no_gmean": _W(range(1, 8)),                     # the mean(G^) term dropped
    "no_gw_term": _W(range(2, 8)),                   # the w^ sum(G^ w^) term dropped; layer 1 is scale-invariant per channel and cannot see it
    "n_for_nm1": _W(range(2, 5)),                    # n for n - 1; under the margin on layers 6-7
    "no_eps": _W(range(1, 8)),                       # 1e-5 dropped from s + 1e-5
    "unmasked_affine": [f"conv{l}.1.{k}" for l in range(1, 8) for k in ("weight", "bias")],
    "bias_from_t": [f"conv{l}.0.bias" for l in range(2, 8)],
    "prerelu_input": _W(range(2, 8)),
    "kykx_swapped": _W(range(1, 5)),                 # at 5 x 9 layers 5..7 read a 1 x 1 map: only the centre tap sees data, a transpose is invisible
    "no_head_scale": ["pose_pred.weight"],
}


def _pinned_net(sd, dtype):
    net = standins.PoseNetTwin(sd).to(dtype).eval()
    for p in net.parameters():
        p.requires_grad_(True)
    return net


def forward_pinned_net(net, imgs, masks, dtype, keep=None):
    """net (a PoseNetTwin in `dtype`, parameters as they are) layer by layer with ReLU replaced by masks[l]; keep: a list that
    receives layer 1's masked activation"""
    x = GI._normalised(imgs, dtype)
    used = []
    for i in range(7):
        seq = getattr(net, f"conv{i + 1}")
        y = seq[1](seq[0](x))
        m = (y > 0) if masks is None else masks[i]
        used.append(m.detach())
        x = y * m.to(dtype)
        if i == 0 and keep is not None:
            keep.append(x)
    return 0.01 * net.pose_pred(x).mean(3).mean(2).view(-1, 6), used


def param_grads_pinned(sd, imgs, masks, d_pose, dtype=torch.float64, with_imgs=False):
    """{name: gradient in `dtype`} (+ 'imgs' when with_imgs): autograd through the pinned twin, parameters requiring grad.
    -> (grads, masks used)"""
    net = _pinned_net(sd, dtype)
    x = imgs.clone().to(dtype).requires_grad_(with_imgs)
    pose, used = forward_pinned_net(net, x, masks, dtype)
    named = dict(net.named_parameters())
    leaves = [named[k] for k in NAMES] + ([x] if with_imgs else [])
    gs = torch.autograd.grad(pose, leaves, d_pose.to(dtype))
    out = {k: g for k, g in zip(NAMES, gs)}
    if with_imgs:
        out["imgs"] = gs[-1]
    return out, used


def conv1_bias_bound(sd, imgs, masks, d_pose):
    """[16] float64: n u D_c of the module docstring, from the float64 twin"""
    net = _pinned_net(sd, torch.float64)
    keep = []
    pose, _ = forward_pinned_net(net, imgs, masks, torch.float64, keep)
    da, = torch.autograd.grad(pose, keep[0], d_pose.double())
    with torch.no_grad():
        z = net.conv1[0](PL.operand64(1, imgs))
        N = z.shape[0]
        zg = z.reshape(N, 16, -1)
        mean, var = zg.mean(2, keepdim=True), zg.var(2, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + PL.EPS)
        xh = (zg - mean) * rstd
        t = (net.conv1[1].weight.view(1, 16, 1, 1) * da * masks[0].double()).reshape(N, 16, -1)
        s1, s2 = t.mean(2, keepdim=True), (t * xh).mean(2, keepdim=True)
        D = (rstd * (t.abs() + s1.abs() + (xh * s2).abs())).sum(dim=(0, 2))
        return N * zg.shape[2] * PL.U * D


def param_backward_manual(sd, imgs, masks, d_pose, fault=None):
    """the backward's parameter formulas in float64 at torch level (module docstring) -> {name: gradient}"""
    assert fault is None or fault in FAULTS
    out = {}
    with torch.no_grad():
        a = PL.operand64(1, imgs)
        N = a.shape[0]
        tape, pre = [], None
        for l in range(1, 8):
            w = torch.as_tensor(sd[f"conv{l}.0.weight"]).double()
            n = w[0].numel()
            m = w.mean(dim=(1, 2, 3), keepdim=True)
            s = w.flatten(1).std(dim=1).view(-1, 1, 1, 1)
            wh = (w - m) / (s + 1e-5)
            k = w.shape[-1]
            z = F.conv2d(a, wh, torch.as_tensor(sd[f"conv{l}.0.bias"]).double(), 2, (k - 1) // 2)
            zg = z.reshape(N, 16, -1)
            mean, var = zg.mean(2, keepdim=True), zg.var(2, unbiased=False, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + PL.EPS)
            xh = ((zg - mean) * rstd).reshape(z.shape)
            gam = torch.as_tensor(sd[f"conv{l}.1.weight"]).double().view(1, -1, 1, 1)
            bet = torch.as_tensor(sd[f"conv{l}.1.bias"]).double().view(1, -1, 1, 1)
            tape.append((wh, s, n, a, pre, xh, rstd, gam))
            pre = xh * gam + bet
            a = pre * masks[l - 1].double()
        h7, w7 = a.shape[2:]
        whd = torch.as_tensor(sd["pose_pred.weight"]).double().reshape(6, 256)
        d = d_pose.double()
        scale = 1.0 if fault == "no_head_scale" else 0.01 / (h7 * w7)
        out["pose_pred.weight"] = (scale * (d.t() @ a.sum(dim=(2, 3)))).reshape(6, 256, 1, 1)
        out["pose_pred.bias"] = 0.01 * d.sum(0)
        da = ((0.01 / (h7 * w7)) * (d @ whd))[:, :, None, None].expand(N, 256, h7, w7)
        for l in range(7, 0, -1):
            wh, s, n, a_in, pre_in, xh, rstd, gam = tape[l - 1]
            g = da * masks[l - 1].double()
            ga = da if fault == "unmasked_affine" else g
            out[f"conv{l}.1.bias"] = ga.sum(dim=(0, 2, 3))
            out[f"conv{l}.1.weight"] = (ga * xh).sum(dim=(0, 2, 3))
            t = gam * g
            tg, xg = t.reshape(N, 16, -1), xh.reshape(N, 16, -1)
            s1, s2 = tg.mean(2, keepdim=True), (tg * xg).mean(2, keepdim=True)
            dz = (rstd * (tg - s1 - xg * s2)).reshape(t.shape)
            out[f"conv{l}.0.bias"] = (t if fault == "bias_from_t" else dz).sum(dim=(0, 2, 3))
            k, pad = wh.shape[-1], (wh.shape[-1] - 1) // 2
            x_in = pre_in if (fault == "prerelu_input" and l > 1) else a_in
            G = torch.nn.grad.conv2d_weight(x_in, wh.shape, dz, stride=2, padding=pad)
            if fault == "kykx_swapped":
                G = G.transpose(2, 3)
            gm = 0.0 if fault == "no_gmean" else G.mean(dim=(1, 2, 3), keepdim=True)
            gw = 0.0 if fault == "no_gw_term" else (G * wh).sum(dim=(1, 2, 3), keepdim=True)
            den = s if fault == "no_eps" else s + 1e-5
            out[f"conv{l}.0.weight"] = (G - gm) / den - wh * gw / ((n if fault == "n_for_nm1" else n - 1) * s)
            op = tuple(a_in.shape[2 + q] - ((dz.shape[2 + q] - 1) * 2 - 2 * pad + k) for q in range(2))
            da = F.conv_transpose2d(dz, wh, None, 2, pad, op)
    return out


def judge_all(got, ref64, yard32, bias_bound, skip=()):
    """-> (names that fail, {name: figures}); conv1.0.bias against bias_bound [16] (None: left out), every other tensor under
    GI.judge; skip: names left out"""
    bad, figs = [], {}
    for k in NAMES:
        if k in skip or (k == DEGENERATE and bias_bound is None):
            continue
        g = torch.as_tensor(got[k]).detach().cpu().reshape(ref64[k].shape)
        if k == DEGENERATE:
            r = (g.double().abs() / bias_bound.clamp_min(1e-300)).max()
            ok = bool(torch.isfinite(g).all()) and float(r) <= 1.0
            figs[k] = dict(worst_over_bound=float(r))
        else:
            ok, figs[k] = GI.judge(g, ref64[k], yard32[k])
        if not ok:
            bad.append(k)
    return bad, figs


def worst(figs):
    """(largest rel-L2 ratio, its tensor, largest max/RMS ratio, its tensor, largest rel L2) over the judged tensors whose bound is the
    yardstick's (the floor-governed ones are left out of the ratio)"""
    rows = [(k, f) for k, f in figs.items() if k != DEGENERATE]
    r1 = max(((f["rel_l2"] / f["bound_rel_l2"], k) for k, f in rows))
    r2 = max(((f["max_rms"] / f["bound_max_rms"], k) for k, f in rows))
    return r1, r2, max(f["rel_l2"] for _, f in rows)


def twin_loop_params(inp, dtype, masks, depth_leaves):
    """pose_loop_grad_inputs.twin_loop with the PoseNet's parameters requiring grad (every call of the loop, the first included,
    under autograd) -> dict: stacked [N, NUM_ITER, 6] (float64 numpy) and {name: gradient of sum R * stacked} (+ d_disp_t, d_disp_s
    when depth_leaves).  masks: per call the seven ReLU masks"""
    import pose_loop_grad_inputs as LI
    from oracle import torch_twin as tw
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    net = _pinned_net(LI.params(), dtype)
    S, B = inp["srcs"].shape[:2]
    split = S * B
    lo, hi = LI._scales()
    disp_t, disp_s = T(inp["disp_t"]).requires_grad_(depth_leaves), T(inp["disp_s"]).requires_grad_(depth_leaves)
    depth_t, depth_s = 1 / (lo + (hi - lo) * disp_t), 1 / (lo + (hi - lo) * disp_s)
    td, sdp = depth_t.repeat(S, 1, 1, 1), depth_s.reshape(split, 1, LI.H, LI.W)
    ti, si = T(inp["tgt"]).repeat(S, 1, 1, 1), T(inp["srcs"]).reshape(split, 3, LI.H, LI.W)
    tgt, src = torch.cat([ti, si], 0), torch.cat([si, ti], 0)
    d_t, d_s = torch.cat([td, sdp], 0), torch.cat([sdp, td], 0)
    K = T(inp["K"]).repeat(2 * S, 1, 1)
    p, _ = forward_pinned_net(net, torch.cat([tgt, src], 1), masks[0], dtype)
    stacked = [p]
    for it in range(1, LI.NUM_ITER):
        rec, valid, _, _ = tw.warp(src, d_t, d_s, -p, K)
        c, _ = forward_pinned_net(net, torch.cat([tgt * valid, rec], 1), masks[it], dtype)
        p = p + c
        stacked.append(p)
    st = torch.stack(stacked, 1)
    (st * T(inp["R"])).sum().backward()
    named = dict(net.named_parameters())
    out = dict(stacked=st.detach().double().numpy(), grads={k: named[k].grad.detach() for k in NAMES})
    if depth_leaves:
        out["d_disp_t"], out["d_disp_s"] = disp_t.grad.double().numpy(), disp_s.grad.double().numpy()
    return out
