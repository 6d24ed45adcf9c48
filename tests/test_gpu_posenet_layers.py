"""GPU: the HIP PoseNet (csrc/posenet_kernel.h) layer by layer against float64, across every work split.

The library's read-out of its last evaluation (tcsfm_debug_posenet_layer / _split, PoseNetHIP.layer / .split) gives every layer's raw
convolution output and GroupNorm (scale, shift) pairs; tests/posenet_layers.py holds the float64 references, the derived rounding
bound of a convolution output, the derived tolerance of the statistics, the parameter sets and the case table.

  1  every layer ALONE: raw[l] against the float64 convolution of the library's own fp32 raw[l-1], scsh[l-1] -- |error| <= bound at
     every output; scale / shift against the float64 GroupNorm of the library's own raw[l] -- inside the derived tolerance
  2  the chain end to end against the chained float64 twin: relative L2 and max error / RMS per layer and the pose within
     max(floor, 4 x the fp32 CPU twin's own figure)
  3  the window form of layer 1 (indexed targets / sources) bit for bit against the pair form on the hand-gathered batch
  4  one image in an N <= 4 call and in an N > 4 call: layers differ by no more than the sum of the two bounds
  5  1 and 2 with group means at 3..10 standard deviations, and with near-zero / negative gammas
  6  constant and almost-empty frames

MEASURED on an MI355X (TCSFM_TEST_POSENET_REPORT=<file> keeps one line per case and layer).

Check 1, worst over all cases (57 tests: base, offset and gamma parameter sets, window and degenerate inputs), share of the derived
bound / tolerance in use -- convolution output | scale | shift:
    layer 1   0.024  regimes, 320x1024 N=5, nb1 ks1 pb1        | 0.054 all-0.45 37x53           | 0.120 gamma 192x640 N=5
    layer 2   0.014  base, 192x640 N=2, nb2 ks1 pb1            | 0.42  constant 100x333, ks2    | 0.33
    layer 3   0.022  gamma, 192x640 N=5, nb4 ks1 pb2           | 0.43  gamma 17x33 N=2, ks2     | 0.32
    layer 4   0.010  base, 375x1242 N=5, nb4 ks1 pb2           | 0.46  base 17x33 N=5, ks2      | 0.35
    layer 5   0.004  base, 375x1242 N=1, nb1 ks1 pb1           | 0.47  window S3 B3, ks3        | 0.34
    layer 6   0.001  base, 5x9 N=7, nb4 ks6 pb1                | 0.46  base 17x33 N=5, ks6      | 0.36
    layer 7   0.001  window S2 B1, nb1 ks16 pb1                | 0.47  window S2 B2, ks6        | 0.36
The convolutions use a fiftieth of the worst-case bound, as torch's fp32 convolution does on the CPU.  K-split layers sum their
statistics in double, their tolerance is the 4 u of the fp32 results themselves and about half of it is used.

Check 2, worst ratio  |hip - f64| / |fp32 CPU twin - f64|  against the margin of 4 (floors: 8 u relative L2, 64 u max / RMS, 8 u pose)
-- relative L2 | max error / RMS:
    layer 1   1.11 (2.4e-7, 5x9 N=7)             | 1.24 (3.2e-6, 37x53 N=7)
    layer 2   1.30 (6.8e-7, constant 37x53)      | 1.29 (3.8e-6, constant 37x53)
    layer 3   1.22 (8.0e-7, constant 37x53)      | 1.40 (6.5e-6, gamma 375x1242 N=1)
    layer 4   1.11 (8.9e-7, constant 37x53)      | 1.35 (4.5e-6, gamma 37x53 N=7)
    layer 5   1.05 (1.1e-6, constant 37x53)      | 1.10 (7.5e-6, gamma 375x1242 N=1)
    layer 6   1.00 (5.2e-5, all-0.45 37x53)      | 1.03 (4.4e-6, constant 37x53)
    layer 7   1.00 (5.0e-5, all-0.45 37x53)      | 1.04 (2.2e-6, 5x9 N=1)
    pose      1.58 (1.8e-6 of the largest pose, base 37x53 N=4)

Check 4, largest  |few - many| / (bound_few + bound_many)  per layer: 0 (layer 1: one kernel, bit-identical), 0.0053, 0.0071, 0.0033,
0.0017, 0.0010, 0.0008 for layers 2..7, all at 100x333 but layer 5 (192x640) and layer 7 (17x33); largest absolute difference 1.1e-4
(layer 6).

Check 5 found a fault, fixed with these tests: the epilogues summed x and x^2 INCLUDING the bias in fp32, and with group means at 3..10
standard deviations the activation formed from the library's (scale, shift) was 20.2 x (17x33 N=2, layer 1: 3.0e-5), 9.8 x (37x53 N=7,
layer 1) and 5.9 x (37x53 N=7, layer 3) further from float64 than torch's fp32 GroupNorm on the same raw output; K-split layers,
summed in double, were at 0.5 x.  The partial sums are now those of x - bias and k_pn_stats adds the bias back in double: the worst
ratio over all offset and gamma cases is 1.01 (17x33 N=2, layer 5), every other layer below 1.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import posenet_layers as PL      # noqa: E402


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_POSENET_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _net(H, W, M, sd, engine_pairs=None):
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    return PoseNetHIP(Engine(H, W, engine_pairs or M), M, sd)


def _layers(net, N):
    """(raw [N,C,h,w], scsh [N,C,2]) of layers 1..7 of the last evaluation, on the CPU"""
    return [tuple(t.cpu().contiguous() for t in net.layer(l, N)) for l in range(1, 8)]


def _check_layers_alone(test, tag, sd, x, net, N):
    """check 1 on the last evaluation of `net` (inputs x [N,6,H,W], CPU) -> (layers, bounds)"""
    lay = _layers(net, N)
    fails, bounds = [], []
    for l in range(1, 8):
        raw, scsh = lay[l - 1]
        a = PL.operand64(1, imgs=x) if l == 1 else PL.operand64(l, raw=lay[l - 2][0], scsh=lay[l - 2][1])
        y, bound = PL.isolated64(sd, l, a)
        bounds.append(bound)
        assert raw.shape == y.shape, (l, raw.shape, y.shape)
        r_conv = float(((raw.double() - y).abs() / bound).max())
        nb, ks, pb = net.split(l, N)[2:]
        ref, tol = PL.scsh_tolerance(raw, sd[f"conv{l}.1.weight"], sd[f"conv{l}.1.bias"], PL.stats_group_size(l, nb, ks, pb))
        d = (scsh.double() - ref).abs()
        r_sc, r_sh = float((d[:, :, 0] / tol[:, :, 0]).max()), float((d[:, :, 1] / tol[:, :, 1]).max())
        rel_sc = float((d[:, :, 0] / ref[:, :, 0].abs().clamp_min(1e-30)).max())
        _report(f"{test}\t{tag}\tlayer {l} nb{nb} ks{ks} pb{pb}\tconv err/bound={r_conv:.4f}\tscale err/tol={r_sc:.4f}\tshift err/tol={r_sh:.4f}\tscale rel err={rel_sc:.2e}")
        if not (r_conv <= 1.0 and r_sc <= 1.0 and r_sh <= 1.0 and bool(torch.isfinite(raw).all()) and bool(torch.isfinite(scsh).all())):
            fails.append((l, r_conv, r_sc, r_sh))
    assert not fails, (test, tag, fails)
    return lay, bounds


def _check_chain(test, tag, sd, x, lay, pose):
    """check 2: per layer and for the pose, error against the chained float64 twin <= max(floor, 4 x the fp32 CPU twin's)"""
    c64, c32 = PL.chained64(sd, x), PL.chained(sd, x, torch.float32)
    fails = []
    for l in range(1, 8):
        ref = c64["raw"][l - 1]
        for name, fn, floor in (("rel L2", PL.rel_l2, PL.FLOOR_REL_L2), ("max/RMS", PL.max_over_rms, PL.FLOOR_MAX_RMS)):
            e, e32 = fn(lay[l - 1][0], ref), fn(c32["raw"][l - 1], ref)
            _report(f"{test}\t{tag}\tlayer {l}\t{name}\thip-f64={e:.3e}\tf32-f64={e32:.3e}\tratio={e / e32 if e32 > 0 else float('nan'):.2f}\tbound={PL.hold(floor, e32):.3e}")
            if not e <= PL.hold(floor, e32):
                fails.append((l, name, e, e32))
    pm = float(c64["pose"].abs().max())
    e, e32 = float((pose.double() - c64["pose"]).abs().max()) / pm, float((c32["pose"].double() - c64["pose"]).abs().max()) / pm
    _report(f"{test}\t{tag}\tpose\tmax/max\thip-f64={e:.3e}\tf32-f64={e32:.3e}\tratio={e / e32 if e32 > 0 else float('nan'):.2f}\tbound={PL.hold(PL.FLOOR_POSE, e32):.3e}")
    if not e <= PL.hold(PL.FLOOR_POSE, e32):
        fails.append(("pose", e, e32))
    assert not fails, (test, tag, fails)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PL.CASES, ids=PL.CASE_IDS)
def test_every_layer_alone_and_chained_vs_float64(case):
    """checks 1 and 2 at every size and in both regimes; the case asserts, through the library's read-out, that it launched the work
    splits it is there for"""
    H, W, N, M, combos = case
    tag = PL.CASE_IDS[PL.CASES.index(case)]
    sd = PL.PARAM_SETS["base"](3)
    x = PL.images(H, W, N, seed=5)
    assert len({x[i].numpy().tobytes() for i in range(N)}) == N
    net = _net(H, W, M, sd)
    tab = PL.selection_table(H, W)
    for l in range(1, 8):
        oh, ow, nb, ks, pb = net.split(l, N)
        assert (oh, ow) == (tab[l - 1]["oh"], tab[l - 1]["ow"])
    for (l, nb, ks, pb) in combos:
        assert net.split(l, N)[2:] == (nb, ks, pb), (l, net.split(l, N))
    pose = net(x.cuda()).cpu()
    lay, _ = _check_layers_alone("alone", tag, sd, x, net, N)
    _check_chain("chain", tag, sd, x, lay, pose)


@pytest.mark.parametrize("pset", ["offset", "gamma"])
@pytest.mark.parametrize("H,W,N", [(17, 33, 2), (37, 53, 7), (100, 333, 2), (192, 640, 5), (375, 1242, 1)])
def test_offset_statistics_and_degenerate_gammas(pset, H, W, N):
    """check 5: group means at 3..10 standard deviations (var = E[x^2] - mean^2 cancels up to 100 times its size) and gammas near zero
    or negative; the same checks as above, and the activation the consumer forms from the library's (scale, shift) no further from
    float64 than 4 x what torch's fp32 GroupNorm on the CPU makes of the same raw output"""
    sd = PL.PARAM_SETS[pset](3)
    x = PL.images(H, W, N, seed=6)
    net = _net(H, W, N, sd)
    pose = net(x.cuda()).cpu()
    tag = f"{pset}-{H}x{W}-N{N}"
    lay, _ = _check_layers_alone("alone", tag, sd, x, net, N)
    fails = []
    for l in range(1, 8):
        raw, scsh = lay[l - 1]
        gamma, beta = torch.as_tensor(sd[f"conv{l}.1.weight"]), torch.as_tensor(sd[f"conv{l}.1.bias"])
        ref = PL.operand64(l + 1, raw=raw, scsh=PL.gn_scsh64(raw.double(), gamma, beta)[0])
        hip = PL.operand64(l + 1, raw=raw, scsh=scsh)
        t32 = torch.relu(torch.nn.functional.group_norm(raw, 16, gamma, beta, 1e-5)).double()
        e, e32 = float((hip - ref).abs().max()), float((t32 - ref).abs().max())
        # floor: the fp32 rounding of scale and shift themselves, which the library's consumer reads as fp32 numbers
        floor = 4 * PL.U * float((raw.double().abs() * scsh[:, :, 0, None, None].double().abs() + scsh[:, :, 1, None, None].double().abs()).max())
        _report(f"gn\t{tag}\tlayer {l}\tactivation max err\thip-f64={e:.3e}\tf32-f64={e32:.3e}\tratio={e / e32 if e32 > 0 else float('nan'):.2f}\tbound={PL.hold(floor, e32):.3e}")
        if not e <= PL.hold(floor, e32):
            fails.append((l, e, e32, floor))
    assert not fails, (tag, fails)
    _check_chain("chain", tag, sd, x, lay, pose)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_window_form_equals_pair_form_bit_for_bit(S, B):
    """check 3: solve_pose_iteratively's first evaluation gathers (tgt b | src (s, b)) and the swapped inverse pairs by index; the
    same network on the explicitly concatenated batch gives the same bits, in the poses and in layer 1's raw output.  All frames
    differ, so a wrong source index cannot pass.  N = 2 S B runs from 2 to 24, across the two regimes."""
    H, W = 37, 53
    N = 2 * S * B
    rng = np.random.default_rng(100 * S + B)
    tgt = torch.tensor(rng.uniform(0, 1, size=(B, 3, H, W)).astype(np.float32))
    srcs = torch.tensor(rng.uniform(0, 1, size=(S, B, 3, H, W)).astype(np.float32))
    depth_t = torch.tensor(rng.uniform(0.5, 2.0, size=(B, 1, H, W)).astype(np.float32))
    depth_s = torch.tensor(rng.uniform(0.5, 2.0, size=(S, B, 1, H, W)).astype(np.float32))
    K = torch.tensor(np.repeat(np.array([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=np.float32)[None], B, 0))
    sd = PL.PARAM_SETS["base"](3)
    net = _net(H, W, N, sd)
    poses, stacked = net.solve_pose_iteratively(1, tgt.cuda(), srcs.cuda(), depth_t.cuda(), depth_s.cuda(), K.cuda())
    raw1_win = net.layer(1, N)[0].clone()
    fwd = torch.cat([torch.cat([tgt[b], srcs[s, b]], 0)[None] for s in range(S) for b in range(B)])
    inv = torch.cat([torch.cat([srcs[s, b], tgt[b]], 0)[None] for s in range(S) for b in range(B)])
    x = torch.cat([fwd, inv]).contiguous()
    assert x.shape == (N, 6, H, W) and len({x[i].numpy().tobytes() for i in range(N)}) == N
    pair = net(x.cuda())
    raw1_pair = net.layer(1, N)[0]
    assert torch.equal(raw1_win, raw1_pair)
    assert torch.equal(poses, pair) and torch.equal(stacked[:, 0], pair)
    # ... and the pair form is the float64 network on that batch (else two equal wrong answers would pass)
    lay, _ = _check_layers_alone("window", f"S{S}-B{B}", sd, x, net, N)


@pytest.mark.parametrize("H,W", [(17, 33), (100, 333), (192, 640), (320, 1024)])
def test_regimes_agree_within_the_sum_of_their_bounds(H, W):
    """check 4: include/tcsfm.h promises that one image evaluated in a call of up to 4 images and in a call of more agrees 'to
    rounding'; per layer the two raw outputs differ by no more than the sum of the two calls' rounding bounds"""
    sd = PL.PARAM_SETS["base"](3)
    x = PL.images(H, W, 5, seed=7)
    few, many = _net(H, W, 2, sd), _net(H, W, 5, sd)
    p_few = few(x[:2].contiguous().cuda()).cpu()
    lay_f, b_f = _check_layers_alone("regimes-few", f"{H}x{W}", sd, x[:2], few, 2)
    p_many = many(x.cuda()).cpu()
    lay_m, b_m = _check_layers_alone("regimes-many", f"{H}x{W}", sd, x, many, 5)
    fails = []
    for l in range(1, 8):
        d = (lay_f[l - 1][0].double() - lay_m[l - 1][0][:2].double()).abs()
        r = float((d / (b_f[l - 1] + b_m[l - 1][:2])).max())
        same = few.split(l, 2)[2:] == many.split(l, 5)[2:]
        _report(f"regimes\t{H}x{W}\tlayer {l}\tfew {few.split(l, 2)[2:]} many {many.split(l, 5)[2:]}\tdiff/(bound+bound)={r:.4f}\tmax diff={float(d.max()):.3e}")
        if not r <= 1.0:
            fails.append((l, r))
        if l == 1:
            assert same and torch.equal(lay_f[0][0], lay_m[0][0][:2]) and torch.equal(lay_f[0][1], lay_m[0][1][:2])    # one kernel, one split
    assert not fails, fails
    assert float((p_few - p_many[:2]).abs().max()) < 3e-6 * float(p_many.abs().max())       # (the bar of tests/test_gpu_posenet.py)


def _degenerate(kind, H, W):
    x = torch.zeros((2, 6, H, W), dtype=torch.float32)
    if kind == "all-0.45":
        x += 0.45
    elif kind == "constant":
        x[0] += 0.8; x[1] += 0.1
    else:                       # zero except the last row and column, values all different
        rng = np.random.default_rng(8)
        x[:, :, -1, :] = torch.tensor(rng.uniform(0.5, 1, size=(2, 6, W)).astype(np.float32))
        x[:, :, :, -1] = torch.tensor(rng.uniform(0.5, 1, size=(2, 6, H)).astype(np.float32))
    return x


@pytest.mark.parametrize("kind", ["all-0.45", "constant", "last-row-and-column"])
@pytest.mark.parametrize("H,W", [(37, 53), (100, 333)])
def test_constant_and_degenerate_inputs(kind, H, W):
    """check 6: padding is applied AFTER the input normalisation (a constant frame is not constant at the border unless it is 0.45),
    and var = max(E[x^2] - mean^2, 0) of a constant layer must give rstd = 1 / sqrt(eps), not NaN"""
    sd = PL.PARAM_SETS["base"](3)
    x = _degenerate(kind, H, W)
    net = _net(H, W, 2, sd)
    pose = net(x.cuda()).cpu()
    assert bool(torch.isfinite(pose).all())
    lay, _ = _check_layers_alone("degenerate", f"{kind}-{H}x{W}", sd, x, net, 2)
    raw1, scsh1 = lay[0]
    bias, gamma = torch.as_tensor(sd["conv1.0.bias"]), torch.as_tensor(sd["conv1.1.weight"])
    if kind == "all-0.45":      # the normalised frame is zero: conv1 = bias exactly, variance over a group = that of its one bias value = 0
        assert torch.equal(raw1, bias.view(1, 16, 1, 1).expand_as(raw1))
        want = gamma.double() / np.sqrt(1e-5)
        assert float(((scsh1[:, :, 0].double() - want).abs() / want.abs()).max()) < 0.02       # dvar <= 3 * 129 u bias^2 = 2e-7 beside eps = 1e-5
    if kind == "constant":      # interior outputs see a constant patch and zero-mean weights: bias again, to rounding; the border does not
        inner = raw1[:, :, 2:-2, 2:-2]
        assert float((inner - bias.view(1, 16, 1, 1)).abs().max()) < 1e-4
        assert float((raw1[:, :, 0, :] - bias.view(1, 16, 1)).abs().min()) > 1e-3
    # end to end by the rule of check 2: a frame of 0.45 leaves only the zero-padded borders of the later layers as signal beside a large
    # constant, and the fp32 CPU twin itself is 1.2e-4 from float64 in the pose at 100x333 -- the twin's own error sets the bar
    _check_chain("chain", f"{kind}-{H}x{W}", sd, x, lay, pose)


def test_read_out_refuses_bad_arguments():
    sd = PL.PARAM_SETS["base"](3)
    net = _net(17, 33, 3, sd)
    with pytest.raises(RuntimeError):
        net.layer(1, 1)                          # nothing evaluated yet
    net(PL.images(17, 33, 2, seed=9).cuda())
    for l, n in ((0, 1), (8, 1), (1, 0), (1, 3)):    # N = 3 exceeds the last evaluation's 2
        with pytest.raises(RuntimeError):
            net.layer(l, n)
    with pytest.raises(RuntimeError):
        net.split(3, 4)                          # beyond max_images
    raw, scsh = net.layer(7, 2)
    assert raw.shape == (2, 256, 1, 1) and scsh.shape == (2, 256, 2)
