"""CPU: the float64 references, the rounding bounds, the parameter sets and the case table of tests/depthnet_layers.py, which the GPU
tests of the depth network's forward (tests/test_gpu_depthnet_layers.py) judge the HIP kernels with.

MEASURED here (printed by the tests):
  * chaining the isolated references reproduces the float64 twin to 2e-15 of a tensor's largest value, and the golden
    fixture's disparity (written by the reference's module in float64, stored as float32) to its storage rounding (2^-25);
  * torch's fp32 CPU convolution of the folded parameters uses at most 0.04 of the derived bound (by family: see
    test_fp32_twin_inside_the_bound);
  * what the bound and the hold rule each make of a faulty kernel's result: see test_criteria_reject_a_faulty_kernel;
  * fp32-against-float64 ReLU decisions of the twin alone are at most 5e-6 of a skip tensor, inside the 0.1 % cap, on every case."""
import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")

import depthnet_layers as DL      # noqa: E402
import depthnet_twin as dt        # noqa: E402


def _tapes(pset, H, W, N, kind, dtype):
    sd = DL.params(pset)
    x = DL.images(H, W, N, kind)
    return sd, x, DL.twin_tapes(sd, x, dtype)


@pytest.mark.parametrize("pset,H,W,kind", [("base", 32, 32, "sample"), ("hard", 96, 160, "special"), ("base", 160, 224, "sample")])
def test_isolated_references_chain_to_the_float64_twin(pset, H, W, kind):
    """every launch alone on the float64 twin's own tape entries is the twin's next entry: two routes to the same numbers (folded
    weights, explicit gather and conv2d / the twin's convolution, batch_norm, F.pad, F.interpolate)"""
    sd = DL.params(pset)
    x = DL.images(H, W, 2, kind)
    enc, dec, disp, skips = DL.twin_tapes(sd, x, torch.float64, c045=0.45)
    assert [tuple(e.shape[1:]) for e in enc] == DL.encoder_tape_shapes(H, W) == dt.encoder_tape_shapes(H, W)
    assert [tuple(d.shape[1:]) for d in dec] == DL.decoder_tape_shapes(H, W)
    names, worst = [], 0.0
    for c in DL.checks(sd, H, W, enc, dec, want_fp32=False, c045=0.45):
        e = float((c["out"] - c["ref"]).abs().max()) / max(1.0, float(c["ref"].abs().max()))
        worst = max(worst, e)
        assert e <= 1e-12, (c["name"], e)
        if c["bound"] is not None:
            assert float(c["bound"].min()) >= 0 and bool(torch.isfinite(c["bound"]).all())
        names.append(c["name"])
    print(f"{pset} {H}x{W}: worst chained-vs-isolated difference {worst:.1e}")
    # 33 launches; a downsample is judged with its block's second convolution (-3), a skip add before and after the add (+4)
    assert len(names) == 33 - 3 + 4 and len(set(names)) == len(names)
    assert torch.equal(DL.nchw(dec[-1].unsqueeze(-1)), disp)
    ref = dt.forward({k: v.double() for k, v in sd.items()}, x.double())
    assert float((disp - ref).abs().max()) <= 1e-12


def test_chained_float64_vs_reference_golden():
    g = load_golden("depthnet")
    for tag, (N, H, W) in (("s64x192", (3, 64, 192)), ("s192x640", (1, 192, 640))):
        sd = dt.depthnet_params(int(g["seed"]))
        x = torch.from_numpy(dt.sample_images(int(g[f"{tag}_img_seed"]), N, H, W))
        _, _, disp, _ = DL.twin_tapes(sd, x, torch.float64, c045=0.45)
        st = int(g[f"{tag}_disp_step"])
        e = float(np.max(np.abs(disp.numpy()[:, :, ::st, ::st] - g[f"{tag}_disp"])))
        print(f"{tag}: float64 chain vs golden disparity {e:.2e} ({g[f'{tag}_disp'].dtype})")
        # the fixture is the reference's float64 output; stored as float32 it carries half an ulp of a value below 1
        assert e <= (2.0 ** -25 if g[f"{tag}_disp"].dtype == np.float32 else 1e-12)


@pytest.mark.parametrize("H,W,pset,kind", [(32, 32, "base", "sample"), (32, 96, "base", "sample"), (96, 32, "hard", "sample"),
                                           (160, 224, "hard", "special"), (160, 416, "base", "special"), (192, 640, "base", "sample"),
                                           (320, 1024, "base", "sample"), (352, 1184, "hard", "sample")])
def test_fp32_twin_inside_the_bound(H, W, pset, kind):
    """the bound is not too tight for a correct fp32 kernel: torch's own fp32 convolution of the fp32-rounded folded parameters on
    the fp32 twin's operands (with relu / elu / the add / sigmoid in fp32) stays inside it at every launch, with room.  MEASURED,
    largest share of the bound in use over these cases: conv1 0.039, encoder 3x3 0.013, residual 0.020, up-convolutions 0.013,
    iconvs 0.022, feature convolution 0.016, head 0.035"""
    N = 2 if kind == "special" else 1
    sd, x, (enc, dec, _, _) = _tapes(pset, H, W, N, kind, torch.float32)
    for c in DL.checks(sd, H, W, enc, dec, want_fp32=True):
        r = DL.judge(dict(c, out=c["f32"], exact=None) if c["f32"] is not None else c)
        print(f"{H}x{W} {pset} {r['name']:32s} err/bound {r['frac']:.4f}  rel L2 {r['rel32']:.2e}  max/RMS {r['mx32']:.2e}")
        assert r["frac"] <= 0.25, r


def _zero_tap(w):
    w[:, 0, w.shape[2] // 2, w.shape[3] // 2] = 0
    return w


def _drop_group(w):
    w[:, 16:32, 0, 0] = 0
    return w


def _tenth_off(w):
    w[:, 0, w.shape[2] // 2, w.shape[3] // 2] *= 0.9
    return w


def _hundredth_off(w):
    """one term of the K wrong by a hundredth: what a worst-case K-term bound lets through in the deep layers (K = 4608)"""
    w[:, 0, w.shape[2] // 2, w.shape[3] // 2] *= 0.99
    return w


def _mantissa10_off(w):
    """one term of the K off by 2^-10, an ulp of a 10-bit mantissa (a weight that went through half precision or tf32)"""
    w[:, 0, w.shape[2] // 2, w.shape[3] // 2] *= 1.0 - 2.0 ** -10
    return w


# (launch, fault, the criterion that must reject it ON ITS OWN: "bound", "hold" (the bound accepts), or "both")
MUTANTS = [
    ("conv1", dict(wfn=_zero_tap), "both"),
    ("layer1.0.conv1", dict(wfn=_zero_tap), "both"), ("layer1.0.conv1", dict(wfn=_drop_group), "both"),
    ("layer2.0.conv1", dict(wfn=_zero_tap), "both"), ("layer2.0.conv1", dict(wfn=_drop_group), "both"),
    ("layer1.0.conv2", dict(wfn=_zero_tap), "both"), ("layer1.0.conv2", dict(wfn=_drop_group), "both"),
    ("layer2.0.downsample", dict(wfn=_zero_tap), "both"), ("layer2.0.downsample", dict(wfn=_drop_group), "both"),
    ("depth_upconvs.0", dict(wfn=_zero_tap), "both"), ("depth_upconvs.0", dict(wfn=_drop_group), "both"), ("depth_upconvs.0", dict(shift_up=1), "both"),
    ("depth_upconvs.4", dict(wfn=_zero_tap), "both"), ("depth_upconvs.4", dict(wfn=_drop_group), "both"), ("depth_upconvs.4", dict(shift_up=1), "both"),
    ("iconvs.0", dict(wfn=_zero_tap), "both"), ("iconvs.0", dict(wfn=_drop_group), "both"), ("iconvs.0", dict(reflect_off=1), "both"),
    ("feature_convs.0", dict(wfn=_zero_tap), "both"), ("feature_convs.0", dict(wfn=_drop_group), "both"), ("feature_convs.0", dict(reflect_off=1), "both"),
    ("head", dict(reflect_off=1), "both"),
    # the deep layers, K = 4608
    ("layer4.1.conv1", dict(wfn=_zero_tap), "both"), ("layer4.1.conv2", dict(wfn=_drop_group), "both"), ("layer4.0.downsample", dict(wfn=_zero_tap), "both"),
    ("layer4.1.conv2", dict(wfn=_tenth_off), "both"),
    ("layer4.1.conv2", dict(wfn=_hundredth_off), "hold"), ("layer4.0.conv2", dict(wfn=_hundredth_off), "hold"),
    ("depth_upconvs.0", dict(wfn=_hundredth_off), "hold"), ("depth_upconvs.0", dict(wfn=_mantissa10_off), "hold"),
]


@pytest.mark.parametrize("launch,fault,by", MUTANTS,
                         ids=[f"{l}-" + "+".join(k if k != "wfn" else f.__name__.strip("_") for k, f in ft.items()) for l, ft, _ in MUTANTS])
def test_criteria_reject_a_faulty_kernel(launch, fault, by):
    """the criteria see the faults they are for.  The fp32 result of a kernel with ONE fault -- one tap of one input channel zeroed or
    a tenth off, one 16-channel K group of one tap dropped, the far-edge reflection index off by one, the nearest up-sampling shifted
    by one -- is judged against the true float64 reference and the true fp32 baseline, as a faulty kernel is on the GPU: the launch
    fails, by the criterion named, and every other launch of the correct fp32 network passes.
    MEASURED (96x160): the gross faults leave the bound by 15 .. 26 000 x and the hold rule by 3e3 .. 4e5 x, except a zeroed tap in
    depth_upconvs.0 (K = 4608), which leaves the bound by 9.3 x only; a term a hundredth off in the K = 4608 layers uses 0.09 .. 0.42
    of the bound and is seen by the hold rule alone, by 27 .. 370 x; a term off by 2^-10 in depth_upconvs.0 by 3.7 x (relative L2)
    and 2.7 x (max / RMS).  So a bound 10 x wider accepts the zeroed tap of depth_upconvs.0, and a margin 10 x wider the last
    mutant: either loosening fails this test.  (Behind a x2 nearest up-sampling the
    reflected column vw - 2 and the column vw - 1 are the same source pixel, so the reflection fault exists for the iconvs, the
    feature convolution and the head only.)"""
    H, W = 96, 160
    sd, x, (enc, dec, _, _) = _tapes("base", H, W, 1, "sample", torch.float32)
    names = [L["name"] for L in DL.layers(H, W)]
    li = "head" if launch == "head" else names.index(launch)
    hit = 0
    for c in DL.checks(sd, H, W, enc, dec, want_fp32=True, fault=(li, fault)):
        if c["faulty"] is None:
            assert DL.judge(c)["ok"], c["name"]
            continue
        hit += 1
        r = DL.judge(dict(c, out=c["faulty"], exact=None))
        h_rel, h_mx = DL.hold(DL.FLOOR_REL_L2, r["rel32"]), DL.hold(DL.FLOOR_MAX_RMS, r["mx32"])
        print(f"MUTANT {launch} {sorted(fault)} {r['name']}: err/bound {r['frac']:.3g}; rel L2 {r['rel']:.2e} = {r['rel'] / h_rel:.3g} x hold; max/RMS {r['mx']:.2e} = {r['mx'] / h_mx:.3g} x hold")
        assert not r["ok"], r
        if by in ("bound", "both"):
            assert not r["ok_bound"], r
        if by in ("hold", "both"):
            assert not r["ok_hold"], r
        if by == "hold":
            assert r["ok_bound"], r          # the worst-case bound lets this one through: only the hold rule sees it
    assert hit == (2 if launch.startswith("depth_upconvs.") and launch != "depth_upconvs.4" else 1)


def test_selection_table_and_cases_cover_every_reachable_split():
    inst, part = set(), set()
    for H in range(32, 353, 32):
        for W in range(32, 1217, 32):
            i, p = DL.reached(H, W)
            inst |= i
            part |= p
    assert inst == DL.NEEDED and part == DL.NEEDED_PARTIAL
    assert {i[1:] for i in DL.NEEDED} == DL.INSTANCES and len(DL.INSTANCES) == 8
    got_i, got_p, old_i, old_p = set(), set(), set(), set()
    for H, W in DL.SIZES:
        i, p = DL.reached(H, W)
        got_i |= i
        got_p |= p
    assert got_i == DL.NEEDED and got_p == DL.NEEDED_PARTIAL
    for H, W in DL.OLD_SIZES:
        i, p = DL.reached(H, W)
        old_i |= i
        old_p |= p
    # what no test launched before: the wide 1x1 downsample (and with it layer2 in the wide form), and any KW = 1 layer partly filled
    assert DL.INSTANCES - {i[1:] for i in old_i} == {(1, 4, 2, 1)}
    assert DL.NEEDED - old_i == {("down1x1", 1, 4, 2, 1), ("stride2", 3, 4, 2, 1)}
    assert DL.NEEDED_PARTIAL - old_p == {(1, "workgroup"), (1, "wave")}
    per_layer = lambda sizes: {(L["name"],) + t[1:4] for H, W in sizes for L, t in list(zip(DL.layers(H, W), DL.selection_table(H, W)))[1:]}
    new = per_layer(DL.SIZES) - per_layer(DL.OLD_SIZES)
    assert len(new) == 14 and {n.split(".")[0] for n, *_ in new} == {"layer2", "layer3", "depth_upconvs", "iconvs"}, sorted(new)
    # the geometry the sizes were chosen for
    tab = {L["name"]: t for L, t in zip(DL.layers(160, 416), DL.selection_table(160, 416))}
    assert tab["layer1.0.conv1"] == (3, 4, 2, 1, 4160, True, False) and 4160 == 32 * 128 + 64
    tab = {L["name"]: t for L, t in zip(DL.layers(352, 1184), DL.selection_table(352, 1184))}
    assert tab["layer2.0.downsample"] == (1, 4, 2, 1, 6512, True, True) and 6512 % 32 == 16
    assert tab["layer3.1.conv2"] == (3, 2, 1, 4, 1628, True, True) and 1628 % 16 == 12
    tab = {L["name"]: t for L, t in zip(DL.layers(320, 1024), DL.selection_table(320, 1024))}
    assert tab["layer2.0.downsample"] == (1, 4, 2, 1, 5120, False, False) and tab["layer3.0.downsample"][:4] == (1, 2, 1, 4)
    tab = {L["name"]: L for L in DL.layers(32, 32)}
    assert (tab["layer4.1.conv2"]["oh"], tab["layer4.1.conv2"]["ow"], tab["depth_upconvs.0"]["oh"]) == (1, 1, 2)
    assert all(1 <= M < N or N == 1 for _, _, N, M, _, _ in DL.CASES)
    assert len(DL.layers(64, 64)) == 31


def test_inputs_and_parameter_sets():
    base, again, hard = dt.depthnet_params(3), dt.depthnet_params(3), DL.params("hard")
    assert all(torch.equal(base[k], again[k]) for k in base)
    assert list(hard) == list(base) and all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in hard.values())
    g, g0 = hard[f"{dt.ENC}layer2.0.bn1.weight"], base[f"{dt.ENC}layer2.0.bn1.weight"]
    assert bool((g[2::4] * g0[2::4] < 0).all()) and bool((g[0::4] * g0[0::4] > 0).all())
    v, v0 = hard[f"{dt.ENC}layer3.1.bn2.running_var"], base[f"{dt.ENC}layer3.1.bn2.running_var"]
    assert 1e-3 * 0.99 <= float((v / v0)[3::8].min()) and float((v / v0)[3::8].max()) <= 0.1 and float((v / v0).min()) < 5e-3
    m, m0 = hard[f"{dt.ENC}layer1.0.bn1.running_mean"], base[f"{dt.ENC}layer1.0.bn1.running_mean"]
    sig = hard[f"{dt.ENC}layer1.0.bn1.running_var"].sqrt()
    assert float(((m - m0).abs() / sig)[1::4].min()) >= 1.99
    f = lambda sd, k: (sd[k + ".weight"].double() / (sd[k + ".running_var"].double() + 1e-5).sqrt())
    spread = max(float(f(hard, f"{dt.ENC}layer{i}.0.bn1").abs().max() / f(hard, f"{dt.ENC}layer{i}.0.bn1").abs().median()) for i in (1, 2, 3, 4))
    assert spread > 8.0
    x = DL.images(64, 192, 2, "sample")
    enc, dec, disp, skips = DL.twin_tapes(hard, x, torch.float64)
    encb, *_ = DL.twin_tapes(base, x, torch.float64)
    for e in (1, 6, 10, 14, 18):       # activations stay O(1)
        assert 0.3 < float(enc[e].pow(2).mean().sqrt() / encb[e].pow(2).mean().sqrt()) < 3.0, e
    share = float((dec[1] < np.expm1(-3.0)).double().mean())       # ELU output of a pre-activation below -3
    print(f"pre-ELU values below -3 in depth_upconvs.0: {share:.2f}; disparity {float(disp.min()):.3f} .. {float(disp.max()):.3f}")
    assert share > 0.15 and float(disp.max() - disp.min()) > 0.05
    s = DL.images(96, 160, 3, "special")
    assert bool((s[0] == np.float32(0.45)).all()) and bool((s[1][:, 2:-2, 2:-2] == np.float32(0.45)).all())
    assert float((s[1][:, :2] - 0.45).abs().mean()) > 0.05 and float((s[1][:, :, -2:] - 0.45).abs().mean()) > 0.05
    assert len({s[i].numpy().tobytes() for i in range(3)}) == 3
    # a frame of 0.45f normalises to exactly zero: conv1's reference is relu(b') at every pixel, padding included
    c = next(iter(DL.checks(base, 96, 160, [s, torch.zeros(3, 48, 80, 64), None], None, want_fp32=False)))
    _, b = DL.fold64(base, DL.layers(96, 160)[0])
    assert torch.equal(c["ref"][0], torch.relu(b).view(64, 1, 1).expand(64, 48, 80))


@pytest.mark.parametrize("case", DL.CASES, ids=DL.CASE_IDS)
def test_fp32_twin_alone_stays_inside_the_decision_cap(case):
    """the chained comparison leaves out skip elements whose ReLU decided differently in fp32 and float64; fp32 arithmetic alone
    must stay inside the cap on every case, or the case is a bad input whatever the kernels do"""
    H, W, N, M, pset, kind = case
    sd = DL.params(pset)
    x = DL.images(H, W, N, kind)
    _, _, d64, s64 = DL.twin_tapes(sd, x, torch.float64)
    _, _, d32, s32 = DL.twin_tapes(sd, x, torch.float32)
    for k, (a, b) in enumerate(zip(s32, s64)):
        n = int(DL.relu_flips(a, b).sum())
        print(f"skip {k}: {n} of {a.numel()} decisions differ ({n / a.numel():.1e}); cap {DL.decision_cap(a.numel())}")
        assert n <= DL.decision_cap(a.numel()), (k, n, a.numel())
    assert bool(torch.isfinite(d32).all()) and float((d32.double() - d64).abs().max()) < 1e-4
