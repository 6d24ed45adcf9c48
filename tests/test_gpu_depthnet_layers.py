"""GPU: the HIP depth network's forward (csrc/depthnet_kernel.h) launch by launch against float64, across every work split.

The training forward (tcsfm_depthnet_encode_train / _decode_train) runs the plain forward's kernels and leaves every launch's input
and output in its tapes; tests/depthnet_layers.py holds the float64 references, the derived rounding bound, the statistical rule, the
parameter sets and the case table.  Per case (DL.CASES), from ONE training forward into tapes this test owns (pre-filled with NaN):

  1  the library's own read-out of its work split (tcsfm_debug_depthnet_split) equals the restated rule, launch by launch
  2  every launch ALONE against the float64 layer on the library's own fp32 operand: |error| <= the derived bound at every output,
     nothing excluded; relative L2 and max error / RMS <= max(floor, 4 x torch's fp32 CPU convolution's on the same operand);
     the max pool, the skip adds and conv1 on a frame of 0.45f bit for bit
  3  disparity and skips against the chained float64 twin, by the same rule against the fp32 CPU twin; skip elements whose ReLU
     decided differently are left out there, at most 0.1 % of a tensor
  4  forward / encode / decode give the tape's bits; forward(x, flip) is forward(torch.flip(x)); an image alone is the image in a group
and once: the union of the splits the cases launch is every (layer kind, KS, NB, PB, KW) the rule can reach (DL.NEEDED), all eight
k_dn_conv instances among them.

MEASURED on an MI355X (TCSFM_TEST_DEPTHNET_REPORT=<file> keeps one line per case and launch); the module takes about 50 s, 0.1-0.8 s of each
case on the GPU and the rest in the float64 references on the CPU (192x640 N = 3: 9.7 s, the two largest sizes 6-7 s each at N = 1).

Check 2, worst over the 11 cases -- share of the derived bound in use | relative L2 / torch fp32's | max error / RMS / torch fp32's:
    conv1                    0.048  352x1184 base                          | 1.15 (1.9e-7, 96x32 hard)     | 1.49 (1.3e-5, 160x416 hard)
    encoder 3x3              0.013  352x1184 hard, layer1.0.conv1 <3,4,2,1> | 1.00 (5.2e-7)                 | 1.32 (1.2e-5, layer2.1.conv1 352x1184, partial wave)
    residual (+ downsample)  0.018  352x1184 hard, layer1.1.conv2 <3,4,2,1> | 1.05 (3.3e-7, 160x416 special)| 1.21 (5.1e-6)
    up-convolutions          0.013  192x640, depth_upconvs.3 <3,4,2,1>      | 1.01 (3.8e-7)                 | 1.13 (1.3e-5)
    iconvs                   0.026  352x1184 base, iconvs.4 <3,2,2,1>       | 1.00 (4.1e-7)                 | 1.29 (1.2e-5, iconvs.2 160x416 hard, partial workgroup)
    feature_convs.0          0.017  352x1184 hard <3,1,2,1>                 | 1.01 (2.6e-7)                 | 1.22 (4.2e-6)
    predict_disps.0          0.036  320x1024                               | 1.00 (6.8e-8)                 | 1.01 (1.2e-6)
The convolutions use a fiftieth of the worst-case bound, as torch's fp32 convolution does on the CPU (test_depthnet_layers_cpu.py).
Check 3 (the float64 chain subtracts 0.45f, as the library and the fp32 twin do), worst ratio |hip - f64| / |fp32 CPU twin - f64|
against the margin of 4 -- relative L2 | max / RMS: disparity 1.31 (1.2e-6) | 1.95 (1.1e-5); skips 0..4: 1.09, 1.69, 2.29, 2.13, 2.14 |
1.37, 1.78, 3.47, 2.20, 2.46, the largest at 352x1184 with the hard parameter set (skip 2: 8.4e-7 and 3.4e-5).  ReLU decisions that differ
from float64: at most 2 per tensor (cap 1e-3 of it), HIP and fp32 twin alike.
No launch left its bound; nothing in the kernels was changed."""
import ctypes as C
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import depthnet_layers as DL     # noqa: E402
import depthnet_twin as dt       # noqa: E402

SKIP_C = (64, 64, 128, 256, 512)


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_DEPTHNET_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _train_forward(mod, x):
    """one encode_train + decode_train into NaN-filled tapes -> (native state, encoder entries, decoder entries, skips NHWC, disparity), on the GPU"""
    nat = mod._native_for(x)
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    e, d = C.c_int64(), C.c_int64()
    nat.eng._call(nat.lib.tcsfm_depthnet_tape_size(nat.dn, N, C.byref(e), C.byref(d)))
    per = lambda shp: N * sum(int(np.prod(s)) for s in shp)
    assert (int(e.value), int(d.value)) == (per(DL.encoder_tape_shapes(H, W)), per(DL.decoder_tape_shapes(H, W)))
    et = torch.full((int(e.value),), float("nan"), device=x.device)
    dtp = torch.full((int(d.value),), float("nan"), device=x.device)
    sk = [torch.full((N, H >> (k + 1), W >> (k + 1), c), float("nan"), device=x.device) for k, c in enumerate(SKIP_C)]
    disp = torch.full((N, 1, H, W), float("nan"), device=x.device)
    nat.eng._bind()
    nat.eng._call(nat.lib.tcsfm_depthnet_encode_train(nat.dn, N, nat.eng._p(x), C.cast(nat.ptrs(sk), C.c_void_p), nat.eng._p(et)))
    nat.eng._call(nat.lib.tcsfm_depthnet_decode_train(nat.dn, N, C.cast(nat.ptrs(sk), C.c_void_p), nat.eng._p(disp), nat.eng._p(dtp)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(et).all()) and bool(torch.isfinite(dtp).all()), "the training forward left part of a tape unwritten"
    enc, dec = dt.encoder_tape_entries(et, N, H, W), DL.decoder_tape_entries(dtp, N, H, W)
    assert torch.equal(enc[0].reshape(x.shape), x) and torch.equal(dec[0], sk[4]) and torch.equal(dec[-1].reshape(disp.shape), disp)
    for k, ei in enumerate(DL.SKIP_ENTRY):
        assert torch.equal(enc[ei], sk[k]), k
    return nat, enc, dec, sk, disp


def _library_split(net):
    return [net.split(li) for li in range(31)]


@pytest.mark.parametrize("case", DL.CASES, ids=DL.CASE_IDS)
def test_every_launch_alone_and_chained_vs_float64(case):
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    from tightly_coupled_sfm_amd.engine import Engine
    H, W, N, M, pset, kind = case
    tag = DL.CASE_IDS[DL.CASES.index(case)]
    t0 = time.time()
    sd = DL.params(pset)
    x = DL.images(H, W, N, kind)
    assert len({x[i].numpy().tobytes() for i in range(N)}) == N
    mod = DepthNetModule(sd, max_images=M).cuda()
    xg = x.cuda()
    nat, enc_g, dec_g, sk, disp = _train_forward(mod, xg)
    net = nat.net

    # 1  the split the library holds is the restated rule's
    LS, tab = DL.layers(H, W), DL.selection_table(H, W)
    with pytest.raises(RuntimeError):
        net.split(31)
    for li, (ks, oh, ow, nb, pb, kw) in enumerate(_library_split(net)):
        assert (ks, oh, ow) == (LS[li]["ks"], LS[li]["oh"], LS[li]["ow"]), (li, ks, oh, ow)
        assert li == 0 or (nb, pb, kw) == tab[li][1:4], (LS[li]["name"], nb, pb, kw, tab[li])

    # 4  the plain calls give the tape's bits (before the tapes leave the GPU)
    assert torch.equal(net.forward(xg), disp)
    for a, b in zip(net.encode(xg), sk):
        assert torch.equal(a, b)
    assert torch.equal(net.decode(sk), disp)
    xf = torch.flip(xg, [3]).contiguous()
    flipped = net.forward(xg, flip=True)
    assert torch.equal(flipped, net.forward(xf))
    assert not torch.equal(flipped, disp)
    if N > 1:
        for i in range(N):
            assert torch.equal(net.forward(xg[i:i + 1].contiguous()), disp[i:i + 1]), i
    else:       # the image behind another one in a group of two, on an instance loaded through the host fold
        pair = DepthNetHIP(Engine(H, W, 2), 2, sd)
        assert torch.equal(pair.forward(torch.cat([xf, xg]).contiguous())[1:2], disp)
        pair.close()
    torch.cuda.synchronize()
    enc, dec = [t.cpu() for t in enc_g], [t.cpu() for t in dec_g]
    hip_disp, hip_skips = disp.cpu(), [DL.nchw(s.cpu()) for s in sk]
    del enc_g, dec_g, sk, disp, nat, net, mod
    torch.cuda.empty_cache()
    t_gpu = time.time() - t0

    # 2  every launch alone
    fails, seen = [], 0
    for c in DL.checks(sd, H, W, enc, dec):
        r = DL.judge(c)
        seen += 1
        sp = "" if c["layer"] is None else " <%d,%d,%d,%d> npix %d" % tab[c["layer"]][:5]
        _report(f"alone\t{tag}\t{r['name']}{sp}\terr/bound={r['frac']:.4f}\trel L2 hip={r['rel']:.3e} f32={r['rel32']:.3e}\tmax/RMS hip={r['mx']:.3e} f32={r['mx32']:.3e}\t{'ok' if r['ok'] else 'FAIL'}")
        if not r["ok"]:
            fails.append(r)
        if c["name"] == "conv1" and kind == "special":     # a frame of 0.45f is a frame of zeros: relu(b'), padding included
            b32 = DL.fold64(sd, LS[0])[1].float()
            assert torch.equal(c["out"][0], torch.relu(b32).view(64, 1, 1).expand_as(c["out"][0]))
    assert seen == 33 - 3 + 4      # a downsample is judged with its block's second convolution, a skip add before and after the add
    assert not fails, (tag, fails)

    # 3  the chain end to end
    _, _, d64, s64 = DL.twin_tapes(sd, x, torch.float64)
    _, _, d32, s32 = DL.twin_tapes(sd, x, torch.float32)
    for name, hip, ref, f32, floors in [("disparity", hip_disp, d64, d32, (DL.FLOOR_DISP, DL.FLOOR_MAX_RMS))] + \
            [(f"skip {k}", hip_skips[k], s64[k], s32[k], (DL.FLOOR_REL_L2, DL.FLOOR_MAX_RMS)) for k in range(5)]:
        keep = torch.ones_like(ref, dtype=torch.bool)
        if name != "disparity":
            fh, f3 = DL.relu_flips(hip, ref), DL.relu_flips(f32, ref)
            cap = DL.decision_cap(ref.numel())
            _report(f"chain\t{tag}\t{name}\tReLU decisions that differ from float64: hip {int(fh.sum())} f32 {int(f3.sum())} of {ref.numel()} (cap {cap})")
            assert int(fh.sum()) <= cap and int(f3.sum()) <= cap, (tag, name, int(fh.sum()), int(f3.sum()), cap)
            keep = ~(fh | f3)
        for what, fn, floor in (("rel L2", DL.rel_l2, floors[0]), ("max/RMS", DL.max_over_rms, floors[1])):
            e, e32 = fn(hip[keep], ref[keep]), fn(f32[keep], ref[keep])
            _report(f"chain\t{tag}\t{name}\t{what}\thip-f64={e:.3e}\tf32-f64={e32:.3e}\tratio={e / e32 if e32 > 0 else float('nan'):.2f}\tbound={DL.hold(floor, e32):.3e}")
            if not e <= DL.hold(floor, e32):
                fails.append((name, what, e, e32))
    _report(f"time\t{tag}\tGPU part {t_gpu:.1f} s, with the CPU references {time.time() - t0:.1f} s")
    assert not fails, (tag, fails)


def test_the_cases_launch_every_reachable_split():
    """the library's own answer at every case size: together the cases launch all eight k_dn_conv instances, every layer kind in every
    split the rule can give it, and for KW = 1 and KW = 4 a partly filled workgroup and a partly filled wave -- a change of
    dn_split's thresholds that un-covers one of them fails here (and in the case that compares the table)"""
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    inst, part = set(), set()
    for H, W in DL.SIZES:
        net = DepthNetHIP(Engine(H, W, 2), 1)
        LS = DL.layers(H, W)
        for li, (ks, oh, ow, nb, pb, kw) in enumerate(_library_split(net)):
            if li == 0:
                continue
            inst.add((LS[li]["kind"], ks, nb, pb, kw))
            npix = oh * ow
            if npix % (16 * pb * (4 // kw)):
                part.add((kw, "workgroup"))
            if npix % (16 * pb):
                part.add((kw, "wave"))
        net.close()
    assert inst == DL.NEEDED, (inst ^ DL.NEEDED)
    assert {i[1:] for i in inst} == DL.INSTANCES
    assert part == DL.NEEDED_PARTIAL
