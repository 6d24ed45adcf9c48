"""The backward passes of disp_to_depth, SSIM_Loss and get_smooth_loss on the GPU -- tcsfm_disp_to_depth_backward, tcsfm_ssim_backward,
tcsfm_smooth_loss_device, tcsfm_smooth_loss_backward, their Engine wrappers and the three drop-ins under autograd -- against autograd
in float64 through the reference's expressions (tests/loss_grad_inputs.py holds the cases, the masks, the cotangents and the judge;
tests/test_loss_grad_inputs_cpu.py checks them without a GPU).  Every tensor of every item is held to 4 x the float32 twin's own error
(relative L2 and max error over RMS), to exact zeros where float64 is exactly zero and to a relative L2 below 1e-4.

The smallest frame here is 4 x 4: a handle cannot be created below that (tests/test_abi_cpu.py), so the 2 x 2 case of the inputs module
is checked at the level of the closed forms only, and the smooth loss's own "image too small" refusal cannot be reached.

TCSFM_TEST_LOSS_GRAD_REPORT=<file> keeps one line per tensor and item, and one per case with the worst ratio and the largest
relative L2 (the table of DESIGN.md section 4 is made from it).
"""
import ctypes as C
import os

import numpy as np
import pytest

import loss_grad_inputs as LG

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PG = LG.PG
GPU_IDS = [LG.IDS[LG.CASES.index(c)] for c in LG.GPU_CASES]
RANGE = (LG.MIN_DEPTH, LG.MAX_DEPTH)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(line):
    print(line)
    f = os.environ.get("TCSFM_TEST_LOSS_GRAD_REPORT")
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _engine(case):
    from tightly_coupled_sfm_amd.engine import Engine
    H, W, N = case
    return Engine(H, W, N)


def _judge(got, ref, t32, tag, tensors):
    fails, worst = LG.judge(got, ref, t32, tag, tensors, _report)
    _report(f"{tag}\tworst ratio to the float32 twin | largest relative L2\t" + "\t".join(f"{k}={v[0]:.3f}|{v[1]:.2e}" for k, v in worst.items()))
    assert not fails, fails


def _d2d(e, disp, cot, subset=LG.D2D_COTS):
    g = {k: (cot[k] if k in subset else None) for k in LG.D2D_COTS}
    return dict(g_disp=_np(e.disp_to_depth_backward(disp, *RANGE, g["g_scaled"], g["g_depth"])))


def _ssim(e, x, y, g, want=LG.SSIM_OUTS):
    out = e.ssim_loss_backward(x, y, g, tuple(k in want for k in LG.SSIM_OUTS))
    return dict(zip(LG.SSIM_OUTS, (_np(o) for o in out)))


def _smooth(e, disp, img, g=LG.SMOOTH_G):
    loss, stats = e.smooth_loss_device(disp, img)
    return dict(g_disp=_np(e.smooth_loss_backward(disp, img, stats, torch.tensor(g, device="cuda"))), loss=_np(loss), stats=_np(stats))


@pytest.mark.parametrize("case", LG.GPU_CASES, ids=GPU_IDS)
def test_disp_to_depth_backward_against_float64(case):
    """both cotangents, and each alone below the production size (the absent one is passed as NULL)"""
    disp, cot = _t(LG.make_disp(case)), {k: _t(v) for k, v in LG.d2d_cotangents(case).items()}
    e = _engine(case)
    for subset in (LG.D2D_SUBSETS if case != LG.LARGE else LG.D2D_SUBSETS[:1]):
        _judge(_d2d(e, disp, cot, subset), LG.twin_d2d(case, subset), LG.twin_d2d(case, subset, "f32"), f"{LG.IDS[LG.CASES.index(case)]}/disp_to_depth/{'+'.join(subset)}", ("g_disp",))
    e.close()


@pytest.mark.parametrize("case", LG.GPU_CASES, ids=GPU_IDS)
def test_ssim_backward_against_float64(case):
    """g_x and g_y together, and each alone below the production size (the other is None)"""
    x, y = (_t(a) for a in LG.make_ssim(case))
    g = _t(LG.ssim_cotangent(case))
    ref, t32 = LG.twin_ssim(case), LG.twin_ssim(case, "f32")
    e = _engine((case[0], case[1], case[2] * LG.SSIM_C))
    for want in (LG.SSIM_WANTS if case != LG.LARGE else LG.SSIM_WANTS[:1]):
        got = _ssim(e, x, y, g, want)
        assert all((got[k] is None) == (k not in want) for k in LG.SSIM_OUTS)
        _judge(got, ref, t32, f"{LG.IDS[LG.CASES.index(case)]}/ssim/{'+'.join(want)}", want)
    e.close()


@pytest.mark.parametrize("case", LG.GPU_CASES, ids=GPU_IDS)
def test_smooth_loss_device_and_backward_against_float64(case):
    """the scalar on the device is within one float32 ulp of the plain call's value; stats hold the mean and the per-image sums; the
    gradient against float64 (one scalar cotangent: nothing is masked, the CPU test vouches for the inputs)"""
    H, W, N = case
    disp, img = _t(LG.make_disp(case)), _t(LG.make_img(case))
    e = _engine(case)
    got = _smooth(e, disp, img)
    plain = e.smooth_loss(disp, img)
    assert isinstance(plain, float)
    ulp = float(np.spacing(np.float32(abs(plain))))
    _report(f"{LG.IDS[LG.CASES.index(case)]}/smooth\tdevice={float(got['loss']):.9e}\tplain={plain:.9e}\tulp={ulp:.2e}")
    assert got["loss"].dtype == np.float32 and got["loss"].shape == () and abs(float(got["loss"]) - plain) <= ulp
    d64 = LG.make_disp(case).astype(np.float64)
    assert np.allclose(got["stats"][:, 0], d64.mean((1, 2, 3)), rtol=1e-14, atol=0)
    Nx, Ny = N * H * (W - 1), N * (H - 1) * W
    assert abs((got["stats"][:, 1].sum() / Nx + got["stats"][:, 2].sum() / Ny) - plain) <= 1e-12 * abs(plain)
    _judge(got, LG.twin_smooth(case), LG.twin_smooth(case, "f32"), f"{LG.IDS[LG.CASES.index(case)]}/smooth", ("g_disp",))
    e.close()


@pytest.mark.parametrize("case", LG.GPU_CASES, ids=GPU_IDS)
def test_bits(case):
    """the same call twice gives the same bits; an output requested alone has the bits of the all-outputs call; item n of a batch has
    the bits of a one-item call.  For the smooth loss stats[n] has the one-item call's bits, and g_disp[n] times N is the one-item
    gradient: the 1 / N sits inside Nx and Ny, two roundings in double before the one to float32, so bit equality is not guaranteed
    there -- MARGIN float32 ulps are allowed and the report line says whether the bits were equal."""
    H, W, N = case
    disp, img, cot = _t(LG.make_disp(case)), _t(LG.make_img(case)), {k: _t(v) for k, v in LG.d2d_cotangents(case).items()}
    x, y = (_t(a) for a in LG.make_ssim(case))
    g = _t(LG.ssim_cotangent(case))
    e = _engine((H, W, N * LG.SSIM_C))
    d1, s1, m1 = _d2d(e, disp, cot), _ssim(e, x, y, g), _smooth(e, disp, img)
    d2, s2, m2 = _d2d(e, disp, cot), _ssim(e, x, y, g), _smooth(e, disp, img)
    assert _same(d1["g_disp"], d2["g_disp"]) and all(_same(s1[k], s2[k]) for k in LG.SSIM_OUTS)
    assert all(_same(m1[k], m2[k]) for k in ("g_disp", "loss", "stats"))
    for k in LG.SSIM_OUTS:
        alone = _ssim(e, x, y, g, (k,))
        assert _same(alone[k], s1[k]), ("alone", k)
    for n in sorted({0, N - 1}):
        one = lambda t: t[n:n + 1].contiguous()
        assert _same(_d2d(e, one(disp), {k: one(v) for k, v in cot.items()})["g_disp"][0], d1["g_disp"][n]), ("item", n)
        so = _ssim(e, one(x), one(y), one(g))
        assert all(_same(so[k][0], s1[k][n]) for k in LG.SSIM_OUTS), ("item", n)
        mo = _smooth(e, one(disp), one(img))
        assert _same(mo["stats"][0], m1["stats"][n]), ("item", n)
        scaled = m1["g_disp"][n].astype(np.float64) * N
        equal = np.array_equal(scaled, mo["g_disp"][0].astype(np.float64))
        _report(f"{LG.IDS[LG.CASES.index(case)]}/bits\tsmooth g_disp[{n}] x N against the one-item call: {'bit-equal' if equal else 'within MARGIN float32 ulps'}")
        assert (np.abs(scaled - mo["g_disp"][0]) <= LG.MARGIN * np.spacing(np.abs(mo["g_disp"][0]))).all(), ("item", n)
    e.close()


def test_host_pointers_and_refusals():
    """numpy arrays through the C ABI (opts.host_ptrs) give the device call's bits; NULL arguments, a missing cotangent or output and
    a bad N are refused; a frame too small for the smooth loss is refused where the handle is created"""
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    case = (17, 33, 3)
    H, W, N = case
    disp, img, cot = LG.make_disp(case), LG.make_img(case), LG.d2d_cotangents(case)
    x, y = LG.make_ssim(case)
    g = LG.ssim_cotangent(case)
    e = _engine((H, W, N * LG.SSIM_C))
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    lib, h = e.lib, e._h
    o = default_opts(host_ptrs=1, min_depth=RANGE[0], max_depth=RANGE[1])
    dev_d = _d2d(e, _t(disp), {k: _t(v) for k, v in cot.items()}, ("g_depth",))
    out = np.full(disp.shape, np.nan, np.float32)
    e._call(lib.tcsfm_disp_to_depth_backward(h, C.byref(o), disp.size, P(disp), None, P(cot["g_depth"]), P(out)))
    assert _same(out, dev_d["g_disp"])
    dev_s = _ssim(e, _t(x), _t(y), _t(g))
    gx, gy = np.full(x.shape, np.nan, np.float32), np.full(x.shape, np.nan, np.float32)
    e._call(lib.tcsfm_ssim_backward(h, C.byref(o), N * LG.SSIM_C, P(x), P(y), P(g), P(gx), P(gy)))
    assert _same(gx, dev_s["g_x"]) and _same(gy, dev_s["g_y"])
    dev_m = _smooth(e, _t(disp), _t(img))
    loss, stats, gd = np.full(1, np.nan, np.float32), np.full((N, 3), np.nan), np.full(disp.shape, np.nan, np.float32)
    gl = np.array([LG.SMOOTH_G], np.float32)
    e._call(lib.tcsfm_smooth_loss_device(h, C.byref(o), N, P(disp), P(img), P(loss), P(stats)))
    e._call(lib.tcsfm_smooth_loss_backward(h, C.byref(o), N, P(disp), P(img), P(stats), P(gl), P(gd)))
    assert _same(loss[0], dev_m["loss"]) and _same(stats, dev_m["stats"]) and _same(gd, dev_m["g_disp"])
    E_ARG = -1
    od = default_opts(min_depth=RANGE[0], max_depth=RANGE[1])
    D = {k: _t(v) for k, v in dict(disp=disp, img=img, gs=cot["g_scaled"], x=x, y=y, g=g).items()}
    o1, o2 = torch.empty_like(D["disp"]), torch.empty_like(D["x"])
    st, ls, gl_d = torch.zeros((N, 3), dtype=torch.float64, device="cuda"), torch.zeros((), device="cuda"), torch.ones((), device="cuda")
    p = e._p
    assert lib.tcsfm_disp_to_depth_backward(h, C.byref(od), disp.size, p(D["disp"]), p(D["gs"]), None, p(o1)) == 0
    assert lib.tcsfm_disp_to_depth_backward(h, C.byref(od), disp.size, p(D["disp"]), None, None, p(o1)) == E_ARG          # no cotangent
    assert lib.tcsfm_disp_to_depth_backward(h, C.byref(od), disp.size, None, p(D["gs"]), None, p(o1)) == E_ARG
    assert lib.tcsfm_disp_to_depth_backward(h, C.byref(od), disp.size, p(D["disp"]), p(D["gs"]), None, None) == E_ARG
    assert lib.tcsfm_disp_to_depth_backward(h, C.byref(od), 0, p(D["disp"]), p(D["gs"]), None, p(o1)) == E_ARG
    assert lib.tcsfm_ssim_backward(h, C.byref(od), N * LG.SSIM_C, p(D["x"]), p(D["y"]), p(D["g"]), None, p(o2)) == 0
    assert lib.tcsfm_ssim_backward(h, C.byref(od), N * LG.SSIM_C, p(D["x"]), p(D["y"]), p(D["g"]), None, None) == E_ARG      # no output
    assert lib.tcsfm_ssim_backward(h, C.byref(od), N * LG.SSIM_C, p(D["x"]), None, p(D["g"]), None, p(o2)) == E_ARG
    assert lib.tcsfm_ssim_backward(h, C.byref(od), N * LG.SSIM_C, p(D["x"]), p(D["y"]), None, None, p(o2)) == E_ARG
    assert lib.tcsfm_ssim_backward(h, C.byref(od), 0, p(D["x"]), p(D["y"]), p(D["g"]), None, p(o2)) == E_ARG
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), N, p(D["disp"]), p(D["img"]), p(ls), p(st)) == 0
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), N, p(D["disp"]), p(D["img"]), None, p(st)) == E_ARG
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), N, p(D["disp"]), p(D["img"]), p(ls), None) == E_ARG
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), N, None, p(D["img"]), p(ls), p(st)) == E_ARG
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), e.max_pairs + 1, p(D["disp"]), p(D["img"]), p(ls), p(st)) == E_ARG   # bad N
    assert lib.tcsfm_smooth_loss_device(h, C.byref(od), 0, p(D["disp"]), p(D["img"]), p(ls), p(st)) == E_ARG
    assert lib.tcsfm_smooth_loss_backward(h, C.byref(od), N, p(D["disp"]), p(D["img"]), p(st), p(gl_d), p(o1)) == 0
    assert lib.tcsfm_smooth_loss_backward(h, C.byref(od), N, p(D["disp"]), p(D["img"]), None, p(gl_d), p(o1)) == E_ARG
    assert lib.tcsfm_smooth_loss_backward(h, C.byref(od), N, p(D["disp"]), p(D["img"]), p(st), None, p(o1)) == E_ARG
    assert lib.tcsfm_smooth_loss_backward(h, C.byref(od), N, p(D["disp"]), p(D["img"]), p(st), p(gl_d), None) == E_ARG
    assert lib.tcsfm_smooth_loss_backward(h, C.byref(od), e.max_pairs + 1, p(D["disp"]), p(D["img"]), p(st), p(gl_d), p(o1)) == E_ARG
    torch.cuda.synchronize()
    e.close()
    with pytest.raises(RuntimeError, match="sizes"):          # H or W below 2 never reaches tcsfm_smooth_loss_device: no such handle
        Engine(1, 9, 1)


def test_autograd_drop_ins():
    """learning_helpers.disp_to_depth, losses.SSIM_Loss and losses.get_smooth_loss with leaves that require grad: the plain call's
    bits forward (the smooth loss: a 0-dim float32 device tensor within one ulp), a grad_fn only when required and never under
    no_grad, backward() with the bits of the direct Engine call, only one of x and y, an absent cotangent, img requiring grad raises"""
    from tightly_coupled_sfm_amd import learning_helpers, losses
    from tightly_coupled_sfm_amd._shared import get_engine
    case = (17, 33, 3)
    H, W, N = case
    disp, img, cot = _t(LG.make_disp(case)), _t(LG.make_img(case)), {k: _t(v) for k, v in LG.d2d_cotangents(case).items()}
    x, y = (_t(a) for a in LG.make_ssim(case))
    g = _t(LG.ssim_cotangent(case))
    e = get_engine(H, W, N * LG.SSIM_C)
    ssim = losses.SSIM_Loss()
    # plain and no_grad: no grad_fn, today's types
    ps, pz = learning_helpers.disp_to_depth(disp, *RANGE)
    pv = ssim(x, y)
    pl = losses.get_smooth_loss(disp, img)
    assert all(t.grad_fn is None and not t.requires_grad for t in (ps, pz, pv, pl))
    with torch.no_grad():
        leaf = disp.clone().requires_grad_()
        q = (*learning_helpers.disp_to_depth(leaf, *RANGE), ssim(leaf.repeat(1, 2, 1, 1), y), losses.get_smooth_loss(leaf, img))
    assert all(t.grad_fn is None for t in q)
    assert _same(_np(q[0]), _np(ps)) and _same(_np(q[1]), _np(pz)) and _same(_np(q[3]), _np(pl))
    # disp_to_depth
    direct = e.disp_to_depth_backward(disp, *RANGE, cot["g_scaled"], cot["g_depth"])
    leaf = disp.clone().requires_grad_()
    s, z = learning_helpers.disp_to_depth(leaf, *RANGE)
    assert s.grad_fn is not None and z.grad_fn is not None and _same(_np(s), _np(ps)) and _same(_np(z), _np(pz))
    ((s * cot["g_scaled"]).sum() + (z * cot["g_depth"]).sum()).backward()
    assert _same(_np(leaf.grad), _np(direct))
    leaf = disp.clone().requires_grad_()
    (learning_helpers.disp_to_depth(leaf, *RANGE)[1] * cot["g_depth"]).sum().backward()          # the cotangent of scaled_disp is absent
    assert _same(_np(leaf.grad), _np(e.disp_to_depth_backward(disp, *RANGE, None, cot["g_depth"])))
    # SSIM_Loss
    dx, dy = e.ssim_loss_backward(x, y, g)
    for req in ((True, True), (True, False), (False, True)):
        lx, ly = x.clone().requires_grad_(req[0]), y.clone().requires_grad_(req[1])
        v = ssim(lx, ly)
        assert v.grad_fn is not None and _same(_np(v), _np(pv))
        (v * g).sum().backward()
        for leaf, rq, ref in ((lx, req[0], dx), (ly, req[1], dy)):
            assert (leaf.grad is None) == (not rq)
            if rq:
                assert _same(_np(leaf.grad), _np(ref)), req
    # get_smooth_loss
    loss, stats = e.smooth_loss_device(disp, img)
    direct = e.smooth_loss_backward(disp, img, stats, torch.tensor(LG.SMOOTH_G, device="cuda"))
    leaf = disp.clone().requires_grad_()
    L = losses.get_smooth_loss(leaf, img)
    assert L.grad_fn is not None and L.is_cuda and L.dim() == 0 and L.dtype == torch.float32
    assert _same(_np(L), _np(loss)) and abs(float(L.detach()) - float(pl)) <= float(np.spacing(np.float32(abs(float(pl)))))
    (L * LG.SMOOTH_G).backward()
    assert _same(_np(leaf.grad), _np(direct))
    assert isinstance(e.smooth_loss(disp, img), float)
    with pytest.raises(NotImplementedError, match="DESIGN"):
        losses.get_smooth_loss(disp, img.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="DESIGN"):
        losses.get_smooth_loss(disp.clone().requires_grad_(), img.clone().requires_grad_())


def test_end_to_end_optimization_loss():
    """17 x 33, B = 1, S = 2: a disparity leaf per frame -> learning_helpers.disp_to_depth -> helpers.compute_photometric_error for
    the forward and the inverse pairs -> losses.compute_optimization_loss (no argmin; inverse reconstruction, depth consistency,
    l_depth_init with SSIM_Loss() and l_smooth on) -> backward().  The library's masks go detached into the float64 and float32
    twins; the disparity gradients are held to 4 x the float32 twin's error.  (Fails before the feature: the leaves' .grad is None.)"""
    from tightly_coupled_sfm_amd import helpers, learning_helpers, losses
    i = {k: _t(v) for k, v in LG.e2e_inputs().items()}
    disp_t, disp_s = i["disp_t"].clone().requires_grad_(), i["disp_s"].clone().requires_grad_()
    depth_t, depth_s = (learning_helpers.disp_to_depth(d, *LG.E2E_DEPTH_RANGE)[1] for d in (disp_t, disp_s))
    tgt2, dt2 = i["tgt"].repeat(2, 1, 1, 1), depth_t.repeat(2, 1, 1, 1)
    fwd = helpers.compute_photometric_error(tgt2, i["src"], dt2, depth_s, i["pose"], i["K"])
    inv = helpers.compute_photometric_error(i["src"], tgt2, depth_s, dt2, -i["pose"], i["K"])
    masks = dict(fwd_valid=_np(fwd["valid_mask"]), inv_valid=_np(inv["valid_mask"]))
    assert masks["fwd_valid"].sum() > 0 and masks["inv_valid"].sum() > 0
    L = losses.compute_optimization_loss(LG.E2E_OPTIONS, i["tgt"], disp_t, i["disp_init"], fwd, inv, losses.SSIM_Loss())
    L.backward()
    assert disp_t.grad is not None and disp_s.grad is not None
    got = dict(d_disp_t=_np(disp_t.grad), d_disp_s=_np(disp_s.grad))
    (ref, L64), (t32, _) = LG.e2e_twin(masks), LG.e2e_twin(masks, "f32")
    _report(f"17x33-B1-S2/end_to_end\tloss={float(L.detach()):.9e}\tfloat64 twin={L64:.9e}")
    assert abs(float(L.detach()) - L64) < 1e-3 * abs(L64)          # (the suite's absolute floors for diff and weight, 3e-5 and 1e-4, on a loss of order 0.1)
    fails, worst = LG.judge(got, ref, t32, "17x33-B1-S2/end_to_end", LG.E2E_TENSORS, _report, None)
    _report("17x33-B1-S2/end_to_end\tworst ratio to the float32 twin | largest relative L2\t" + "\t".join(f"{k}={v[0]:.3f}|{v[1]:.2e}" for k, v in worst.items()))
    assert not fails, fails
