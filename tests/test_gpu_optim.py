"""GPU: the device optimiser (csrc/optim_kernel.h, tcsfm_optim_*, optim.LibraryOptimizer) on the inputs and under the judge of
tests/optim_inputs.py: 314 tensors of every size class in one 4-byte-aligned arena, K = 6 steps, two learning rates, one tensor without
a gradient at steps 2 and 4, gradients whose 16-byte phase differs from the parameters' at every other step.

1. Adam and SGD through the C ABI, a synchronisation after every step: parameters, moments (tcsfm_optim_get_state) and step counts
   against torch.optim on float64 within the judge's bounds; the floats around the arena keep their sentinel.
2. the same with steps 3 and 4 issued back to back (different gradient buffers, no synchronisation between them, and none around
   them): the same bits as run 1, which is also the second run from the same inputs.
3. snapshot, two steps, restore: the snapshot's bits, zero moments, step 0, and the next step is a fresh optimiser's first step.
4. the refusals of include/tcsfm.h return TCSFM_E_ARG with a message.
5. LibraryOptimizer: step() and restore() bump _version, state() is the C ABI's, and a DepthNetModule's forward after a step uses the
   new weights: the bits of a module freshly built from the updated state_dict (32 x 64, N = 1).
The guard-band fixture of conftest.py covers the optimiser's own arenas and tables in every test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_inputs as OI  # noqa: E402

SENTINEL = 12345.0
E_ARG = -1


@pytest.fixture(scope="module")
def eng():
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(32, 32, 1)


@pytest.fixture(scope="module")
def inp():
    return OI.build(0)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Run:
    """the inputs on the device and an optimiser over them, driven through the C ABI"""

    def __init__(self, eng, inp, kind):
        from tightly_coupled_sfm_amd import _lib
        self.eng, self.lib, self.inp, self.kind = eng, eng.lib, inp, kind
        arena = inp["p_arena"].clone()
        self.total = inp["offsets"][-1] + inp["sizes"][-1]
        arena[0] = SENTINEL
        arena[self.total:] = SENTINEL
        self.arena = arena.cuda()
        self.params = OI.params_of(inp, self.arena)
        self.g_arenas = [a.cuda() for a in inp["g_arenas"]]
        self.n = n = len(self.params)
        self.dummy = torch.zeros(4, device="cuda")
        ptrs = (C.c_void_p * n)(*[(p.data_ptr() or None) for p in self.params])
        numel = (C.c_int64 * n)(*inp["sizes"])
        self.o = C.c_void_p()
        eng._bind()
        eng._call(self.lib.tcsfm_optim_create(eng._h, _lib.OPTIM_ADAM if kind == "adam" else _lib.OPTIM_SGD, n, ptrs, numel, C.byref(self.o)))
        self.lr = (C.c_double * n)(*inp["lr"])

    def close(self):
        if self.o:
            self.lib.tcsfm_optim_destroy(self.o)
            self.o = None

    def step(self, k):
        gs = OI.grads_of(self.inp, k, self.g_arenas[k])
        # (an empty tensor has no data pointer: its gradient is signalled by any non-NULL address, include/tcsfm.h)
        gp = (C.c_void_p * self.n)(*[(None if g is None else (g.data_ptr() if g.numel() else self.dummy.data_ptr())) for g in gs])
        self.eng._call(self.lib.tcsfm_optim_step(self.o, gp, self.lr, OI.BETAS[0], OI.BETAS[1], OI.EPS))

    def state(self):
        """-> params, exp_avg, exp_avg_sq (CPU), step counts; exp_avg of even tensors through a HOST pointer, of odd ones through a device one"""
        ps = [p.detach().cpu().clone() for p in self.params]
        ms, vs, counts = [], [], []
        for i, p in enumerate(self.params):
            st = C.c_int64(-1)
            m = v = None
            if self.kind == "adam":
                m = np.zeros(p.numel(), dtype=np.float32) if i % 2 == 0 else torch.zeros_like(p)
                v = torch.zeros_like(p)
                mp = (m.ctypes.data if i % 2 == 0 else m.data_ptr()) if p.numel() else None
                self.eng._call(self.lib.tcsfm_optim_get_state(self.o, i, C.c_void_p(mp) if mp else None, C.c_void_p(v.data_ptr()) if p.numel() else None, C.byref(st)))
                m = torch.from_numpy(m) if i % 2 == 0 else m.cpu()
                v = v.cpu()
            else:
                self.eng._call(self.lib.tcsfm_optim_get_state(self.o, i, None, None, C.byref(st)))
            ms.append(m); vs.append(v); counts.append(int(st.value))
        return ps, ms, vs, counts

    def sentinels_intact(self):
        a = self.arena.cpu()
        return float(a[0]) == SENTINEL and bool((a[self.total:] == SENTINEL).all())


def _run(eng, inp, kind, back_to_back):
    r = _Run(eng, inp, kind)
    try:
        for k in range(OI.K):
            r.step(k)
            if not back_to_back:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out = r.state()
        assert r.sentinels_intact()
        return out
    finally:
        r.close()


_RESULTS = {}


def _result(eng, inp, kind, back_to_back=False):
    key = (kind, back_to_back)
    if key not in _RESULTS:
        _RESULTS[key] = _run(eng, inp, kind, back_to_back)
    return _RESULTS[key]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_steps_against_float64(eng, inp, kind):
    ps, ms, vs, counts = _result(eng, inp, kind)
    r = OI.judge(inp, kind, OI.reference(0, inp, kind), ps, ms, vs, counts)
    print(kind, "share of the bounds: p %.3f m %.3f v %.3f" % (r["p"], r["m"], r["v"]))
    assert r["ok"], r["failures"][:8]
    assert counts[OI.NONE_TENSOR] == OI.K - len(OI.NONE_STEPS) and counts[0] == OI.K and counts[1] == OI.K
    moved = sum(not _bits_equal(p, p0) for p, p0 in zip(ps, OI.params_of(inp)))
    assert moved == len([n for n in inp["sizes"] if n])


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_back_to_back_steps_and_reproducibility(eng, inp, kind):
    """no synchronisation between any two steps (steps 3 and 4 among them, with different gradient buffers and, for tensor NONE_TENSOR, a
    gradient at one and none at the other; six steps in flight also wrap the ring of per-step tables): judged as above, and bit-identical
    to the run that synchronises after every step"""
    a = _result(eng, inp, kind)
    b = _result(eng, inp, kind, back_to_back=True)
    r = OI.judge(inp, kind, OI.reference(0, inp, kind), *b)
    assert r["ok"], r["failures"][:8]
    assert a[3] == b[3]
    for x, y in zip(a[0], b[0]):
        assert _bits_equal(x, y)
    if kind == "adam":
        for k in (1, 2):
            for x, y in zip(a[k], b[k]):
                assert _bits_equal(x, y)


def test_snapshot_restore(eng, inp):
    r, fresh = _Run(eng, inp, "adam"), _Run(eng, inp, "adam")
    try:
        assert r.lib.tcsfm_optim_restore(r.o) == E_ARG and b"snapshot" in r.lib.tcsfm_last_error(eng._h)
        r.step(0)
        eng._call(r.lib.tcsfm_optim_snapshot(r.o))         # a snapshot of moved parameters: restore must not go back to the inputs
        snap = [p.detach().clone() for p in r.params]
        r.step(1); r.step(2)
        assert not _bits_equal(r.params[5], snap[5])
        eng._call(r.lib.tcsfm_optim_restore(r.o))
        ps, ms, vs, counts = r.state()
        assert all(_bits_equal(p, s.cpu()) for p, s in zip(ps, snap))
        assert counts == [0] * r.n
        assert all(not bool(m.any()) and not bool(v.any()) for m, v in zip(ms, vs))
        # the next step is a fresh optimiser's first step from the same values
        fresh.arena.copy_(r.arena)
        r.step(3); fresh.step(3)
        a, b = r.state(), fresh.state()
        assert a[3] == b[3] and a[3][0] == 1 and a[3][OI.NONE_TENSOR] == 0
        for k in range(3):
            assert all(_bits_equal(x, y) for x, y in zip(a[k], b[k]))
        assert any(not _bits_equal(p, s.cpu()) for p, s in zip(a[0], snap))
        assert r.sentinels_intact() and fresh.sentinels_intact()
    finally:
        r.close(); fresh.close()


def test_refusals(eng):
    from tightly_coupled_sfm_amd import _lib
    lib = eng.lib
    buf = torch.zeros(16, device="cuda")
    o = C.c_void_p()

    def create(kind, n, ptrs, numel):
        o.value = None
        rc = lib.tcsfm_optim_create(eng._h, kind, n, (C.c_void_p * len(ptrs))(*ptrs), (C.c_int64 * len(numel))(*numel), C.byref(o))
        return rc, lib.tcsfm_last_error(eng._h).decode()

    for what, args in (("n < 1", (_lib.OPTIM_ADAM, 0, [buf.data_ptr()], [4])), ("NULL parameter", (_lib.OPTIM_ADAM, 2, [buf.data_ptr(), None], [4, 4])),
                       ("negative numel", (_lib.OPTIM_SGD, 1, [buf.data_ptr()], [-1])), ("unknown kind", (7, 1, [buf.data_ptr()], [4])),
                       ("misaligned", (_lib.OPTIM_ADAM, 1, [buf.data_ptr() + 2], [4]))):
        rc, msg = create(*args)
        print(what, "->", rc, msg)
        assert rc == E_ARG and msg.startswith("tcsfm_optim_create") and not o.value, what
    # numel = 0 is legal (with a NULL pointer too) and does nothing; an SGD optimiser has no moments to hand out
    rc, _ = create(_lib.OPTIM_SGD, 2, [None, buf.data_ptr()], [0, 16])
    assert rc == 0 and o.value
    try:
        g = torch.ones(16, device="cuda")
        eng._call(lib.tcsfm_optim_step(o, (C.c_void_p * 2)(g.data_ptr(), g.data_ptr()), (C.c_double * 2)(0.5, 0.5), 0.9, 0.999, 1e-8))
        torch.cuda.synchronize()
        assert torch.equal(buf, torch.full_like(buf, -0.5))
        st = C.c_int64()
        assert lib.tcsfm_optim_get_state(o, 1, C.c_void_p(g.data_ptr()), None, C.byref(st)) == E_ARG
        assert lib.tcsfm_optim_get_state(o, 2, None, None, C.byref(st)) == E_ARG
        assert lib.tcsfm_optim_get_state(o, 0, None, None, C.byref(st)) == 0 and st.value == 1
        assert lib.tcsfm_optim_restore(o) == E_ARG and "snapshot" in lib.tcsfm_last_error(eng._h).decode()
    finally:
        lib.tcsfm_optim_destroy(o)


def test_library_optimizer_and_module_reload():
    import depthnet_twin as dt
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    from tightly_coupled_sfm_amd.optim import LibraryOptimizer
    torch.manual_seed(3)
    model = DepthNetModule(dt.depthnet_params(0), max_images=1).cuda()
    x = torch.rand(1, 3, 32, 64, device="cuda")
    with torch.no_grad():
        d0 = model(x=x)[0][0].clone()
    enc = list(model.encoder.parameters())
    opt = LibraryOptimizer([{"params": enc[:10], "lr": 1e-2}, {"params": enc[10:]}], kind="adam", lr=2e-4)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 2e-4] and sum(len(g["params"]) for g in opt.param_groups) == len(enc)
    opt.snapshot()
    before = [p.detach().clone() for p in enc]
    for p in enc[:-1]:
        p.grad = torch.randn_like(p)
    enc[0].grad = torch.randn(tuple(enc[0].shape)[::-1], device="cuda").permute(3, 2, 1, 0)      # not contiguous: made so by step()
    assert not enc[0].grad.is_contiguous()
    versions = [p._version for p in enc]
    opt.step()
    assert all(p._version > v for p, v in zip(enc[:-1], versions)) and enc[-1]._version == versions[-1]
    assert all(not _bits_equal(p.detach(), b) for p, b in zip(enc[:-1], before)) and _bits_equal(enc[-1].detach(), before[-1])
    # Adam's first step moves every element with a gradient by lr (m / sqrt(v) = +-1 up to eps)
    assert float((enc[0].detach() - before[0]).abs().max()) == pytest.approx(1e-2, rel=1e-3)
    st = opt.state(enc[0])
    assert st["step"] == 1 and opt.state(enc[-1])["step"] == 0
    assert torch.allclose(st["exp_avg"], 0.1 * enc[0].grad, rtol=1e-5, atol=0) and torch.allclose(st["exp_avg_sq"], 0.001 * enc[0].grad ** 2, rtol=1e-5, atol=0)
    # the module's next forward uses the new weights: the bits of a module freshly built from the updated state_dict
    with torch.no_grad():
        d1 = model(x=x)[0][0].clone()
        fresh = DepthNetModule({k: v.detach().cpu() for k, v in model.state_dict().items()}, max_images=1).cuda()
        d2 = fresh(x=x)[0][0]
    assert _bits_equal(d1, d2) and not _bits_equal(d1, d0)
    native = dict(model._native)
    opt.zero_grad()
    assert all(p.grad is None for p in enc)
    versions = [p._version for p in enc]
    opt.restore()
    assert all(p._version > v for p, v in zip(enc, versions))
    assert all(_bits_equal(p.detach(), b) for p, b in zip(enc, before)) and opt.state(enc[0])["step"] == 0
    with torch.no_grad():
        assert _bits_equal(model(x=x)[0][0], d0)
    assert all(model._native[k] is v for k, v in native.items()) and len(model._native) == len(native)
    with pytest.raises(ValueError):
        LibraryOptimizer([enc[0].detach().cpu()])
    with pytest.raises(ValueError):
        LibraryOptimizer([enc[0], enc[0]])
