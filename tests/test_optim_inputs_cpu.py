"""CPU: the inputs and the judge of the device optimiser's tests (tests/optim_inputs.py) are fair and bite, and the optimiser's entry
points and option are in place.
1. build(seed) is deterministic and has the properties its docstring names.
2. torch's own fp32 Adam / SGD on the CPU pass the judge (the inputs are fair), as does the kernel's arithmetic written in fp32 torch.
3. a deliberately wrong step fails it: the second bias correction left out, or the last element of every tensor never updated.
4. _lib registers the tcsfm_optim_* entry points with the signatures of include/tcsfm.h.
5. DepthOptimizer(options={'fused_step': True}) without weight_tuning is a ValueError.
"""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_inputs as OI  # noqa: E402


@pytest.fixture(scope="module")
def inp():
    return OI.build(0)


def test_builder_is_deterministic_and_as_described(inp):
    again = OI.build(0)
    assert inp["sizes"] == again["sizes"] and torch.equal(inp["p_arena"], again["p_arena"])
    assert all(torch.equal(a, b) for a, b in zip(inp["g_arenas"], again["g_arenas"]))
    assert not torch.equal(inp["p_arena"], OI.build(1)["p_arena"])
    assert inp["sizes"][:len(OI.HEAD_SIZES)] == OI.HEAD_SIZES and len(inp["sizes"]) == len(OI.HEAD_SIZES) + OI.N_SMALL
    assert all(1 <= n <= 97 for n in inp["sizes"][len(OI.HEAD_SIZES):])
    # 4-byte aligned only, every 16-byte phase occurs, and the phase changes from tensor to tensor
    phases = [o % 4 for o in inp["offsets"]]
    assert set(phases) == {0, 1, 2, 3} and sum(a != b for a, b in zip(phases, phases[1:])) > 200
    # the gradients' phase equals the parameters' at steps 1, 3, 5 and differs at steps 2, 4, 6
    for k in range(OI.K):
        same = [go % 4 == o % 4 for go, o in zip(inp["g_offsets"][k], inp["offsets"])]
        assert all(same) if k % 2 == 0 else not any(same)
    g = torch.cat([a for a in inp["g_arenas"]])
    nz = g[g != 0].abs()
    assert float(nz.min()) >= 0.99e-10 and float(nz.max()) <= 1.0 and float((nz * nz).min()) > 1.2e-38
    for k in range(OI.K):
        gs = OI.grads_of(inp, k)
        assert (gs[OI.NONE_TENSOR] is None) == ((k + 1) in OI.NONE_STEPS)
        assert sum(x is None for x in gs) == int((k + 1) in OI.NONE_STEPS)
        assert not bool(gs[OI.BIG_TENSOR][:100].any()) and bool(gs[OI.BIG_TENSOR][100:].any())
        body = torch.cat([x for x in gs if x is not None])
        assert 0.03 < float((body == 0).float().mean()) < 0.07
    assert set(inp["lr"]) == set(OI.LRS)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_torch_fp32_passes_the_judge(inp, kind):
    ref = OI.reference(0, inp, kind)
    for name, run in (("torch fp32", lambda: OI.torch_run(inp, kind, torch.float32)), ("kernel arithmetic", lambda: OI.plain_run(inp, kind))):
        r = OI.judge(inp, kind, ref, *run())
        print(kind, name, "share of the bounds: p %.3f m %.3f v %.3f" % (r["p"], r["m"], r["v"]))
        assert r["ok"], r["failures"][:5]
    assert ref[3][OI.NONE_TENSOR] == OI.K - len(OI.NONE_STEPS) and ref[3][0] == OI.K


@pytest.mark.parametrize("wrong", ["no_bc2", "tail"])
def test_a_wrong_step_fails_the_judge(inp, wrong):
    r = OI.judge(inp, "adam", OI.reference(0, inp, "adam"), *OI.plain_run(inp, "adam", wrong=wrong))
    print(wrong, len(r["failures"]), "failures, first:", r["failures"][:2])
    assert not r["ok"]
    if wrong == "tail":         # every tensor loses exactly its last element: each non-empty one is reported
        assert len({f.split(" ")[1] for f in r["failures"]}) >= len(inp["sizes"]) - 5
    rs = OI.judge(inp, "sgd", OI.reference(0, inp, "sgd"), *OI.plain_run(inp, "sgd", wrong="tail"))
    assert not rs["ok"]


def test_lib_registers_the_optimiser_entry_points():
    import ctypes as C
    from tightly_coupled_sfm_amd import _lib
    names = ("tcsfm_optim_create", "tcsfm_optim_destroy", "tcsfm_optim_step", "tcsfm_optim_snapshot", "tcsfm_optim_restore", "tcsfm_optim_get_state")
    assert set(names) <= set(_lib.EXPORTS)
    assert len(_lib._SIGNATURES["tcsfm_optim_create"][1]) == 6 and len(_lib._SIGNATURES["tcsfm_optim_get_state"][1]) == 5
    assert _lib._SIGNATURES["tcsfm_optim_step"][1][3:] == [C.c_double] * 3 and _lib._SIGNATURES["tcsfm_optim_destroy"][0] is None
    assert (_lib.OPTIM_ADAM, _lib.OPTIM_SGD) == (0, 1)
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n


def test_fused_step_needs_weight_tuning():
    from tightly_coupled_sfm_amd import optimizer as O
    net = torch.nn.Identity()
    with pytest.raises(ValueError, match="fused_step"):
        O.DepthOptimizer({"fused_step": True, "optimize_depth_encoder": True}, {}, net, net, "09_02")
    with pytest.raises(ValueError, match="fused_step"):
        O.DepthOptimizer({"fused_step": True}, {}, net, net, "09_02")
    # with weight_tuning the option is accepted; unset, nothing changes
    assert O.DepthOptimizer({"fused_step": True, "weight_tuning": True, "optimize_depth_encoder": True}, {}, net, net, "09_02").fused_step
    assert not O.DepthOptimizer({"weight_tuning": True, "optimize_depth_encoder": True}, {}, net, net, "09_02").fused_step
