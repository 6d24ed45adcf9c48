"""GPU: ONE launch of each production pose solve kernel -- k_solve, k_solve_lean, the pair role of k_solve_front without and with the
pose-consistency code -- on records and optimiser state given by the test (tcsfm_debug_solve), against exact arithmetic.  Cases, reference,
float64 twin, bounds and judge: tests/solve_exact_inputs.py (their conditions and the planted faults: tests/test_solve_exact_inputs_cpu.py).

Every case: the record sums through the mode-2 export against their derived bound; the step and the new trial transform with
E <= 4 E(float64 twin) + 8 2^-52 max|exact|; lambda, have_cur, the decisions and everything a launch must leave alone bit for bit; the
constants of the next linearisation to 1 ulp32; the emitted pose against the float32 twin of the extraction.  The record-count sweep also
asserts that item 1 of the N = 3 launch is the pair launched alone, bit for bit; accepting launches that their stored system is the mode-2
export of the same records.  The refusals return TCSFM_E_ARG with the message of the check meant and leave every output as it was.  A launch
that wrote outside the entry's device arrays would make the entry return an error (it reads its own guard bands back before freeing).

MEASURED (MI355X; per group of cases the worst ratio E / E(float64 twin) and the largest E of the step d and of the trial transform T, the
worst record-sum error in units of its bound, the worst pose error in units of its bound, the worst constant error in units of its
tolerance; TCSFM_TEST_SOLVE_EXACT_REPORT=<file> writes the line of every case):
    cases                              n  d ratio        E  T ratio        E    sums   pose  const
    sweep v0 np6 dc0                  10        -        -        -        -   0.244      -      -
    sweep v0 np6 dc1                  10        -        -        -        -   0.234      -      -
    sweep v0 np7 dc0                  10        -        -        -        -   0.258      -      -
    sweep v0 np7 dc1                   8        -        -        -        -   0.260      -      -
    sweep v1 np6 dc0                  10        -        -        -        -   0.244      -      -
    sweep v1 np6 dc1                  10        -        -        -        -   0.234      -      -
    sweep v1 np7 dc0                  10        -        -        -        -   0.258      -      -
    sweep v1 np7 dc1                  10        -        -        -        -   0.260      -      -
    sweep v2 np6 dc0                  10        -        -        -        -   0.244      -      -
    sweep v2 np6 dc1                  10        -        -        -        -   0.234      -      -
    sweep v3 np6 dc0                  10        -        -        -        -   0.244      -      -
    sweep v3 np6 dc1                  10        -        -        -        -   0.234      -      -
    solver paths np6                  14     3.49  8.9e-16     2.30  1.5e-15       -  0.248  0.000
    conditioning np6                   8     3.32  2.6e-11     3.55  2.6e-11       -  0.123  0.000
    beyond the judged range np6        1     0.68  4.2e-07     0.68  4.1e-07       -  0.123  0.000
    additive Euler np6                 2     2.46  4.5e-16     1.00  1.4e-15       -  0.176  0.000
    solver paths np7                  16     3.39  1.0e-15     1.40  1.1e-15       -  0.248  0.000
    conditioning np7                   8     1.07  5.8e-12     1.96  2.5e-12       -  0.123  0.000
    beyond the judged range np7        1     0.63  3.5e-07     0.77  1.1e-07       -  0.123  0.000
    additive Euler np7                 2     0.68  3.3e-16     1.39  1.5e-15       -  0.120  0.000
    retraction                        12     2.13  1.8e-16     1.70  2.4e-16       -  0.209  0.000
    pose extraction                    3        -        -        -        -       -  0.250      -
    window rule                        9     2.37  2.9e-16     2.32  2.8e-16   0.202  0.106  0.000
    pose consistency v0                4     6.54  5.9e-17     2.32  1.3e-16       -  0.094  0.000
    pose consistency v3                4     6.54  5.9e-17     2.32  1.3e-16       -  0.094  0.000
    coalesced routing                  4     1.81  2.8e-16     1.45  3.2e-16       -  0.269  0.000
    solver paths v1 np6               14     3.49  4.6e-13     3.55  4.5e-13       -  0.269  0.000
    solver paths v1 np7                9     3.39  2.1e-12     1.12  6.7e-13       -  0.137  0.000
    solver paths v2 np6               14     3.49  4.6e-13     3.55  4.5e-13       -  0.269  0.000
    solver paths v3 np6               14     3.49  4.6e-13     3.55  4.5e-13       -  0.269  0.000
(the last four groups: bookkeeping, conditioning, retraction, routing and window-rule cases of k_solve again on the 1024-thread variants;
their wave-0 arithmetic is the 256-thread kernel's, hence the same figures)
Every variant sums the sweep's records to within a quarter of the bound (the worst entry is at ngrp = 1, where only the roundings of the
assembly remain, hence the same figure in every variant).  The step's ratio to the Cholesky twin stays under the margin of 4 wherever the
twin's own error is above the floor: 3.5 at most (LM accept, 6 unknowns; 3.3 at condition 1e6).  The two ratios above 4 -- 4.9 and 6.5,
pose consistency, unsliced form, it = 1 and 2 -- are steps whose error is 4.4e-17 / 5.9e-17 against a twin that happens to be within 9e-18
of exact there: both are below the floor 8 2^-52 max|d| = 7e-17 .. 3.5e-16 of those pairs, which is what the floor is for; no group needs a
wider margin.  Constants: every
entry of A, kt, R, t the kernel wrote IS the correctly rounded float32 of the exact value (error 0 throughout).  Beyond the judged range
(condition 1e13) kernel and twin both keep 6 to 7 digits.  Under the additive-Euler chart delta_out carries the step of the SE(3) chart
(the lane-parallel solve; its consumer, the dense update, is SE(3) only): it is judged as that, the Euler step through the transform.
"""
import ctypes as C
import os

import numpy as np
import pytest

import solve_exact_inputs as SX

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope="module")
def eng():
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(16, 16, 4)


def _addr(a):
    return None if a is None else a.ctypes.data


def launch(e, c):
    """-> (return code, outputs as SX.new_outputs: filled with the sentinel before the launch, copied back whole)"""
    from tightly_coupled_sfm_amd import _lib
    o = SX.new_outputs(c)
    opts = _lib.default_opts(n_iters=c.n_iters, solver=c.solver, param=c.param, refine=_lib.REFINE_POSE_SCALE if c.np == 7 else _lib.REFINE_POSE,
                             w_dc=c.w_dc, lambda_up=c.lam_up, lambda_down=c.lam_down, lambda_min=c.lam_min, prior_scale=c.prior_scale)
    rec = np.ascontiguousarray(c.rec, np.float32)
    norms = None if c.norms is None else np.ascontiguousarray(c.norms, np.int32)
    a = _lib.DebugSolveArgs()
    a.variant, a.N, a.ngrp, a.mode, a.it, a.n_alloc = c.variant, c.N, c.ngrp, c.mode, c.it, c.n_alloc
    a.rule, a.grp_fwd, a.n_pairs = c.rule, c.grp_fwd, c.n_pairs
    a.norm_n, a.norm_Bt, a.norm_B = (0 if norms is None else norms.shape[0]), c.norm_Bt, c.norm_B
    a.pc_np, a.pc_self0, a.pc_part0, a.pose_lin_pairs = c.pc_np, c.pc_self0, c.pc_part0, (0 if c.pose_lin is None else c.pose_lin.shape[1])
    a.c_ncall, a.c_B, a.c_S, a.c_n0 = c.c_ncall, c.c_B, c.c_S, c.c_n0
    for i in range(c.c_ncall):
        a.c_len[i] = c.c_len[i]
        a.c_pose_out[i] = _addr(o["c_pose_out"][i])
        a.c_ls_out[i] = _addr(o["c_ls_out"][i])
    a.scale_fwd, a.scale_inv, a.w_pc, a.pc_eps = c.scale_fwd, c.scale_inv, c.w_pc, c.pc_eps
    a.records, a.norms, a.state, a.pconst = _addr(rec), _addr(norms), _addr(o["state"]), _addr(o["pconst"])
    for k in SX.ALL_OUT:
        setattr(a, k, _addr(o[k]))
    a.pose_lin = _addr(o["pose_lin"])
    assert C.sizeof(_lib.PairState) == SX.STATE_DT.itemsize and C.sizeof(_lib.PairConst) == SX.CONST_DT.itemsize
    rc = e.debug_solve(opts, a)
    return rc, o


def _run(e):
    def run(c):
        rc, o = launch(e, c)
        assert rc == 0, (c.name, rc, e.last_error())
        return o
    return run


def _report(line):
    path = os.environ.get("TCSFM_TEST_SOLVE_EXACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_struct_layout_is_the_librarys():
    from tightly_coupled_sfm_amd import _lib
    assert _lib.debug_solve_layout() == (C.sizeof(_lib.PairState), C.sizeof(_lib.PairConst)) == (SX.STATE_DT.itemsize, SX.CONST_DT.itemsize)


@pytest.mark.parametrize("name", [c.name for c in SX.all_cases()])
def test_one_launch_against_exact_arithmetic(eng, name):
    c = SX.by_name()[name]
    run = _run(eng)
    out = run(c)
    fails, meas = SX.judge_case(c, lambda _c: out)
    if SX.wants_m8_export(c):
        fails += SX.check_m8_export(c, run, out)
    if "sweep" in c.claims:
        fails += SX.check_alone(c, run)
    line = SX.report_line(c, meas, len(fails))
    print(line)
    _report(line)
    assert not fails, fails[:6]


@pytest.mark.parametrize("what", [n for n, _, _ in SX.refusal_cases()])
def test_refusals_launch_nothing(eng, what):
    c, words = {n: (c, w) for n, c, w in SX.refusal_cases()}[what]
    rc, o = launch(eng, c)
    assert rc == E_ARG, (what, rc)
    assert eng.last_error().startswith("tcsfm_debug_solve: ") and words in eng.last_error(), eng.last_error()       # (the check meant is the one that fired)
    fresh = SX.new_outputs(c)
    for k, v in fresh.items():
        if isinstance(v, list):
            assert all(x is None or np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(o[k], v)), (what, k)
        elif v is not None:
            assert np.array_equal(np.ascontiguousarray(o[k]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), (what, k)
    # the handle is still good: the base case of the refusal's family runs
    ok = SX.by_name()["gn it0 np6"]
    assert launch(eng, ok)[0] == 0


def test_guard_bands_of_the_entrys_own_allocations(eng):
    """The entry frees its device arrays before it returns, so tcsfm_debug_check_guards (live allocations only; the conftest's check after
    every test too) never sees them: the entry reads their bands back itself after the launch and returns an error when one is hit --
    every case above asserts return code 0, and that is what says no launch wrote outside its arrays.  Here: the guards are on, the
    check the entry runs detects a damaged band (the library's self-test damages an allocation of its own and runs that same check over
    it and over an intact one), and the entry leaves no allocation behind."""
    from tightly_coupled_sfm_amd import _lib
    n0, bad0 = _lib.check_guards()
    assert n0 > 0, "the GPU tests run with TCSFM_DEBUG_GUARDS=1 (tests/conftest.py)"
    detected = C.c_int(-2)
    assert _lib.load().tcsfm_debug_guard_selftest(C.byref(detected)) == 0 and detected.value == 1
    assert launch(eng, SX.by_name()["sweep v1 np7 dc1 ngrp259"])[0] == 0
    n1, bad1 = _lib.check_guards()
    assert bad0 == 0 and bad1 == 0 and n0 == n1
