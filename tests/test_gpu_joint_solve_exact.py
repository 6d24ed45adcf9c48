"""GPU: ONE launch of each production joint solve kernel -- k_solve_joint<NS>, the joint role of k_solve_front<NS> / <NS, PC>, both roles of
k_solve_joint2<NS> / <NS, PC> -- on records and optimiser state given by the test (tcsfm_debug_solve_joint), against exact arithmetic.  Cases,
reference, float64 stand-in and twins, bounds and judge: tests/joint_solve_exact_inputs.py (their conditions and the planted faults:
tests/test_joint_solve_exact_inputs_cpu.py).

Every case: the record sums (through the export, the split partials in jpart and the stored system of accepted steps) against their derived
bound; the step and the trial transforms with E <= 4 E_env + 8 2^-52 max|exact|, E_env the largest error among 16 float64 twins; lambda,
have_cur, decisions, the ticket and everything a launch must leave alone bit for bit; the constants of the next linearisation to 1 ulp32;
emitted poses against the float32 twin of the extraction.  Sweep cases: target 1 of the B = 3 launch is the target launched alone, bit for
bit.  Split cases marked so: three launches give the same bits.  Two-role launches: every group equals the group launched alone through
k_solve_joint.  Accepting launches without the pose-consistency term: the stored right-hand side and cost are the export of the same
records.  The refusals return TCSFM_E_ARG with the message of the check meant and leave every output as it was.

MEASURED (MI355X; per group of cases the worst E of the step d and of the trial transforms T in units of their bar 4 E_env + floor, and the
largest E itself; the worst record-sum error in units of its bound, the worst pose error in units of its bound, the worst constant error in
units of its tolerance; TCSFM_TEST_JOINT_SOLVE_EXACT_REPORT=<file> writes the line of every case):
    cases                              n  d of bar        E  T of bar        E    sums   pose  const
    sweep S1                           9         -        -         -        -   0.249      -      -
    sweep S2                           9         -        -         -        -   0.232      -      -
    sweep S3                           9         -        -         -        -   0.243      -      -
    sweep S4                           7         -        -         -        -   0.241      -      -
    split sum S1                      57     0.162  7.9e-16     0.137  7.2e-16   0.178  0.230  0.000
    split sum S2                      57     0.204  1.6e-15     0.203  1.7e-15   0.190  0.278  0.000
    split sum S4                      57     0.238  2.5e-15     0.205  2.5e-15   0.182  0.391  0.000
    solver paths S1                   16     0.131  2.3e-16     0.096  3.0e-16   0.154  0.231  0.000
    solver paths S2                   16     0.214  6.2e-16     0.170  6.5e-16   0.127  0.433  0.000
    solver paths S3                   16     0.281  1.3e-15     0.247  1.3e-15   0.156  0.433  0.000
    solver paths S4                   16     0.186  1.5e-15     0.186  1.5e-15   0.161  0.433  0.000
    normalisers                       10     0.163  5.6e-16     0.119  6.8e-16   0.161  0.250  0.000
    conditioning S1                    6     0.103  3.5e-12     0.101  3.4e-12       -  0.106  0.000
    beyond the judged range S1         1     0.028  1.5e-07     0.028  1.5e-07       -  0.051  0.000
    conditioning S2                    6     0.119  8.1e-12     0.111  8.1e-12       -  0.106  0.000
    beyond the judged range S2         1     0.056  2.1e-07     0.061  2.0e-07       -  0.051  0.000
    conditioning S3                    6     0.170  8.0e-12     0.154  9.2e-12       -  0.106  0.000
    beyond the judged range S3         1     0.057  1.2e-07     0.057  1.2e-07       -  0.051  0.000
    conditioning S4                    6     0.196  1.5e-11     0.180  1.5e-11       -  0.106  0.000
    beyond the judged range S4         1     0.058  3.9e-07     0.058  3.9e-07       -  0.051  0.000
    block structure                    2     0.103  1.8e-16     0.071  2.0e-16   0.101  0.224  0.000
    retraction                         2     0.000  1.8e-24     0.057  1.1e-16       -  0.297  0.000
    pose consistency v2                6     0.093  1.6e-16     0.061  1.8e-16   0.159  0.128  0.000
    pose consistency v4                6     0.156  1.6e-16     0.063  1.8e-16   0.159  0.145  0.000
    coalesced routing                  3     0.230  1.2e-15     0.198  1.2e-15   0.189  0.330  0.000
    two-role launches v1               4     0.094  2.0e-16     0.048  1.9e-16   0.118  0.419  0.000
    two-role launches v2               4     0.094  2.0e-16     0.048  1.9e-16   0.118  0.419  0.000
    two-role launches v3               4     0.177  2.0e-16     0.072  1.9e-16   0.118  0.419  0.000
    two-role launches v4               4     0.177  2.0e-16     0.072  1.9e-16   0.118  0.419  0.000
(342 cases and 21 refusals; the split groups' step figures are the nine cases that take a full step, the rest go through the export.)
The kernel's worst step error is 0.28 of the bar (an LM step at S = 3), in the range of the clean float64 stand-in on the CPU (0.30); no
group comes near the margin, none needs a wider one.  Every record sum is within a quarter of its bound, worst at nblk = 1 where only the
roundings of the assembly remain.  Every constant the kernel wrote is the correctly rounded float32 of the exact value (error 0); in the
ill-conditioned cases whose transform bar exceeds 2^-40 the constants are judged as a function of the transform that was written
(joint_solve_exact_inputs.judge_case says why).  Beyond the judged range (condition 1e13) kernel and twins both keep 6 to 7 digits.
solve_joint_body needed no fix.
"""
import ctypes as C
import os

import numpy as np
import pytest

import joint_solve_exact_inputs as JX
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
    """-> (return code, outputs as JX.new_outputs: filled with the sentinel before the launch, copied back whole)"""
    from tightly_coupled_sfm_amd import _lib
    o = JX.new_outputs(c)
    opts = _lib.default_opts(n_iters=c.n_iters, solver=c.solver, lambda0=c.lam0, lambda_up=c.lam_up, lambda_down=c.lam_down, lambda_min=c.lam_min)
    a = _lib.DebugSolveJointArgs()
    a.variant, a.NS, a.it, a.mode, a.n_alloc, a.pc_np = c.variant, c.NS, c.it, c.mode, c.n_alloc, c.pc_np
    a.c_ncall, a.c_B, a.c_S = c.c_ncall, c.c_B, c.c_S
    for i in range(c.c_ncall):
        a.c_len[i] = c.c_len[i]
        a.c_pose_out[i] = _addr(o["c_pose_out"][i])
    a.w_pc, a.pc_eps = c.w_pc, c.pc_eps
    keep = []
    for g, q, ga in zip(c.groups, o["g"], (a.a, a.b)):
        rec = np.ascontiguousarray(g.rec, np.float32)
        norms = None if g.norms is None else np.ascontiguousarray(g.norms, np.int32)
        keep += [rec, norms]
        ga.B, ga.b_alloc, ga.nblk, ga.nsplit, ga.n0 = g.B, g.b_alloc, g.nblk, g.nsplit, g.n0
        ga.norm_n, ga.norm_B, ga.pc_self0, ga.pc_part0, ga.c_f = (0 if norms is None else norms.shape[0]), g.norm_B, g.pc_self0, g.pc_part0, g.c_f
        ga.records, ga.norms = _addr(rec), _addr(norms)
        for k in ("js", "delta_out", "accept_out", "export_out", "jpart", "jtick"):
            setattr(ga, k, _addr(q[k]))
    a.state, a.pconst, a.pose_lin = _addr(o["state"]), _addr(o["pconst"]), _addr(o["pose_lin"])
    for k in JX.ALL_OUT:
        setattr(a, k, _addr(o[k]))
    rc = e.debug_solve_joint(opts, a)
    del keep
    return rc, o


def _run(e):
    def run(c):
        rc, o = launch(e, c)
        assert rc == 0, (c.name, rc, e.last_error())
        return o
    return run


def _report(line):
    path = os.environ.get("TCSFM_TEST_JOINT_SOLVE_EXACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_struct_layout_is_the_librarys():
    from tightly_coupled_sfm_amd import _lib
    assert _lib.debug_solve_joint_layout() == (C.sizeof(_lib.PairState), C.sizeof(_lib.PairConst), C.sizeof(_lib.JointState)) == \
        (SX.STATE_DT.itemsize, SX.CONST_DT.itemsize, JX.JS_DT.itemsize)


@pytest.mark.parametrize("name", [c.name for c in JX.all_cases()])
def test_one_launch_against_exact_arithmetic(eng, name):
    c = JX.by_name()[name]
    run = _run(eng)
    out = run(c)
    fails, meas = JX.judge_case(c, lambda _c: out)
    if JX.wants_m_export(c):
        fails += JX.check_m_export(c, run, out)
    fails += JX.check_alone(c, run, out)
    if "repeat" in c.claims:
        fails += JX.check_repeat(c, run, out)
    line = JX.report_line(c, meas, len(fails))
    print(line)
    _report(line)
    assert not fails, fails[:6]


@pytest.mark.parametrize("what", [n for n, _, _ in JX.refusal_cases()])
def test_refusals_launch_nothing(eng, what):
    c, words = {n: (c, w) for n, c, w in JX.refusal_cases()}[what]
    rc, o = launch(eng, c)
    assert rc == E_ARG, (what, rc)
    assert eng.last_error().startswith("tcsfm_debug_solve_joint: ") and words in eng.last_error(), eng.last_error()       # (the check meant is the one that fired)
    fresh = JX.new_outputs(c)

    def same(x, y, k):
        if isinstance(y, list):
            for i, (p, q) in enumerate(zip(x, y)):
                same(p, q, f"{k}[{i}]")
        elif isinstance(y, dict):
            for kk in y:
                same(x[kk], y[kk], f"{k}.{kk}")
        elif y is not None:
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)
    same(o, fresh, "out")
    # the handle is still good: the base case of the refusals runs
    assert launch(eng, JX.by_name()["gn it0 S2"])[0] == 0


def test_guard_bands_of_the_entrys_own_allocations(eng):
    """As in test_gpu_solve_exact.py: the entry frees its device arrays before it returns, so it reads their guard bands back itself and
    returns an error when one is hit -- every case above asserts return code 0.  Here: the guards are on, and the entry leaves no
    allocation behind (a split two-role launch with every optional array given)."""
    from tightly_coupled_sfm_amd import _lib
    n0, bad0 = _lib.check_guards()
    assert n0 > 0, "the GPU tests run with TCSFM_DEBUG_GUARDS=1 (tests/conftest.py)"
    assert launch(eng, JX.by_name()["roles v4 S3 split"])[0] == 0
    n1, bad1 = _lib.check_guards()
    assert bad0 == 0 and bad1 == 0 and n0 == n1
