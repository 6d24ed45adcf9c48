"""GPU: the normal equations of ONE pose linearisation (k_linearize -> k_solve's record: H, g, cost_photo, cost_dc, mask count), entry by entry
against the float64 oracle under the engine's own recorded decisions.  Cases, metric, bound and judge: tests/linearize_exact_inputs.py
(conditions and planted faults: tests/test_linearize_exact_inputs_cpu.py).

Every case runs twice, with the decision trace on and off: H, g and the four statistics must be the same bits, so the traced run vouches
for the production instantiation of the kernel.  The traced run is judged: every measure E <= 4 E(float32 oracle, same bits) + D 2^-24,
the mask count equal to the population count of the trace's bit 0, and no hard flip among the decisions (the oracle, replaying, also
decides for itself).  Batch independence: item 1 of an N = 3 call is the same pair called alone, bit for bit.  The adjoint form of the SSIM
gradient (TCSFM_ADJOINT=1, read once per process) is judged the same way in a fresh child process.

MEASURED (MI355X; per group of cases: worst ratio E / E(float32 twin), and the largest E, columns H | g | cost_photo | cost_dc;
TCSFM_TEST_LIN_EXACT_REPORT=<file> writes the line of every case):
    cases                                                       n   ratio  H     g     photo dc     |  E  H        g        photo    dc
    pair 8x16 N=3 default                                       1          1.70  0.16  2.99  0.00  |      1.8e-05  4.6e-07  7.8e-08  0.0e+00
    pair 16x32 N=3 default                                      1          0.13  0.12  0.16  0.00  |      8.6e-07  2.5e-07  1.0e-07  0.0e+00
    pair 17x33 N=3 default                                      1          0.14  0.10  0.09  0.00  |      7.2e-07  2.3e-07  5.6e-08  0.0e+00
    pair 37x53 N=3 default                                      1          0.06  0.03  0.14  0.00  |      4.4e-07  2.0e-07  1.7e-07  0.0e+00
    pair 48x160 N=3 default                                     1          0.16  0.13  0.13  0.00  |      9.8e-07  2.3e-06  2.5e-07  0.0e+00
    pair 256x512 N=3 default                                    1          0.07  0.07  0.09  0.00  |      4.6e-06  1.1e-06  5.5e-07  0.0e+00
    pair 208x640 N=3 default                                    1          0.32  0.05  0.02  0.00  |      2.5e-06  2.3e-06  2.3e-07  0.0e+00
    pair 256x512 N=1 default                                    1          0.07  0.07  0.00  0.00  |      7.0e-07  1.1e-06  1.7e-08  0.0e+00
    pair 208x640 N=1 default                                    1          0.32  0.04  0.02  0.00  |      1.4e-06  1.0e-06  2.3e-07  0.0e+00
    pair 17x33 refine 0 w_dc 0, weights x automask              5          0.25  0.17  0.62  0.00  |      3.2e-06  2.4e-07  1.1e-07  0.0e+00
    pair 17x33 refine 0 w_dc 0.15, weights x automask           6          0.25  0.17  0.62  0.08  |      3.2e-06  2.4e-07  1.1e-07  9.9e-09
    pair 17x33 refine 0 w_dc 128, weights x automask            6          0.23  0.03  0.62  0.08  |      4.8e-07  1.3e-07  1.1e-07  9.9e-09
    pair 17x33 refine 1 w_dc 0, weights x automask              6          1.32  0.67  0.26  0.00  |      7.1e-06  4.7e-07  8.1e-08  0.0e+00
    pair 17x33 refine 1 w_dc 0.15, weights x automask           6          1.58  0.52  0.26  0.61  |      7.0e-06  4.7e-07  8.1e-08  4.7e-08
    pair 17x33 refine 1 w_dc 128, weights x automask            6          0.28  0.05  0.26  0.61  |      3.9e-06  4.6e-07  8.1e-08  4.7e-08
    pair 37x53 refine 0 w_dc 0, weights x automask              5          0.36  0.08  0.33  0.00  |      1.7e-05  1.8e-07  1.0e-07  0.0e+00
    pair 37x53 refine 0 w_dc 0.15, weights x automask           6          0.36  0.08  0.33  1.05  |      1.7e-05  2.0e-07  1.7e-07  5.1e-08
    pair 37x53 refine 0 w_dc 128, weights x automask            6          0.36  0.09  0.33  1.05  |      8.9e-06  1.5e-07  1.7e-07  5.1e-08
    pair 37x53 refine 1 w_dc 0, weights x automask              6          0.45  0.49  0.94  0.00  |      5.3e-06  5.5e-07  1.6e-07  0.0e+00
    pair 37x53 refine 1 w_dc 0.15, weights x automask           6          0.45  0.63  0.94  0.54  |      5.3e-06  5.7e-07  1.6e-07  5.9e-08
    pair 37x53 refine 1 w_dc 128, weights x automask            6          0.70  0.44  0.94  0.54  |      3.1e-06  1.0e-06  1.6e-07  5.9e-08
    pair 17x33 out of bounds                                    1          1.03  0.51  0.42 14.85  |      3.3e-06  7.5e-07  1.1e-07  3.8e-08
    pair 37x53 out of bounds                                    1          1.09  0.69  0.77 57.18  |      6.2e-06  1.4e-06  1.1e-07  7.8e-08
    window 17x33 refine 0, argmin x rule                        4          0.18  0.17  0.84  0.00  |      1.7e-06  2.3e-07  1.4e-07  0.0e+00
    window 17x33 refine 1, argmin x rule                        4          0.45  0.35  0.99  0.00  |      3.2e-06  9.2e-07  1.2e-07  0.0e+00
    window 37x53 refine 0, argmin x rule                        4          0.08  0.20  0.21  0.00  |      4.2e-06  8.0e-07  1.8e-07  0.0e+00
    window 37x53 refine 1, argmin x rule                        4          0.54  0.23  2.60  0.00  |      2.4e-06  1.2e-06  3.5e-07  0.0e+00
    pair 17x33 N=3 default ADJOINT                              1          0.14  0.09  0.09  0.00  |      7.2e-07  2.1e-07  5.6e-08  0.0e+00
    pair 37x53 N=3 default ADJOINT                              1          0.06  0.04  0.14  0.00  |      4.4e-07  1.8e-07  1.7e-07  0.0e+00
    window 17x33 refine 0, argmin x rule ADJOINT                4          0.18  0.14  0.84  0.00  |      1.7e-06  3.0e-07  1.4e-07  0.0e+00
    window 17x33 refine 1, argmin x rule ADJOINT                4          0.45  0.38  0.99  0.00  |      3.2e-06  8.4e-07  1.2e-07  0.0e+00
    window 37x53 refine 0, argmin x rule ADJOINT                4          0.08  0.24  0.21  0.00  |      4.2e-06  8.7e-07  1.8e-07  0.0e+00
    window 37x53 refine 1, argmin x rule ADJOINT                4          0.54  0.24  2.60  0.00  |      2.4e-06  1.2e-06  3.5e-07  0.0e+00
Ratios above 1 mean the kernel's fp32 accumulation shows; none reaches the margin of 4 except cost_dc of the out-of-bounds cases, where
the float32 twin happens to be within 1.4e-9 of float64 and the kernel's 7.8e-8 is a tenth of the accumulation allowance A = 7.7e-7.
The adjoint form changes g only (H is not touched by it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import linearize_exact_inputs as LX
import parity_util as PU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("H", "g", "cost", "cost_photo", "cost_dc", "n_mask")


def _eng(c):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(c.H, c.W, c.max_pairs)


def _judge(c, items, bits, tag):
    fails, summ = LX.judge_case(c, items, bits, tag)
    print(tag, " ".join(f"{k}: x{summ[k][0]:.2f} E={summ[k][1]:.2e}" for k in LX.MEASURES))
    PU.check_flips_every_linearisation(LX.oracle("f64"), 1, c.N * c.H * c.W, tag)          # no hard flip; near-ties within the allowance
    assert not fails, (tag, fails)


@pytest.mark.parametrize("cid", LX.IDS)
def test_linearisation_entry_by_entry(cid):
    c = LX.BY_ID[cid]
    items, bits = LX.traced_and_production(_eng(c), c)
    _judge(c, items, bits, cid)


BATCH = [LX.pair_case(17, 33), LX.pair_case(37, 53, refine=1, w_dc=0.15), LX.pair_case(48, 160), LX.pair_case(208, 640)]


@pytest.mark.parametrize("c", BATCH, ids=[LX.case_id(c) for c in BATCH])
def test_item_of_a_batch_is_the_pair_called_alone(c):
    e = _eng(c)
    one = c._replace(N=1)
    assert np.array_equal(LX.inputs(one)["tgt"][0], LX.inputs(c)["tgt"][1]) and np.array_equal(LX.inputs(one)["ls"][0], LX.inputs(c)["ls"][1])
    many, bits_many = LX.run_engine(e, c, True)
    alone, bits_alone = LX.run_engine(e, one, True)
    assert np.array_equal(bits_many[1], bits_alone[0])
    for k in KEYS:
        assert np.array_equal(many[1][k], alone[0][k]), k


def test_trace_of_a_linearisation_call():
    """capacity is counted for ONE linearisation (not opts.n_iters), `decide` is left untouched, tcsfm_loss_surface records nothing"""
    c = LX.pair_case(37, 53)
    e, d = _eng(c), LX.inputs(c)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    args = (t(d["tgt"]), t(d["src"]), t(d["depth_t"]), t(d["depth_s"]), t(d["K"]), t(d["pose"]))
    o = LX.engine_opts(c)
    assert o.n_iters == 4
    e.trace_begin(1, c.N)
    e.linearize(*args, o)                                   # fits: one linearisation of N pairs
    bits, dec = e.trace_end()
    assert (bits[0] & 1).sum() > 0 and np.all(dec == 1)     # (trace_begin fills `decide` with ones)
    e.trace_begin(1, c.N - 1)
    with pytest.raises(RuntimeError, match="bits buffer too small"):
        e.linearize(*args, o)
    e.trace_end()
    e.trace_begin(1, c.N)
    e.loss_surface(*(a[:1] for a in args[:5]), args[5], o)
    bits, _ = e.trace_end()
    assert not bits.any()


def test_adjoint_form_entry_by_entry(tmp_path):
    ids = [LX.case_id(c) for c in LX.ADJOINT_CASES]
    f = str(tmp_path / "adjoint.npz")
    code = "import sys; sys.path.insert(0, 'tests'); import linearize_exact_inputs as LX; LX.child_main(sys.argv[1], sys.argv[2:])"
    r = subprocess.run([sys.executable, "-c", code, f] + ids, env=dict(os.environ, TCSFM_ADJOINT="1"), capture_output=True, text=True,
                       timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    res = np.load(f)
    for cid in ids:
        c = LX.BY_ID[cid]
        items = [{k: res[f"{cid}/{k}"][n] for k in KEYS} for n in range(c.N)]
        _judge(c, items, res[cid + "/bits"], cid + "-adjoint")
    if os.environ.get("TCSFM_ADJOINT", "0") == "0":          # it really is another code path: this process runs the default form
        c = LX.pair_case(37, 53)
        here, _ = LX.run_engine(_eng(c), c, False)
        assert not np.array_equal(np.stack([it["g"] for it in here]), res[LX.case_id(c) + "/g"])
