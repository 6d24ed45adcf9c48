"""GPU: ONE linearisation of the dense mode on the reference's loss (tcsfm_linearize_dense_window_sources: scal_out, g_pose, g_rho, g_rho_src),
pixel by pixel and entry by entry against the float64 oracle under the engine's own recorded decisions.  Cases, metric, bound and judge:
tests/dense_linearize_exact_inputs.py (conditions and planted faults: tests/test_dense_linearize_exact_inputs_cpu.py).

Every case runs twice, with the decision trace on and off: scal_out, g_pose, g_rho and g_rho_src must be the same bits, so the traced run
vouches for the production instantiations of k_linearize<FRONT> and k_dense_joint.  The traced run is judged: every measure
E <= 4 E(float32 oracle, same bits) + A, K_f and K_i exact and equal to the population counts of the trace, exact zeros where nothing
contributes, and no hard flip among the decisions (the oracle, replaying, also decides for itself).  g_rho_src comes from launches that are
NOT traced and take their decisions again (k_dref_scatter_src, k_dense_joint<1> on the inverse pairs): it is judged under the same recorded
bits, so a decision they take differently shows as an error of that pixel.
Batch independence.  The loss's normalisers are sums over the CALL (K_f, K_i, and B itself in the depth-consistency, prior and smoothness
weights), so a target's outputs in a B = 2 call are not those of its window called alone.  Exactly comparable are: (1) the same two windows
in the other ORDER -- every normaliser is the same integer, the scatter is integer addition: g_rho, g_rho_src, every g_pose row and every
trace plane of a target must be the same bits in either slot; (2) against the window called alone: the trace planes (decisions see no
normaliser) bit for bit, K_f and K_i as the sum of the windows' own, and -- on the option row without depth consistency, prior and
smoothness, where a_f = 1 / K_f is the forward pairs' only factor, applied in double by k_solve_joint -- the forward pairs' g_pose rows after
rescaling by the exact integer ratio K_f(call) / K_f(alone), to the two roundings of that product.  g_rho carries two normalisers whose
ratio a_i / a_f changes with the call inside one fp32 sum: it has no exact counterpart in the call alone; (1) covers it.
The trace capacity of the export is counted for one linearisation, whatever opts.n_iters says.

MEASURED (MI355X; per group of cases: worst ratio E / E(float32 twin), and the largest E; columns rho | rho_s | xi_fwd | xi_inv | fwd |
inv_photo | inv_dc; TCSFM_TEST_DENSE_LIN_EXACT_REPORT=<file> writes the line of every case, with the 99th percentiles of rho and rho_s):
    cases                                  n  ratio    rho  rho_s xi_fwd xi_inv    fwd inv_ph inv_dc  |  E      rho    rho_s   xi_fwd   xi_inv      fwd  inv_pho   inv_dc  | p99 rho    rho_s
    5x9-B1-S2 no argmin, automask 0        1          1.64   0.11   0.35   0.09   2.50   0.40   0.22  |     3.6e-06  1.0e-05  8.1e-08  1.9e-07  7.7e-08  1.2e-08  1.0e-08  |   3.3e-06  7.5e-06
    9x40-B1-S1 w_smooth 2                  1          0.19   0.12   0.10   0.07   0.44  93.80   0.16  |     2.4e-06  1.9e-05  2.3e-07  2.7e-07  2.0e-08  7.7e-08  2.8e-08  |   1.0e-06  1.0e-05
    16x48-B2-S2 default                    1          0.41   0.21   0.08   0.04   0.34   0.02   1.74  |     3.0e-05  5.2e-05  2.3e-07  3.0e-07  5.4e-08  6.4e-09  6.5e-08  |   1.5e-05  1.7e-05
    12x36-B1-S3 no argmin                  1          0.21   0.12   0.04   0.04   0.06   0.17   0.08  |     1.4e-05  2.6e-05  1.1e-07  2.9e-07  4.9e-09  4.7e-08  1.3e-08  |   5.3e-06  1.1e-05
    20x36-B2-S4 default                    1          0.94   0.08   0.06   0.05   0.15   0.72   0.27  |     2.6e-05  4.1e-05  2.9e-07  5.0e-07  2.8e-08  5.5e-08  2.8e-08  |   1.6e-05  9.7e-06
    17x33-B2-S2 default                    1          0.28   0.38   0.10   0.15   0.10   0.05  25.00  |     1.9e-05  4.8e-05  3.0e-07  3.9e-07  2.3e-08  1.4e-08  4.8e-08  |   1.3e-05  7.0e-06
    37x53-B2-S2 default                    1          0.31   0.62   0.10   0.04   0.04   0.08   0.20  |     3.2e-05  5.8e-05  6.3e-07  2.6e-07  4.9e-08  5.5e-08  4.0e-08  |   1.7e-05  1.4e-05
    208x640-B1-S2 default                  1          0.15   0.05   0.03   0.04   0.02   0.03   0.06  |     1.0e-03  6.7e-03  9.6e-07  1.3e-06  1.3e-07  3.2e-07  1.6e-08  |   1.6e-05  9.8e-06
    17x33-B2-S2 option rows, w_dc 0        4          2.46   1.14   0.16   0.39  64.71   0.13   0.00  |     1.3e-04  7.1e-05  3.2e-07  3.7e-07  3.6e-07  3.3e-08  0.0e+00  |   5.6e-05  5.5e-06
    17x33-B2-S2 option rows, w_dc 0.15     4          0.26   0.40   0.44   0.15   6.28   0.34  25.00  |     1.3e-05  4.8e-05  3.1e-07  4.0e-07  1.5e-07  5.9e-08  4.8e-08  |   2.2e-06  8.1e-06
    17x33-B2-S2 option rows, w_dc 2        3          0.20   0.36   0.17   0.08   1.64   0.17  25.00  |     1.4e-05  4.8e-05  3.6e-07  3.3e-07  5.4e-08  5.9e-08  4.8e-08  |   1.7e-06  1.0e-05
    37x53-B2-S2 option rows, w_dc 0        4          1.20   0.40   0.13   0.05   1.39   0.08   0.00  |     1.5e-04  8.1e-05  6.8e-07  2.7e-07  2.4e-07  5.5e-08  0.0e+00  |   6.9e-05  6.4e-06
    37x53-B2-S2 option rows, w_dc 0.15     4          1.13   0.50   0.13   0.07   9.27   0.08   0.20  |     3.1e-05  8.8e-05  7.1e-07  2.9e-07  1.6e-07  5.5e-08  4.0e-08  |   4.8e-06  2.8e-05
    37x53-B2-S2 option rows, w_dc 2        3          0.23   0.40   0.20   0.07   0.93   0.08   0.20  |     7.1e-06  9.2e-05  2.5e-07  9.1e-07  1.2e-07  5.5e-08  4.0e-08  |   3.2e-06  4.8e-05
    37x53-B1-S2 out of bounds              1          1.34   0.13   0.19   0.91   0.34   0.01   0.85  |     1.6e-04  5.9e-05  2.2e-07  1.9e-06  2.3e-08  3.8e-09  3.7e-08  |   2.7e-05  4.8e-06
    37x53-B1-S2 scatter fallback           1          1.56   0.06   0.64   0.75   0.17   0.55   0.48  |     4.2e-04  6.8e-05  2.9e-06  3.6e-06  1.1e-07  5.9e-08  2.2e-08  |   1.0e-04  2.1e-05
Ratios above 1 mean the kernels' fp32 accumulation shows.  The largest for a pixel map is 2.46 (17x33, argmin 0, w_dc 0: E_rho 1.3e-4 against
the twin's 5.3e-5), under the margin of 4.  The three scalars reach ratios of 6 .. 94 only where the float32 twin happens to be nearly exact:
their E (at most 3.6e-7 for fwd, 7.7e-8 for inv_photo, 4.8e-8 for inv_dc) is below the accumulation allowance alone (fwd: 15 x 2^-24 =
8.9e-7, the inverse sums: 13 x 2^-24 = 7.7e-7).  The large E_rho / E_rho_s of 208x640 (1.0e-3, 6.7e-3) are single pixels on which the float32
twin is off by seven and twenty times as much (ratio 0.15, 0.05); the 99th percentiles are 1.6e-5 and 9.8e-6.
FOUND by the zero rule, and fixed in joint_kernel.h (s_store): on pixels that carry no contribution at all in float64 -- won by a source
other than source 0 where source 0 samples the zero padding, so that its weight map, which multiplies every selected pixel, is exactly 0 --
the engine left 1e-12 .. 8e-12 in g_rho: cd * rcp(cd) may be 1 - 2^-24, the weight 6e-8 instead of 0.  Four option rows (w_dc 0, prior 0, no
smoothness: nothing else reaches those pixels) failed on 7 .. 59 such pixels before the fix.
"""
import numpy as np
import pytest
import torch

import dense_linearize_exact_inputs as DX
import parity_util as PU

pytestmark = pytest.mark.gpu


def _eng(c):
    from tightly_coupled_sfm_amd.engine import Engine
    return Engine(c.H, c.W, 2 * c.S * c.B)


@pytest.mark.parametrize("cid", DX.IDS)
def test_linearisation_pixel_by_pixel(cid):
    c = DX.BY_ID[cid]
    e = _eng(c)
    eng, bits = DX.traced_and_production(e, c)
    e.close()
    fails, summ = DX.judge_case(c, eng, bits, cid)
    print(cid, " ".join(f"{k}: x{summ[k][0]:.2f} E={summ[k][1]:.2e}" for k in DX.MEASURES))
    PU.check_flips_every_linearisation(DX.oracle("f64"), 1, 2 * c.S * c.B * c.H * c.W, cid)      # no hard flip; near-ties within the allowance
    assert not fails, (cid, fails)


SWAP = [DX.case(17, 33, 2, 2), [c for c in DX.OPTION_CASES if (c.H, c.W) == (37, 53) and c.w_smooth > 0 and c.w_dc > 0 and c.prior > 0][0], DX.case(20, 36, 2, 4)]


@pytest.mark.parametrize("c", SWAP, ids=[DX.case_id(c) for c in SWAP])
def test_target_is_the_same_bits_in_either_slot_of_the_call(c):
    e = _eng(c)
    a, bits_a = DX.run_engine(e, c, True)
    b, bits_b = DX.run_engine(e, c, True, order=(1, 0))
    e.close()
    S, B = c.S, c.B
    assert a["K_f"] == b["K_f"] and a["K_i"] == b["K_i"]
    assert np.array_equal(a["g_rho"][::-1], b["g_rho"]) and np.array_equal(a["g_rho_src"][:, ::-1], b["g_rho_src"])
    assert np.array_equal(a["g_pose"].reshape(2, S, B, 6)[:, :, ::-1], b["g_pose"].reshape(2, S, B, 6))
    assert np.array_equal(bits_a.reshape(2, S, B, c.H, c.W)[:, :, ::-1], bits_b.reshape(2, S, B, c.H, c.W))
    assert not np.array_equal(a["g_rho"][0], a["g_rho"][1])


ALONE = [[c for c in DX.OPTION_CASES if (c.H, c.W) == hw and c.w_dc == 0 and c.prior == 0 and c.w_smooth == 0 and c.w_pc == 0 and c.argmin == 1
          and c.w_ssim > 0][0] for hw in DX.OPTION_SHAPES]


@pytest.mark.parametrize("c", ALONE, ids=[DX.case_id(c) for c in ALONE])
def test_target_of_a_batch_against_its_window_called_alone(c):
    e = _eng(c)
    many, bits = DX.run_engine(e, c, True)
    S, B = c.S, c.B
    Kf = Ki = 0
    for t in range(B):
        one, bits1 = DX.run_engine(e, c, True, sub=t)
        assert np.array_equal(bits.reshape(2, S, B, c.H, c.W)[:, :, t], bits1.reshape(2, S, c.H, c.W)), t
        Kf += one["K_f"]; Ki += one["K_i"]
        gm, g1 = many["g_pose"].reshape(2, S, B, 6)[0, :, t] * many["K_f"], one["g_pose"].reshape(2, S, 6)[0] * one["K_f"]
        assert np.allclose(gm, g1, rtol=1e-14, atol=0), (t, np.abs(gm / g1 - 1).max())
        assert many["K_f"] != one["K_f"]
    e.close()
    assert (many["K_f"], many["K_i"]) == (Kf, Ki)


def test_trace_capacity_is_counted_for_one_linearisation():
    c = DX.case(37, 53, 2, 2)
    e, d = _eng(c), DX.inputs(c)
    N = 2 * c.S * c.B
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    args = (t(d["tgt"]), t(d["srcs"]), t(d["depth_t"][:, None]), t(d["depth_s"][:, :, None]), t(d["K"]), t(d["pose"]))
    o = DX.engine_opts(c)
    o.n_iters = 4
    for sources in (False, True):
        e.trace_begin(1, N)
        e.linearize_dense_window(*args, o, argmin=True, sources=sources)          # fits: one linearisation of 2 S B pairs
        bits, _ = e.trace_end()
        assert all((bits[0, m] & 1).sum() > 0 for m in range(N))
        e.trace_begin(1, N - 1)
        with pytest.raises(RuntimeError, match="bits buffer too small"):
            e.linearize_dense_window(*args, o, argmin=True, sources=sources)
        e.trace_end()
    e.close()
