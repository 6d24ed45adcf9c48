"""The float64 oracle's restatement of the reference's loss at S = 4 (the five-frame window t-2 .. t+2): value and gradients of
orc_linearize_dense_ref against reference autograd (golden `winloss4src24x40`, tests/golden/make_golden_four_sources.py) to 1e-10 --
the yardstick the GPU tests of the four-source dense mode (test_gpu_four_sources.py) measure the engine with."""
import numpy as np
import pytest

from conftest import load_golden
from oracle.oracle import default_opts


def _maxabs(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


@pytest.fixture(scope="module")
def g4():
    g = load_golden("winloss4src24x40")
    assert g["sources"].shape[:2] == (4, 2) and g["first"].shape == (16, 6)
    return g


@pytest.mark.parametrize("tag,argmin,w_init", [("full", True, 0.0), ("noargmin_full", False, 0.0), ("fullinit", True, 0.1),
                                               ("fullinit_smooth", True, 0.1), ("full_pc", True, 0.0)])
def test_oracle_loss_and_gradients_at_four_sources(tag, argmin, w_init, g4, oracle64):
    g = g4
    S, B = g["sources"].shape[:2]
    a = (g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"], g["first"])
    mind, maxd = (float(x) for x in g["min_max_depth"])
    rd = 1.0 / mind - 1.0 / maxd
    op = default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15)
    op.w_smooth = 2.0 if tag == "fullinit_smooth" else 0.0
    op.w_pose_consist = 0.1 if tag == "full_pc" else 0.0
    depth0 = None if w_init == 0 else 1.0 / (1.0 / maxd + rd * g["sig_t0"])
    L = oracle64.linearize_dense_ref(*a, op, argmin=argmin, w_init=w_init, depth0=depth0, min_depth=mind, max_depth=maxd)
    ref_loss = float(g[f"{tag}_loss"])
    assert abs(L["loss"] - ref_loss) < 1e-12 * ref_loss, (L["loss"], ref_loss)
    gp = np.stack([oracle64.euler_left_jacobian(g["first"][m]).T @ L["g_xi"][m] for m in range(2 * S * B)])
    ref_gp = g[f"{tag}_grad_pose"]
    assert _maxabs(gp, ref_gp) < 1e-10 * np.abs(ref_gp).max(), (_maxabs(gp, ref_gp), np.abs(ref_gp).max())
    # every one of the 16 directed poses carries a gradient (no source is silently dropped)
    assert np.all(np.abs(ref_gp).max(axis=1) > 1e-4 * np.abs(ref_gp).max())
    if tag == "full":
        gd, ref = -L["g_rho"] / g["depth_t"][:, 0] ** 2, g["full_grad_depth_t"]
        assert _maxabs(gd, ref) < 1e-10 * np.abs(ref).max(), (_maxabs(gd, ref), np.abs(ref).max())
        gds, refs = -L["g_rho_s"] / g["depth_s"][:, :, 0] ** 2, g["full_grad_depth_s"]
        assert _maxabs(gds, refs) < 1e-10 * np.abs(refs).max(), (_maxabs(gds, refs), np.abs(refs).max())
        assert all(np.abs(refs[s]).max() > 0.05 * np.abs(refs).max() for s in range(S))       # all four source maps see the loss
        # w_dc couples the four poses of a target: the reduced system's off-diagonal blocks are not zero for any pair of sources
        Hj = L["H_joint"]
        for s in range(S):
            for t in range(s):
                assert np.abs(Hj[:, 6 * s:6 * s + 6, 6 * t:6 * t + 6]).max() > 0.0, (s, t)
    if tag in ("fullinit", "fullinit_smooth"):
        gs, ref = L["g_rho"] * rd, g[f"{tag}_grad_sig_t"]
        assert _maxabs(gs, ref) < 1e-10 * np.abs(ref).max(), (_maxabs(gs, ref), np.abs(ref).max())


def test_oracle_quarter_resolution_gradient_at_four_sources(g4, oracle64):
    """the reference's parametrisation (`qinit`): at the x4-upsampled quarter-resolution maps of target and sources, the loss, the pose
    gradients and the target map's gradient carried through the transposed upsampling equal reference autograd"""
    g = g4
    S, B = g["sources"].shape[:2]
    mind, maxd = (float(x) for x in g["min_max_depth"])
    rd = 1.0 / mind - 1.0 / maxd
    depth_of = lambda sig: 1.0 / (1.0 / maxd + rd * sig)
    depth_s = np.stack([depth_of(g["q_up"][:, 1 + s]) for s in range(S)])
    L = oracle64.linearize_dense_ref(g["target"], g["sources"], depth_of(g["q_up"][:, 0]), depth_s, g["K"], g["first"],
                                     default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15), argmin=True, w_init=0.1, depth0=depth_of(g["sig_t0"]),
                                     min_depth=mind, max_depth=maxd)
    assert abs(L["loss"] - float(g["qinit_loss"])) < 1e-12 * float(g["qinit_loss"])
    gp = np.stack([oracle64.euler_left_jacobian(g["first"][m]).T @ L["g_xi"][m] for m in range(2 * S * B)])
    assert _maxabs(gp, g["qinit_grad_pose"]) < 1e-10 * np.abs(g["qinit_grad_pose"]).max()
    gq = np.stack([oracle64.up4_adjoint(L["g_rho"][b] * rd) for b in range(B)])
    ref = g["qinit_grad_q"][:, 0]
    assert _maxabs(gq, ref) < 1e-10 * np.abs(ref).max(), (_maxabs(gq, ref), np.abs(ref).max())
