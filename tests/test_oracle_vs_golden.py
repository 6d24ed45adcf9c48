"""CPU oracle (oracle/tcsfm_oracle.c) pinned against outputs of the reference itself
(tests/golden/*.npz, produced by tests/golden/make_golden.py which imports /root/reference).

Tolerances: float64 oracle vs float64 reference 1e-10 (pure rounding-order differences);
float32 twin vs float32 reference 1e-4 absolute on [0,1] maps, masks may flip on <=0.2% of
pixels (near-ties decided differently in fp32)."""
import os
import numpy as np
import pytest

from conftest import load_golden
from oracle.oracle import default_opts

SIZES = ["s8x16", "s24x40", "s48x160"]


def _border_only(bad):
    """at the exact identity pose border pixels project to x_n = +-1 +- 1 ulp: the OOB test
    (stn.py:223-227) is then decided by rounding order, the only place a float64 flip is tolerated."""
    inner = bad[1:-1, 1:-1]
    return not inner.any()


IDENTITY = 5  # index of the all-zero pose in the small fixtures


def _maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.mark.parametrize("name", SIZES)
def test_warp_G1(name, oracle64, oracle32):
    g = load_golden(name)
    for O, p, tol, flips in ((oracle64, "f64", 1e-10, 0), (oracle32, "f32", 1e-4, 0.002)):
        for k, pose in enumerate(g["poses"]):
            rec, valid, pd, cd = O.warp(g["src"], g["depth_t"], g["depth_s"], pose, g["K"])
            bad = valid != g[f"{p}_valid"][k]
            if len(g["poses"]) > IDENTITY and k == IDENTITY:
                assert _border_only(bad)
            else:
                assert bad.mean() <= flips, (name, p, k, bad.sum())
            ok = ~bad
            assert _maxabs(rec[:, ok], g[f"{p}_rec"][k][:, ok]) < tol
            assert _maxabs(pd[ok], g[f"{p}_proj_depth"][k][ok]) < tol * 10
            assert _maxabs(cd, g[f"{p}_comp_depth"][k]) < tol * 10 * max(1.0, float(np.abs(cd).max()))
    # the stress poses really exercise OOB and the Z clamp
    if name != "s48x160":
        assert g["f64_valid"][3].mean() < 0.9 and (g["f64_comp_depth"][4] == 1e-3).any()


@pytest.mark.parametrize("name", SIZES)
def test_ssim_G2(name, oracle64, oracle32):
    g = load_golden(name)
    assert _maxabs(oracle64.ssim(g["tgt"], g["src"]), g["f64_ssim_ts"]) < 1e-12
    # fp32 SSIM is cancellation-limited (E[x^2]-mu^2): ~1e-4 absolute noise in the reference's own fp32 run
    assert _maxabs(oracle32.ssim(g["tgt"], g["src"]), g["f32_ssim_ts"]) < 3e-4


@pytest.mark.parametrize("name", SIZES)
def test_photometric_G3(name, oracle64, oracle32):
    g = load_golden(name)
    for O, p, tol, flips in ((oracle64, "f64", 1e-10, 0), (oracle32, "f32", 3e-4, 0.003)):
        for k, pose in enumerate(g["poses"]):
            o = O.photometric(g["tgt"], g["src"], g["depth_t"], g["depth_s"], pose, g["K"])
            mask = o["valid"] * o["auto_mask"]                      # helpers.py:19
            bad = mask != g[f"{p}_mask"][k]
            vbad = o["valid"] != g[f"{p}_valid"][k]
            if len(g["poses"]) > IDENTITY and k == IDENTITY:
                assert _border_only(vbad)
            else:
                assert bad.mean() <= flips, (name, p, k, int(bad.sum()))
            ok = ~vbad
            assert _maxabs(o["weight"][ok], g[f"{p}_weight"][k][ok]) < tol * 10
            # diff at a pixel depends on its 3x3 neighbourhood of rec -> only compare where no valid flip nearby
            if vbad.sum() == 0:
                assert _maxabs(o["diff"], g[f"{p}_diff"][k]) < tol


@pytest.mark.parametrize("name", SIZES)
def test_cost_and_gradient_G6(name, oracle64):
    """scalar cost and d(cost)/d(pose) equal the reference's autograd result.  The oracle
    differentiates w.r.t. a left SE(3) perturbation; A = d(xi)/d(pose) maps it to the
    reference's additive [t, euler] parameterisation."""
    g = load_golden(name)
    for k, pose in enumerate(g["poses"]):
        if g["f64_mask"][k].sum() == 0 or (len(g["poses"]) > IDENTITY and k == IDENTITY):
            continue
        lin = oracle64.linearize(g["tgt"], g["src"], g["depth_t"], g["depth_s"], pose, g["K"])
        assert abs(lin["cost"] - g["f64_cost"][k]) < 1e-12
        assert lin["n_mask"] == g["f64_mask"][k].sum()
        gp = oracle64.euler_left_jacobian(pose).T @ lin["g"]
        ref = g["f64_grad_pose"][k]
        assert _maxabs(gp, ref) < 1e-9 * max(1.0, np.abs(ref).max()), (name, k, gp, ref)
        assert abs(oracle64.cost(g["tgt"], g["src"], g["depth_t"], g["depth_s"], pose, g["K"]) - g["f64_cost"][k]) < 1e-12


def test_jacobian_rows_G6(oracle64):
    """per-pixel Jacobian rows of E1 = W e_l1, E2 = W e_ssim, E3 = 1-W (pose and log-scale columns)
    against torch.autograd.functional.jacobian through the reference code."""
    g = load_golden("jac24x40")
    lin = oracle64.linearize(g["tgt"], g["src"], g["depth_t"], g["depth_s"], g["pose"], g["K"],
                             default_opts(nparam=7), rows=True)
    A = oracle64.euler_left_jacobian(g["pose"])
    for r, key in enumerate(("J1", "J2", "J3")):
        assert _maxabs(lin["E"][..., r], g["E"][r]) < 1e-12
        Jpose = lin[key][..., :6] @ A
        assert _maxabs(Jpose, g["J_pose"][r]) < 1e-9 * max(1.0, np.abs(g["J_pose"][r]).max()), key
        assert _maxabs(lin[key][..., 6], g["J_logscale"][r]) < 1e-9 * max(1.0, np.abs(g["J_logscale"][r]).max()), key
    assert np.array_equal(lin["M"], g["mask"])
    assert abs(lin["cost"] - g["cost"]) < 1e-12
    # d cost / d log-scale = sum dC/dD_t D_t + dC/dD_s D_s
    gs = (g["grad_depth_t"] * g["depth_t"]).sum() + (g["grad_depth_s"] * g["depth_s"]).sum()
    assert abs(lin["g"][6] - gs) < 1e-10
    assert _maxabs(A.T @ lin["g"][:6], g["grad_pose"]) < 1e-9
    # The GN matrix itself is a design choice the reference does not pin (it has no second-order
    # solver): check the structural properties the solver relies on.
    Hm = lin["H"]
    assert _maxabs(Hm, Hm.T) == 0.0
    assert np.linalg.eigvalsh(Hm).min() > -1e-9 * np.abs(Hm).max()
    lin6 = oracle64.linearize(g["tgt"], g["src"], g["depth_t"], g["depth_s"], g["pose"], g["K"], default_opts(nparam=6))
    assert _maxabs(lin6["H"], Hm[:6, :6]) < 1e-12 * np.abs(Hm).max() and _maxabs(lin6["g"], lin["g"][:6]) < 1e-12


def test_full_size_summary(oracle64, oracle32):
    """192x640 (BASELINE size): inputs regenerate bit-identically from the seed, cost / gradient /
    mask count / strided samples match the reference run."""
    from tightly_coupled_sfm_amd import synth
    g = load_golden("full192x640")
    p = synth.make_pair(192, 640, seed=0)
    chk = np.array([p[k].astype(np.float64).sum() for k in ("tgt", "src", "depth_t", "depth_s")])
    assert np.allclose(chk, g["in_checksum"], rtol=0, atol=1e-6), "synthetic generator drifted from the fixture"
    pose = g["pose"]
    lin = oracle64.linearize(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"])
    assert abs(lin["cost"] - float(g["f64_cost"])) < 1e-11
    assert lin["n_mask"] == float(g["f64_n_mask"])
    gp = oracle64.euler_left_jacobian(pose).T @ lin["g"]
    assert _maxabs(gp, g["f64_grad_pose"]) < 1e-8 * np.abs(g["f64_grad_pose"]).max()
    o = oracle64.photometric(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"])
    assert _maxabs(o["diff"][::7, ::7], g["f64_diff_sub"]) < 1e-10
    assert _maxabs(o["weight"][::7, ::7], g["f64_weight_sub"]) < 1e-10
    assert _maxabs(o["rec"][:, ::7, ::7], g["f64_rec_sub"]) < 1e-10
    assert np.array_equal((o["valid"] * o["auto_mask"])[::7, ::7], g["f64_mask_sub"])
    # fp32 twin vs the reference's own fp32 run (fp32 SSIM is cancellation-limited): cost within 2e-4 relative
    lin32 = oracle32.linearize(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"])
    assert abs(lin32["cost"] - float(g["f32_cost"])) < 2e-4 * float(g["f32_cost"])
    assert abs(lin32["n_mask"] - float(g["f32_n_mask"])) <= 0.001 * float(g["f32_n_mask"])


def test_loss_surface_G7(oracle32, oracle64):
    """generate_loss_surface tz / yaw sweeps (plot_loss_surface.py:11-87), run by the reference in fp32."""
    g = load_golden("sweep48x160")
    args = (g["tgt"], g["src"], g["depth_t"], g["depth_s"])
    c0 = oracle64.cost(*args, g["pose"], g["K"])
    assert abs(c0 - float(g["original_error"])) < 2e-5 * c0
    for deltas, errs, idx in ((g["delta_list"], g["errors"], 2), (g["delta_list_yaw"], g["errors_yaw"], 4)):
        mine = []
        for d in deltas:
            q = g["pose"].astype(np.float64).copy(); q[idx] += d
            mine.append(oracle64.cost(*args, q, g["K"]))
        mine = np.array(mine)
        rel = np.abs(mine - errs) / errs
        # fp32 reference vs f64 oracle: typical agreement 1e-6; a sample where a few of the 7680 mask
        # decisions flip in fp32 moves by up to ~1e-3
        assert np.median(rel) < 2e-5 and np.max(rel) < 2e-3
        assert abs(int(np.argmin(mine)) - int(np.argmin(errs))) <= 1


def test_helpers_G8(oracle64):
    g = load_golden("helpers")
    s, d = oracle64.disp_to_depth(g["disp"], 0.06, 2.67)
    assert _maxabs(s, g["scaled_disp"]) < 1e-13 and _maxabs(d, g["depth"]) < 1e-13


def test_scale_recovery_G10(oracle64, oracle32):
    """DNet ScaleRecovery (dnet_layers.py:249-327) against the reference run on CPU"""
    g = load_golden("scale48x160")
    for O, p, tol in ((oracle64, "f64", 1e-12), (oracle32, "f32", 1e-6)):
        for b in range(2):
            h, m = O.ground_height(g["depth"][b], g["K"][b])
            assert np.array_equal(m, g[f"{p}_mask"][b]) and _maxabs(h, g[f"{p}_height"][b]) < tol
        s, med = O.scale_recovery(g["depth"], g["K"], float(g["cam_height"]))
        assert abs(med - float(g[f"{p}_median"])) < tol and abs(s - float(g[f"{p}_scale"][0])) < 10 * tol
        # a batch of 2 padded to 5 with copies of image 0 (dnet_layers.py:307-311)
        pad = lambda a: np.concatenate([a, np.repeat(a[:1], 3, 0)])
        s5, _ = O.scale_recovery(pad(g["depth"]), pad(g["K"]), float(g["cam_height"]))
        assert abs(s5 - float(g[f"{p}_scale_pad5"][0])) < 10 * tol


def test_postprocess_and_averaging_G8():
    """batch_post_process_disparity (learning_helpers.py:115-123) and avg_final_predictions (helpers.py:25-33) mirrors
    used on the DepthOptimizer return path"""
    import torch
    from tightly_coupled_sfm_amd.optimizer import avg_final_predictions, batch_post_process_disparity
    g = load_golden("helpers")
    assert _maxabs(batch_post_process_disparity(g["l_disp"], g["r_disp"]), g["post"]) < 1e-15
    lst = [torch.tensor(x) for x in g["avg_list"]]
    assert _maxabs(avg_final_predictions(lst, 5).numpy(), g["avg5"]) < 1e-6


def test_window_G9_initial_poses(oracle64):
    """G9: the reference's optimize_window on a B=2, S=2 window with the stand-in networks of tests/standins.py.  The
    PoseNet-in-the-loop initial poses (train_mono.py:64-80) are reproduced with the oracle's warp: pins the stacked
    fwd/inv ordering, the (tgt*valid | img_rec) assembly and disp_to_depth on a whole window."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import standins
    g = load_golden("window48x160")
    w = {k[3:]: g[k] for k in g if k.startswith("in_")}
    iters = int(w.pop("iterations"))
    S, B = w["sources"].shape[:2]
    depth = lambda d: oracle64.disp_to_depth(d, 0.06, 2.67)[1]
    d_t, d_s = depth(w["disp_t"]), [depth(w["disp_s"][i]) for i in range(S)]
    for i in range(S + 1):
        assert _maxabs((d_t if i == 0 else d_s[i - 1]) / g["out_depths_init"][i], 1.0) < 1e-6
    # stacked order: fwd pairs source-major, then inv pairs
    tgt = [w["target"][b] for _ in range(S) for b in range(B)] + [w["sources"][i][b] for i in range(S) for b in range(B)]
    src = [w["sources"][i][b] for i in range(S) for b in range(B)] + [w["target"][b] for _ in range(S) for b in range(B)]
    dt = [d_t[b, 0] for _ in range(S) for b in range(B)] + [d_s[i][b, 0] for i in range(S) for b in range(B)]
    ds = [d_s[i][b, 0] for i in range(S) for b in range(B)] + [d_t[b, 0] for _ in range(S) for b in range(B)]
    K = [w["K"][b] for _ in range(2 * S) for b in range(B)]
    pm, _ = standins.window_models(w, iters)
    x0 = torch.tensor(np.stack([np.concatenate([t, s]) for t, s in zip(tgt, src)]))
    full = pm(x0).double().numpy()
    stacked = [full.copy()]
    for _ in range(iters - 1):
        new = []
        for n in range(2 * S * B):
            rec, valid, _, _ = oracle64.warp(src[n], dt[n], ds[n], full[n], K[n])
            new.append(np.concatenate([tgt[n] * valid[None], rec]))
        full = full + pm(torch.tensor(np.stack(new), dtype=torch.float32)).double().numpy()
        stacked.append(full.copy())
    stacked = np.stack(stacked, 1)
    split = S * B
    assert _maxabs(stacked[:split], g["out_stacked_poses_init"]) < 2e-6
    assert _maxabs(stacked[split:], g["out_stacked_poses_inv_init"]) < 2e-6
    assert _maxabs(full[:split], g["out_poses_init"]) < 2e-6 and _maxabs(full[split:], g["out_poses_inv_init"]) < 2e-6
    assert _maxabs(g["out_gt_poses"], w["gt"].reshape(-1, 6)) == 0 and _maxabs(g["out_gt_poses_inv"], -w["gt"].reshape(-1, 6)) == 0


def test_window_selection_vs_reference_maps_G4(oracle64):
    """min-over-sources selection (optimizer.py:47-69) of the oracle's window mode against the selection computed from the
    reference's own fwd maps of solve_pose_iteratively (golden G4, B=2, S=2)"""
    g = load_golden("batch24x40")
    S, B = g["sources"].shape[:2]
    H, W = g["target"].shape[2:]
    poses = g["first"][:S * B]                                            # iters=1: the poses the maps were evaluated at
    mine = oracle64.window_select(g["target"], g["sources"], g["depths"][0][:, 0], g["depths"][1:][:, :, 0], g["K"], poses)
    diff = g["it1_fwd_diff_img"][:, 0].reshape(S, B, H, W)
    valid = g["it1_fwd_valid_mask"][:, 0].reshape(S, B, H, W)
    ae = g["it1_fwd_auto_mask_error"][:, 0].reshape(S, B, H, W)
    smin = np.argmin(diff, 0)                                             # first minimum, like torch.min
    keep = (valid.sum(0).clip(0, 1) > 0) & (diff.min(0) < ae.min(0))
    ref = np.stack([(keep & (smin == s)).astype(np.float64) for s in range(S)]).reshape(S * B, H, W)
    assert np.array_equal(mine, ref)
    assert 0.02 < ref.mean() < 0.6 and all(ref[s * B:(s + 1) * B].sum() > 0 for s in range(S))   # both sources get selected


def test_window_mode_reduces_to_pair_mode(oracle64):
    """without the selection (or with one source) the window refinement is the per-pair refinement in the stacked order"""
    from oracle.oracle import default_opts
    g = load_golden("batch24x40")
    S, B = g["sources"].shape[:2]
    d_t, d_s = g["depths"][0][:, 0], g["depths"][1:][:, :, 0]
    o = default_opts(n_iters=2)
    pw, _, sw = oracle64.refine_window(g["target"], g["sources"], d_t, d_s, g["K"], g["first"], o, argmin=False)
    for m in (0, 3, 5, 6):
        inv, q = m >= S * B, m % (S * B)
        s, b = divmod(q, B)
        t, sr, dt, ds = g["target"][b], g["sources"][s, b], d_t[b], d_s[s, b]
        if inv:
            t, sr, dt, ds = sr, t, ds, dt
        p, _, st = oracle64.refine(t, sr, dt, ds, g["first"][m], g["K"][b], o)
        assert _maxabs(p, pw[m]) < 1e-14 and _maxabs(st, sw[m]) < 1e-14
    # with the selection the forward pairs change (fewer pixels each), the inverse pairs do not
    pa, _, sa = oracle64.refine_window(g["target"], g["sources"], d_t, d_s, g["K"], g["first"], o, argmin=True)
    assert np.all(sa[:S * B, 0, 2] < sw[:S * B, 0, 2]) and _maxabs(pa[S * B:], pw[S * B:]) == 0
    assert _maxabs(pa[:S * B], pw[:S * B]) > 1e-7


G13_VARIANTS = (("fwd", dict(w_dc=0.0), True, "fwd"), ("fwd_inv", dict(w_dc=0.0), True, "all"), ("full", dict(w_dc=0.15), True, "all"),
                ("noargmin_full", dict(w_dc=0.15), False, "all"), ("noauto_fwd", dict(w_dc=0.0, automask=0), True, "fwd"),
                # round 4: + l_pose_consist = 0.1 (poses + poses_inv).abs().mean() (optimizer.py:95-96)
                ("full_pc", dict(w_dc=0.15, w_pose_consist=0.1), True, "all"))


@pytest.mark.parametrize("name", ["winloss24x40", "winloss48x160", "winloss28x48"])
def test_window_reference_rule_vs_reference_loss_G13(name, oracle64):
    """The REFERENCE window rule (tcsfm_opts.window_rule = 1): the scalar the window refinement minimises IS the reference's
    compute_optimization_loss (optimizer.py:47-86; batch-summed normalisers, source 0's weight map on every forward pixel,
    0.25 x inverse term, depth consistency averaged over all pairs) and every pair's gradient is the reference's autograd
    gradient w.r.t. that pair's pose -- golden G13: S = 2 sources, term by term, with and without the min over the sources."""
    g = load_golden(name)
    S, B = g["sources"].shape[:2]
    SB = S * B
    for tag, kw, argmin, which in G13_VARIANTS:
        # irls_eps -> 0: the Huberisation of the depth-consistency gradient (a documented deviation) is switched off for the pin
        op = default_opts(n_iters=1, irls_eps=1e-12, **kw)
        L = oracle64.linearize_window(g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"], g["first"], op,
                                      argmin=argmin, rule=1)
        nn = SB if which == "fwd" else 2 * SB
        ref_loss, ref_grad = float(g[f"{tag}_loss"]), g[f"{tag}_grad_pose"]
        assert abs(L["cost"][:nn].sum() - ref_loss) < 1e-12 * ref_loss, (tag, L["cost"][:nn].sum(), ref_loss)
        gp = np.stack([oracle64.euler_left_jacobian(g["first"][m]).T @ L["g"][m] for m in range(2 * SB)])
        assert _maxabs(gp[:nn], ref_grad[:nn]) < 1e-11 * np.abs(ref_grad).max(), (tag, _maxabs(gp[:nn], ref_grad[:nn]))
        if which == "fwd":
            assert _maxabs(ref_grad[SB:], 0) == 0           # (the forward term does not see the inverse poses)
    # the fixture exercises what the rule is about: the two sources' weight maps differ, and both sources win pixels
    w = g["fwd_weight_mask"].reshape(S, B, *g["target"].shape[2:])
    assert np.abs(w[0] - w[1]).mean() > 1e-3
    # ... and the per-pair rule (0) minimises a DIFFERENT scalar: its costs do not add up to the reference's loss
    op = default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15)
    L0 = oracle64.linearize_window(g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"], g["first"], op, argmin=True, rule=0)
    assert abs(L0["cost"].sum() - float(g["full_loss"])) > 1e-3


def test_pose_consistency_term_is_visible_and_lowers_its_loss(oracle64):
    """l_pose_consist under the REFERENCE rule: the term changes loss and gradients at the pin's tolerance (so the `full_pc` pin above is
    about the term), its Gauss-Newton iteration lowers the reference's loss WITH the term, and pulls p_fwd + p_inv towards zero"""
    g = load_golden("winloss24x40")
    full = (g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"])
    assert abs(float(g["full_pc_loss"]) - float(g["full_loss"])) > 1e-5 and _maxabs(g["full_pc_grad_pose"], g["full_grad_pose"]) > 1e-3 * np.abs(g["full_grad_pose"]).max()
    SB = g["sources"].shape[0] * g["sources"].shape[1]
    o1 = default_opts(n_iters=8, w_dc=0.15, w_pose_consist=0.1)        # (the damped block-Jacobi / IRLS model of the L1 term needs a few more steps than 4)
    o0 = default_opts(n_iters=8, w_dc=0.15)
    p1, _, _ = oracle64.refine_window(*full, g["first"], o1, argmin=True, rule=1)
    p0, _, _ = oracle64.refine_window(*full, g["first"], o0, argmin=True, rule=1)
    L = lambda p: oracle64.linearize_window(*full, p, o1, argmin=True, rule=1)["cost"].sum()
    assert L(p1) < L(g["first"]) and L(p1) < L(p0)
    r = lambda p: np.abs(p[:SB] + p[SB:]).mean()
    assert r(p1) < r(p0)


def test_window_reference_rule_refines_and_reduces(oracle64):
    """rule 1 with one source and one target is the per-pair problem up to the constant factors of the reference's loss (they
    cancel in a Marquardt-damped step); with S = 2 it lowers the reference's loss"""
    g = load_golden("winloss24x40")
    S, B = g["sources"].shape[:2]
    SB = S * B
    a = (g["target"][:1], g["sources"][:1, :1], g["depth_t"][:1, 0], g["depth_s"][:1, :1, 0], g["K"][:1], g["first"][[0, SB]])
    o = default_opts(n_iters=3)
    p0, _, _ = oracle64.refine_window(*a, o, argmin=True, rule=0)
    p1, _, _ = oracle64.refine_window(*a, o, argmin=True, rule=1)
    assert _maxabs(p0, p1) < 1e-9
    full = (g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"])
    o = default_opts(n_iters=4, w_dc=0.15)
    p, _, st = oracle64.refine_window(*full, g["first"], o, argmin=True, rule=1)
    before = oracle64.linearize_window(*full, g["first"], o, argmin=True, rule=1)["cost"].sum()
    after = oracle64.linearize_window(*full, p, o, argmin=True, rule=1)["cost"].sum()
    assert after < 0.9 * before, (before, after)
    assert abs(st[:, 0, 0].sum() - before) < 1e-12


@pytest.mark.parametrize("name", ["winloss24x40", "winloss48x160", "winloss28x48"])
def test_joint_dense_gradients_vs_reference_autograd_G13(name, oracle64):
    """joint dense mode (ONE inverse-depth map per target frame, shared by its S forward pairs -- optimizer.py:194-198,235-247):
    the gradient of the forward term of the reference's loss w.r.t. the SHARED target depth and w.r.t. the S poses equals reference
    autograd (golden G13), with the min over the sources (weight map of source 0 as optimizer.py:69 has it, or of the winning
    source: the two window rules) and without it (:71-73);
    with one source the joint linearisation IS the pair-form dense linearisation"""
    g = load_golden(name)
    S, B = g["sources"].shape[:2]
    op = default_opts(n_iters=1)
    # fwd: the reference's forward term as written (weight map of source 0 on every pixel); fwd_ownw: the same with every pixel
    # weighted by the map of the source that won it -- the cost of the HIP joint mode; noargmin_fwd: without the min over the sources
    for tag, argmin, factor, rule in (("fwd", True, 1.0, 1), ("fwd_ownw", True, 1.0, 0), ("noargmin_fwd", False, 0.25, 0)):
        parts = [oracle64.linearize_dense_joint(g["target"][b], g["sources"][:, b], g["depth_t"][b, 0], g["depth_s"][:, b, 0], g["K"][b],
                                                g["first"][[s * B + b for s in range(S)]], op, argmin=argmin, rule=rule) for b in range(B)]
        Ktot = sum(L["K"] for L in parts)                     # the reference normalises over the batch; the joint problem per target
        loss = factor * sum(L["cost_photo"] * L["K"] for L in parts) / Ktot
        assert abs(loss - float(g[f"{tag}_loss"])) < 1e-12 * loss
        for b in range(B):
            gd = -factor * parts[b]["g_rho"] * parts[b]["K"] / Ktot / g["depth_t"][b, 0] ** 2          # d / d depth = -rho^2 d / d rho
            ref = g[f"{tag}_grad_depth_t"][b]
            assert _maxabs(gd, ref) < 1e-11 * np.abs(ref).max(), (tag, b, _maxabs(gd, ref))
            # pose gradients: with the depth block frozen (lambda_depth -> infinity) the reduced system is the pose system itself
            Lf = oracle64.linearize_dense_joint(g["target"][b], g["sources"][:, b], g["depth_t"][b, 0], g["depth_s"][:, b, 0], g["K"][b],
                                                g["first"][[s * B + b for s in range(S)]], op, argmin=argmin, lambda_depth=1e30, rule=rule)
            for s in range(S):
                m = s * B + b
                gp = factor * Lf["K"] / Ktot * (oracle64.euler_left_jacobian(g["first"][m]).T @ Lf["g"][6 * s:6 * s + 6])
                assert _maxabs(gp, g[f"{tag}_grad_pose"][m]) < 1e-11 * np.abs(g[f"{tag}_grad_pose"]).max(), (tag, m)
        # the reduced camera system: 6S x 6S.  Under the min over the sources every pixel counts for exactly one source and the
        # off-diagonal blocks vanish identically; without it the shared depth couples the poses
        off = np.abs(parts[0]["H"][:6, 6:]).max() / np.abs(parts[0]["H"]).max()
        assert (off == 0.0) if argmin else (off > 0.05), (tag, off)
    b = 0
    kw = dict(lambda_depth=0.3, w_prior=10.0, depth0=g["depth_t"][b, 0] * 1.01)
    L1 = oracle64.linearize_dense_joint(g["target"][b], g["sources"][:1, b], g["depth_t"][b, 0], g["depth_s"][:1, b, 0], g["K"][b], g["first"][[b]], op, **kw)
    Lp = oracle64.linearize_dense(g["target"][b], g["sources"][0, b], g["depth_t"][b, 0], g["depth_s"][0, b, 0], g["first"][b], g["K"][b], op, **kw)
    assert _maxabs(L1["H"], Lp["H"]) < 1e-13 * np.abs(Lp["H"]).max() and _maxabs(L1["g"], Lp["g"]) < 1e-15 and _maxabs(L1["g_rho"], Lp["g_rho"]) < 1e-16
    assert _maxabs(L1["D"], Lp["D"]) < 1e-16 and abs(L1["cost"] - Lp["cost"]) < 1e-15


@pytest.mark.parametrize("rule,nit", [(0, 4), (0, 8), (1, 16)])
def test_joint_dense_refinement_beats_per_pair_copies(rule, nit, oracle64):
    """the joint problem (one shared depth map, 6S x 6S reduced system) ends at a lower value of ITS cost than the per-pair-copy mode
    (every forward pair refines its own copy of the target depth; inverse depths averaged afterwards) from the same start.
    With the winning source's own weight map (window rule PAIR, the default) already after 4 Gauss-Newton iterations; with the
    reference's weighting (source 0's map on every pixel, optimizer.py:69) the pose of source 0 carries a gradient term from the
    pixels the other source won that the Gauss-Newton curvature cannot model (the weight 1 - dd is concave in the pose), the
    iteration is slower and overtakes the copies only towards convergence -- numbers: DESIGN.md section 2."""
    g = load_golden("winloss48x160")
    S, B = g["sources"].shape[:2]
    n_fwd = S * B
    d_t, d_s = g["depth_t"][:, 0] * 1.03, g["depth_s"][:, :, 0]                 # start from a biased target depth
    a = (g["target"], g["sources"], d_t, d_s, g["K"])
    o = default_opts(n_iters=nit)
    kw = dict(lambda_depth=1.0, w_prior=10.0, min_depth=0.06, max_depth=2.67)
    pj, dj, st = oracle64.refine_dense_joint(*a, g["first"][:n_fwd], o, argmin=True, rule=rule, **kw)
    assert st[0, nit - 1, 0] < st[0, 0, 0]
    pw, dw, _ = oracle64.refine_dense_window(*a, g["first"], o, argmin=True, **kw)
    avg = 1.0 / (1.0 / dw[:n_fwd]).reshape(S, B, *d_t.shape[1:]).mean(0)        # what optimizer.py did with the copies (r02)
    cost = lambda poses, depth: oracle64.linearize_dense_joint(g["target"][0], g["sources"][:, 0], depth[0], d_s[:, 0], g["K"][0], poses[[s * B for s in range(S)]],
                                                               default_opts(n_iters=1), argmin=True, w_prior=10.0, depth0=d_t[0], rule=rule)["cost"]
    c0, cj, cw = cost(g["first"], d_t), cost(pj, dj), cost(pw, avg)
    assert cj < c0 and cj < cw, (c0, cj, cw)


def test_torch_twin_vs_reference_golden():
    """oracle/torch_twin.py (the reference-style Adam/autograd step that bench.py times on the host cores) against the
    reference's own float64 outputs: maps, cost and autograd gradient (goldens G1-G3, G6)"""
    import torch
    from oracle import torch_twin as tw
    g = load_golden("s24x40")
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    tgt, src, dt, ds, K = T(g["tgt"])[None], T(g["src"])[None], T(g["depth_t"])[None, None], T(g["depth_s"])[None, None], T(g["K"])[None]
    for k in range(len(g["poses"])):
        pose = T(g["poses"][k])[None].clone().requires_grad_()
        rec, valid, pd, cd = tw.warp(src, dt, ds, -pose, K)
        vbad = valid[0, 0].numpy() != g["f64_valid"][k]
        if k == IDENTITY:         # border pixels on x_n = +-1 +- 1 ulp: decided by the host BLAS's rounding order, as in test_warp_G1
            assert _border_only(vbad)
        else:
            assert not vbad.any()
        ok = ~vbad
        assert _maxabs(rec[0].detach().numpy()[:, ok], g["f64_rec"][k][:, ok]) < 1e-10
        assert _maxabs(pd[0, 0].detach().numpy()[ok], g["f64_proj_depth"][k][ok]) < 1e-10 and _maxabs(cd[0, 0].detach(), g["f64_comp_depth"][k]) < 1e-10
        r = tw.photometric(tgt, src, dt, ds, pose, K)
        assert _maxabs(r["weight"][0, 0].detach().numpy()[ok], g["f64_weight"][k][ok]) < 1e-10
        if vbad.any():            # a flipped border pixel moves the diff of its 3x3 neighbourhood; at the identity the auto-mask is a tie
            continue              # everywhere: diff, mask and cost are compared only without a flip (test_photometric_G3 / G6)
        assert _maxabs(r["diff"][0, 0].detach(), g["f64_diff"][k]) < 1e-10
        assert np.array_equal(r["mask"][0, 0].numpy(), g["f64_mask"][k])
        if float(r["mask"].sum()) > 0:
            c = tw.masked_cost(r)
            assert abs(float(c.detach()) - float(g["f64_cost"][k])) < 1e-12
            c.backward()
            assert _maxabs(pose.grad[0], g["f64_grad_pose"][k]) < 1e-10 * max(1.0, np.abs(g["f64_grad_pose"][k]).max())
    assert _maxabs(tw.ssim(tgt, src)[0], g["f64_ssim_ts"]) < 1e-12
    # and the timed step runs: two steps on a tiny window
    from tightly_coupled_sfm_amd import synth
    p = synth.make_pair(24, 40, seed=3)
    F32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    sig = lambda d: F32(synth.depth_to_sigmoid_disp(d.astype(np.float64)))[None, None]
    rate, steps = tw.time_adam_steps(F32(p["tgt"])[None], F32(p["src"])[None], sig(p["depth_t"]), sig(p["depth_s"]), F32(p["K"])[None],
                                     F32(synth.perturb_pose(p["pose_gt"], 3))[None], seconds=0.05, threads=1)
    assert steps >= 1 and rate > 0


def test_oracle_vs_torch_twin_random_sweep(oracle64):
    """two independent CPU restatements of the reference residual -- the C oracle and the torch twin, each pinned on the goldens
    -- against each other on random sizes, intrinsics and poses (incl. large ones): maps, cost and gradient"""
    import torch
    from oracle import torch_twin as tw
    from oracle.oracle import default_opts
    from tightly_coupled_sfm_amd import synth
    rng = np.random.default_rng(5)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    for case in range(10):
        H, W = int(rng.integers(9, 40)), int(rng.integers(12, 70))
        K = synth.scaled_K(H, W); K[0, 0] *= rng.uniform(0.8, 1.3); K[1, 1] *= rng.uniform(0.8, 1.3); K[0, 2] += rng.normal(scale=2); K[1, 2] += rng.normal(scale=1)
        p = synth.make_pair(H, W, seed=600 + case, K=K, dtype=np.float64)
        pose = p["pose_gt"] + rng.normal(scale=[0.004, 0.004, 0.01, 0.004, 0.01, 0.004]) * rng.choice([1.0, 6.0])
        tgt, src, dt, ds, Kt = T(p["tgt"])[None], T(p["src"])[None], T(p["depth_t"])[None, None], T(p["depth_s"])[None, None], T(p["K"])[None]
        pt = T(pose)[None].clone().requires_grad_()
        r = tw.photometric(tgt, src, dt, ds, pt, Kt)
        o = oracle64.photometric(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"])
        assert _maxabs(r["diff"][0, 0].detach(), o["diff"]) < 1e-10 and _maxabs(r["weight"][0, 0].detach(), o["weight"]) < 1e-10
        assert _maxabs(r["rec"][0].detach(), o["rec"]) < 1e-10
        assert np.mean(r["mask"][0, 0].numpy() != o["valid"] * o["auto_mask"]) < 0.01          # exact ties only
        lin = oracle64.linearize(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"], default_opts())
        if lin["n_mask"] < 10 or not np.array_equal(r["mask"][0, 0].numpy(), o["valid"] * o["auto_mask"]):
            continue
        c = tw.masked_cost(r)
        assert abs(float(c.detach()) - lin["cost"]) < 1e-11
        c.backward()
        gp = oracle64.euler_left_jacobian(pose).T @ lin["g"]
        assert _maxabs(pt.grad[0], gp) < 1e-8 * max(1.0, np.abs(gp).max())


def test_dense_depth_gradient_vs_reference_autograd_G6(oracle64):
    """dense mode: d cost / d (inverse depth of every target pixel) of the oracle (adjoint form) equals the reference's autograd
    d loss / d depth_t (golden G6) through the chain rule rho = 1 / depth; so does the pose block"""
    from oracle.oracle import default_opts
    g = load_golden("jac24x40")
    r = oracle64.linearize_dense(g["tgt"], g["src"], g["depth_t"], g["depth_s"], g["pose"], g["K"], default_opts(), lambda_depth=0.0, w_prior=0.0)
    assert abs(r["cost"] - float(g["cost"])) < 1e-12
    ref = -g["grad_depth_t"] * g["depth_t"] ** 2                       # dC/drho = dC/dD dD/drho = -D^2 dC/dD
    assert _maxabs(r["g_rho"], ref) < 1e-12 * np.abs(ref).max()
    assert np.count_nonzero(ref) > 0.3 * ref.size
    # the Schur-reduced pose gradient with the depth block switched off (D = 0 pixels) must reduce to the pose-mode gradient
    lin = oracle64.linearize(g["tgt"], g["src"], g["depth_t"], g["depth_s"], g["pose"], g["K"], default_opts())
    full_g = lin["g"]
    back = r["g"] + np.einsum("hwj,hw->j", r["B"], np.where(r["D"] > 1e-30, r["g_rho"] / np.where(r["D"] > 1e-30, r["D"], 1.0), 0.0))
    assert _maxabs(back, full_g) < 1e-9 * np.abs(full_g).max()          # g_S + sum B g_rho / D = g_xi


def test_dense_depth_gradient_vs_torch_twin_random(oracle64):
    """the same identity on random cases against autograd through the torch twin"""
    import torch
    from oracle import torch_twin as tw
    from oracle.oracle import default_opts
    from tightly_coupled_sfm_amd import synth
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    checked = 0
    for case in range(6):
        H, W = 14 + 3 * case, 30 + 7 * case
        p = synth.make_pair(H, W, seed=700 + case, dtype=np.float64)
        pose = synth.perturb_pose(p["pose_gt"], 700 + case, sigma_t=0.003, sigma_r=0.001)
        d = T(p["depth_t"])[None, None].clone().requires_grad_()
        r = tw.photometric(T(p["tgt"])[None], T(p["src"])[None], d, T(p["depth_s"])[None, None], T(pose)[None], T(p["K"])[None])
        o = oracle64.linearize_dense(p["tgt"], p["src"], p["depth_t"], p["depth_s"], pose, p["K"], default_opts(), lambda_depth=0.0, w_prior=0.0)
        if float(r["mask"].sum()) != o["n_mask"]:
            continue
        tw.masked_cost(r).backward()
        ref = -d.grad[0, 0].numpy() * p["depth_t"] ** 2
        assert _maxabs(o["g_rho"], ref) < 1e-9 * np.abs(ref).max(), case
        checked += 1
    assert checked >= 4


def test_optimization_loss_mirror_on_reference_maps_G5():
    """losses.compute_optimization_loss (the mirror of optimizer.py:29-134) fed with the REFERENCE's own fwd / inv maps of
    solve_pose_iteratively (golden G4), in float64 on the CPU: every option toggle reproduces the reference's scalar (G5)
    -- pins the loss assembly itself (min over sources, union mask, weight-map quirk, 0.25 / 0.15 / 0.1 weights) without a GPU"""
    import torch
    from oracle import torch_twin as tw
    from tightly_coupled_sfm_amd.losses import compute_optimization_loss
    g = load_golden("batch24x40")
    S = g["sources"].shape[0]
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    base = {'diff_img_argmin': True, 'automasking': True, 'l_depth_consist': True, 'l_depth_consist_weight': 0.15,
            'l_depth_init': True, 'l_depth_init_weight': 0.1, 'l_inverse_reconstruction': True, 'l_smooth': False,
            'l_smooth_weight': 2, 'l_pose_consist': False, 'num_source_imgs': S}
    for iters in (1, 4):
        part = lambda d: {k: T(g[f"it{iters}_{d}_{k}"]) for k in ("diff_img", "valid_mask", "weight_mask", "auto_mask_error", "auto_mask", "poses")}
        fwd, inv = part("fwd"), part("inv")
        for tag, upd in (("default", {}), ("noargmin", {'diff_img_argmin': False}), ("noauto", {'automasking': False}),
                         ("noinv", {'l_inverse_reconstruction': False}), ("nodc", {'l_depth_consist': False}),
                         ("smooth", {'l_smooth': True}), ("posec", {'l_pose_consist': True}), ("noinit", {'l_depth_init': False})):
            loss = compute_optimization_loss(dict(base, **upd), T(g["target"]), T(g["loss_disp"]), T(g["loss_disp0"]), fwd, inv, tw.ssim)
            ref = float(g[f"it{iters}_loss_{tag}"])
            assert abs(float(loss.reshape(-1)[0]) - ref) < 1e-12 * max(1.0, abs(ref)), (iters, tag)


def test_pose_vec2mat_a3(oracle64):
    """pose_vec2mat / euler2mat (stn.py:81-116,143-158) of the reference on random 6-vectors incl. large angles: the oracle's
    pose_to_T, the library's host utility and the torch drop-in all reproduce it"""
    import torch
    from tightly_coupled_sfm_amd import engine as E, stn
    g = load_golden("helpers")
    for v, M in zip(g["pose_vec"], g["pose_mat"]):
        assert _maxabs(np.asarray(oracle64.pose_to_T(-v)).reshape(3, 4), M) < 1e-14      # pose_to_T(p) == pose_vec2mat(-p), the call sites' form
        assert _maxabs(E.pose_to_matrix(-v), M) < 1e-14
        assert _maxabs(E.matrix_to_pose(M), -v) < 1e-9 or abs(v[4]) > 1.5               # inverse map (inside the Euler chart)
    assert _maxabs(stn.pose_vec2mat(torch.tensor(g["pose_vec"])).numpy(), g["pose_mat"]) < 1e-14


@pytest.mark.parametrize("name", ["winloss24x40", "winloss48x160", "winloss28x48"])
def test_dense_reference_loss_and_gradients_vs_reference_autograd_G13(name, oracle64):
    """round 4: the dense mode's restatement of the reference's COMPLETE loss (optimizer.py:47-90: forward term with source 0's
    weight map, 0.25 x inverse term, depth consistency of both directions, l_depth_init = SSIM between the target's current and
    initial sigmoid disparity) -- its value, its gradient w.r.t. the pose of every directed pair and w.r.t. the SHARED target depth,
    which the inverse pairs see through their bilinear SAMPLE of it (the adjoint scatter), equal reference autograd (golden G13
    variants `full`, `noargmin_full`, `fullinit`)"""
    g = load_golden(name)
    S, B = g["sources"].shape[:2]
    SB = S * B
    a = (g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"], g["first"])
    mind, maxd = (float(x) for x in g["min_max_depth"])
    rd = 1.0 / mind - 1.0 / maxd
    for tag, argmin, w_init in (("full", True, 0.0), ("noargmin_full", False, 0.0), ("fullinit", True, 0.1), ("fullinit_smooth", True, 0.1), ("full_pc", True, 0.0)):
        op = default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15)      # (irls_eps -> 0: no Huberisation of the depth-consistency gradient for the pin)
        if tag == "fullinit_smooth":
            op.w_smooth = 2.0          # round 4: + l_smooth_weight (2) x get_smooth_loss(target disparity, target image), optimizer.py:92-93
        if tag == "full_pc":
            op.w_pose_consist = 0.1    # round 5: + 0.1 (poses + poses_inv).abs().mean() as a term of the dense mode, optimizer.py:95-96
        depth0 = None if w_init == 0 else 1.0 / (1.0 / maxd + rd * g["sig_t0"])
        L = oracle64.linearize_dense_ref(*a, op, argmin=argmin, w_init=w_init, depth0=depth0, min_depth=mind, max_depth=maxd)
        ref_loss = float(g[f"{tag}_loss"])
        assert abs(L["loss"] - ref_loss) < 1e-12 * ref_loss, (tag, L["loss"], ref_loss)
        gp = np.stack([oracle64.euler_left_jacobian(g["first"][m]).T @ L["g_xi"][m] for m in range(2 * SB)])
        ref_gp = g[f"{tag}_grad_pose"]
        assert _maxabs(gp, ref_gp) < 1e-10 * np.abs(ref_gp).max(), (tag, _maxabs(gp, ref_gp), np.abs(ref_gp).max())
        if tag == "full":            # d / d depth = -rho^2 d / d rho
            gd, ref = -L["g_rho"] / g["depth_t"][:, 0] ** 2, g["full_grad_depth_t"]
            assert _maxabs(gd, ref) < 1e-10 * np.abs(ref).max(), (tag, _maxabs(gd, ref), np.abs(ref).max())
            # the SOURCE depth maps -- leaves of the reference's optimize_depth_pred that the engine holds fixed: local in their inverse pair,
            # sampled by their forward pair (whose weight map multiplies every selected pixel under argmin); equal to reference autograd too
            gds, refs = -L["g_rho_s"] / g["depth_s"][:, :, 0] ** 2, g["full_grad_depth_s"]
            assert _maxabs(gds, refs) < 1e-10 * np.abs(refs).max(), (tag, _maxabs(gds, refs), np.abs(refs).max())
            assert np.abs(refs).max() > 0.1 * np.abs(ref).max()        # (not a negligible part of the loss's gradient)
        if tag == "fullinit_smooth":     # the smoothness term through the shared map, incl. the mean-normalisation's per-image constant
            gs, ref = L["g_rho"] * rd, g["fullinit_smooth_grad_sig_t"]
            assert _maxabs(gs, ref) < 1e-10 * np.abs(ref).max(), (tag, _maxabs(gs, ref), np.abs(ref).max())
            assert _maxabs(ref, g["fullinit_grad_sig_t"]) > 0.05 * np.abs(ref).max()       # (the term is visible at the pin's tolerance)
        if tag == "fullinit":        # d / d sigma = r d / d rho; the prior's own value
            gs, ref = L["g_rho"] * rd, g["fullinit_grad_sig_t"]
            assert _maxabs(gs, ref) < 1e-10 * np.abs(ref).max(), (tag, _maxabs(gs, ref), np.abs(ref).max())
            assert abs(L["L_init"] - float(g["fullinit_init_term"])) < 1e-13
            assert np.abs(ref - g["full_grad_depth_t"] * (-g["depth_t"][:, 0] ** 2) * rd).max() > 1e-3 * np.abs(ref).max()   # (the prior's gradient is visible at the pin's tolerance)
    # the scatter terms are a visible part of the depth gradient: without the inverse pairs' samples the pin would fail at the 1e-2 level
    Lf = oracle64.linearize_dense_ref(*a, default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15), argmin=True, min_depth=mind, max_depth=maxd)
    fwd_only = [oracle64.linearize_dense_joint(g["target"][b], g["sources"][:, b], g["depth_t"][b, 0], g["depth_s"][:, b, 0], g["K"][b],
                                               g["first"][[s * B + b for s in range(S)]], default_opts(n_iters=1), argmin=True, rule=1) for b in range(B)]
    Kt = sum(x["K"] for x in fwd_only)
    g_fwd = np.stack([x["g_rho"] * x["K"] / Kt for x in fwd_only])
    assert np.abs(Lf["g_rho"] - g_fwd).max() > 0.02 * np.abs(Lf["g_rho"]).max()


def test_dense_reference_refinement_lowers_the_reference_loss(oracle64):
    """Gauss-Newton on the reference's loss over poses and the shared depth: the loss falls from linearisation to linearisation, the
    prior keeps the map near its start, and a model check -- the predicted decrease of the first step has the sign and the order of
    the realised one"""
    g = load_golden("winloss48x160")
    a = (g["target"], g["sources"], g["depth_t"][:, 0] * 1.03, g["depth_s"][:, :, 0], g["K"], g["first"])
    o = default_opts(n_iters=5, w_dc=0.15)
    p, d, st = oracle64.refine_dense_ref(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    assert np.all(np.diff(st[:, 0]) < 0), st[:, 0]
    assert st[-1, 0] < 0.93 * st[0, 0]
    # (where the photometric term is masked out the depth-consistency term alone drives the depth towards the -- deliberately
    # inconsistent -- source maps of this fixture: large changes at a few pixels are the loss's own minimum, the bulk moves by per cents)
    rel = np.abs(d / a[2] - 1)
    assert np.isfinite(p).all() and np.isfinite(d).all() and 0 < np.median(rel) < 0.05 and rel.max() < 1.25 ** 5


def test_dense_reference_refinement_with_free_source_maps(oracle64):
    """orc_refine_dense_ref_free: the source depth maps as unknowns too (every inverse pair a group of its pose and the map it back-projects,
    the adjoint of the forward pair's samples in its gradient -- the gradient pinned on reference autograd above): the loss falls from
    linearisation to linearisation and further than with the sources held fixed; with zero iterations nothing moves"""
    g = load_golden("winloss48x160")
    a = (g["target"], g["sources"], g["depth_t"][:, 0] * 1.03, g["depth_s"][:, :, 0], g["K"], g["first"])
    o = default_opts(n_iters=5, w_dc=0.15)
    p1, d1, ds1, st1 = oracle64.refine_dense_ref_free(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    p0, d0, st0 = oracle64.refine_dense_ref(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    assert np.all(np.diff(st1[:, 0]) < 0), st1[:, 0]
    assert st1[0, 0] == st0[0, 0] and np.all(st1[1:, 0] < st0[1:, 0]), (st1[:, 0], st0[:, 0])
    rel = np.abs(ds1 / a[3] - 1)
    assert np.isfinite(p1).all() and np.isfinite(ds1).all() and 0 < np.median(rel) < 0.1 and rel.max() < 1.25 ** 5
    # the first linearisation does not depend on which maps are free: same loss terms
    assert np.array_equal(st1[0], st0[0])
    # the reference's own parametrisation of all of them (quarter-resolution maps of target and sources): the loss falls as well, the returned
    # source maps are x4 upsamplings (linear across the pixels 4c+2 .. 4c+5 of a row)
    p2, d2, ds2, st2 = oracle64.refine_dense_ref_q_free(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    assert np.all(np.diff(st2[:, 0]) < 0), st2[:, 0]
    rho = 1.0 / ds2[0, 0]
    assert np.abs(rho[:, 2:-4:4] - 2 * rho[:, 3:-3:4] + rho[:, 4:-2:4]).max() < 1e-12 * np.abs(rho).max()
    assert np.isfinite(p2).all() and np.abs(ds2 / a[3] - 1).max() > 1e-3


@pytest.mark.parametrize("name", ["winloss24x40", "winloss48x160", "winloss28x48"])
def test_quarter_resolution_parametrisation_vs_reference_G13(name, oracle64):
    """round 4: the reference's own parametrisation of optimize_depth_pred (optimizer.py:194-198, 235-239) -- the leaf is the QUARTER-
    resolution sigmoid disparity, upsampled x4 (bilinear) every epoch.  (a) the oracle's down / up-sampling weights are torch's (the
    fixture holds F.interpolate's outputs); (b) at the upsampled maps the oracle's loss and pose gradients equal the reference's, and
    its full-resolution depth gradient carried through the TRANSPOSE of the upsampling equals reference autograd w.r.t. the quarter-
    resolution leaf (golden G13 `qinit`)"""
    g = load_golden(name)
    S, B = g["sources"].shape[:2]
    SB = S * B
    mind, maxd = (float(x) for x in g["min_max_depth"])
    rd = 1.0 / mind - 1.0 / maxd
    sig_full = np.concatenate([g["sig_t"][:, None], np.transpose((1.0 / g["depth_s"][:, :, 0] - 1.0 / maxd) / rd, (1, 0, 2, 3))], 1)    # [B, S+1, H, W]
    for b in range(B):
        for c in range(S + 1):
            assert _maxabs(oracle64.down4(sig_full[b, c]), g["q_sig"][b, c]) < 1e-15
            assert _maxabs(oracle64.up4(g["q_sig"][b, c]), g["q_up"][b, c]) < 1e-15
    depth_of = lambda sig: 1.0 / (1.0 / maxd + rd * sig)
    depth_t = depth_of(g["q_up"][:, 0])
    depth_s = np.stack([depth_of(g["q_up"][:, 1 + s]) for s in range(S)])
    op = default_opts(n_iters=1, irls_eps=1e-12, w_dc=0.15)
    L = oracle64.linearize_dense_ref(g["target"], g["sources"], depth_t, depth_s, g["K"], g["first"], op, argmin=True, w_init=0.1,
                                     depth0=depth_of(g["sig_t0"]), min_depth=mind, max_depth=maxd)
    ref_loss = float(g["qinit_loss"])
    assert abs(L["loss"] - ref_loss) < 1e-12 * ref_loss, (L["loss"], ref_loss)
    gp = np.stack([oracle64.euler_left_jacobian(g["first"][m]).T @ L["g_xi"][m] for m in range(2 * SB)])
    assert _maxabs(gp, g["qinit_grad_pose"]) < 1e-10 * np.abs(g["qinit_grad_pose"]).max()
    gq = np.stack([oracle64.up4_adjoint(L["g_rho"][b] * rd) for b in range(B)])           # d / d sigma_q = U' (r d / d rho)
    ref = g["qinit_grad_q"][:, 0]
    assert _maxabs(gq, ref) < 1e-10 * np.abs(ref).max(), (_maxabs(gq, ref), np.abs(ref).max())
    # the source channels of the reference's quarter-resolution leaf (held fixed by the engine): the same chain on the source maps' gradient
    for s_ in range(S):
        gqs = np.stack([oracle64.up4_adjoint(L["g_rho_s"][s_, b] * rd) for b in range(B)])
        refs = g["qinit_grad_q"][:, 1 + s_]
        assert _maxabs(gqs, refs) < 1e-10 * np.abs(refs).max(), (s_, _maxabs(gqs, refs), np.abs(refs).max())
    # (a quarter-resolution cell gathers ~16 pixels' gradients: the chain rule is not a formality at the pin's tolerance)
    assert np.abs(gq - (L["g_rho"] * rd)[:, 1::4, 1::4]).max() > 0.5 * np.abs(gq).max()


def test_quarter_resolution_refinement_lowers_the_reference_loss(oracle64):
    """Gauss-Newton in the reference's parametrisation (quarter-resolution map, lumped cell curvature): the loss falls from linearisation
    to linearisation; the returned map IS the x4 upsampling of the returned quarter-resolution unknown; the start is the projection of
    the input (optimizer.py:194-196), not the input itself"""
    g = load_golden("winloss48x160")
    d_in = g["depth_t"][:, 0] * 1.03
    a = (g["target"], g["sources"], d_in, g["depth_s"][:, :, 0], g["K"], g["first"])
    o = default_opts(n_iters=5, w_dc=0.15)
    p, d, st, rq = oracle64.refine_dense_ref_q(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    assert np.all(np.diff(st[:, 0]) < 0), st[:, 0]
    assert st[-1, 0] < 0.95 * st[0, 0]
    for b in range(d.shape[0]):
        assert _maxabs(1.0 / oracle64.up4(rq[b]), d[b]) < 1e-12
    p0, d0, st0, rq0 = oracle64.refine_dense_ref_q(*a, default_opts(n_iters=0, w_dc=0.15), argmin=True, w_init=0.1, lambda_depth=1.0)
    assert _maxabs(rq0[0], oracle64.down4(1.0 / d_in[0])) < 1e-15 and _maxabs(d0, d_in) > 1e-5 and np.allclose(p0, g["first"])
    # the full-resolution mode reaches a lower loss in the same number of steps (16 x the unknowns); both start from a comparable value
    pf, df, stf = oracle64.refine_dense_ref(*a, o, argmin=True, w_init=0.1, lambda_depth=1.0)
    assert stf[-1, 0] < st[-1, 0] and abs(stf[0, 0] - st[0, 0]) < 0.05 * st[0, 0]
