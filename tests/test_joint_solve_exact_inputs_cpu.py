"""Host-only conditions of tests/joint_solve_exact_inputs.py: every case is what its name claims, the JointState mirrors have the library's
size, the golden condition constant recomputes, the judge passes the clean float64 stand-in on every case (under half of the bar) and
fails each planted fault of the stand-in on at least one."""
import ctypes as C

import numpy as np
import pytest

import joint_solve_exact_inputs as JX
import solve_exact_inputs as SX


def _standin_with(fault):
    return lambda c: JX.standin(c, fault)


def test_struct_mirrors_have_the_librarys_sizes():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    ss, sc, sj = _lib.debug_solve_joint_layout()
    assert (ss, sc) == _lib.debug_solve_layout() == (SX.STATE_DT.itemsize, SX.CONST_DT.itemsize)
    assert sj == C.sizeof(_lib.JointState) == JX.JS_DT.itemsize == 24 + 8 * 24 * 25
    for name, _ in _lib.JointState._fields_:
        assert getattr(_lib.JointState, name).offset == JX.JS_DT.fields[name][1], name


def test_args_structs_match_the_header():
    """tcsfm_debug_joint_group / tcsfm_debug_solve_joint_args as the C compiler lays them out against the ctypes mirrors; the pose hook's
    prototype is still there"""
    import os, subprocess, tempfile
    from conftest import REPO
    from tightly_coupled_sfm_amd import _lib
    gn = ["B", "n0", "c_f", "records", "js", "export_out", "jtick"]
    an = ["variant", "c_len", "w_pc", "a", "b", "state", "stats", "pose_lin", "c_pose_out"]
    protos = '#include "tcsfm.h"\nint (*keep1)(tcsfm_handle, const tcsfm_opts *, tcsfm_debug_solve_joint_args *) = tcsfm_debug_solve_joint;\n' \
             'int (*keep2)(int *, int *) = tcsfm_debug_solve_layout;\nint (*keep3)(int *, int *, int *) = tcsfm_debug_solve_joint_layout;\n'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tcsfm.h"\nint main(void){printf("%zu", sizeof(tcsfm_debug_joint_group));' + \
          "".join(f'printf(" %zu", offsetof(tcsfm_debug_joint_group, {n}));' for n in gn) + 'printf(" %zu", sizeof(tcsfm_debug_solve_joint_args));' + \
          "".join(f'printf(" %zu", offsetof(tcsfm_debug_solve_joint_args, {n}));' for n in an) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(protos)
        open(os.path.join(d, "s.c"), "w").write(src)
        inc = "-I" + os.path.join(REPO, "include")
        subprocess.check_call(["gcc", "-std=c99", "-Werror", "-c", inc, os.path.join(d, "p.c"), "-o", os.path.join(d, "p.o")])      # the prototypes, as declared
        subprocess.check_call(["gcc", "-std=c99", inc, os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    G, A = _lib.DebugJointGroup, _lib.DebugSolveJointArgs
    assert got == [C.sizeof(G)] + [getattr(G, n).offset for n in gn] + [C.sizeof(A)] + [getattr(A, n).offset for n in an]
    assert A.c_pose_out.size == SX.TC_MAX_COAL * C.sizeof(C.c_void_p)
    assert "tcsfm_debug_solve_joint" in _lib.EXPORTS and "tcsfm_debug_solve_joint_layout" in _lib.EXPORTS and "tcsfm_debug_solve_layout" in _lib.EXPORTS


def test_split_and_counts_follow_the_kernel():
    assert [JX.split(s) for s in (1, 2, 3, 4)] == [(32, 16), (8, 32), (4, 32), (2, 32)]
    assert [JX.layout(s).NACC for s in (1, 2, 3, 4)] == [32, 97, 198, 335]
    assert JX.sweep_nblk(1) == [1, 2, 31, 32, 33, 511, 512, 513, 1027] and JX.sweep_nblk(4) == [1, 2, 3, 63, 64, 65, 131]
    assert JX.shares(9, 8) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9), (9, 9), (9, 9), (9, 9)] and JX.shares(1, 3) == [(0, 1), (1, 1), (1, 1)]
    assert JX.n_terms(481, 2) == 243 and JX.n_terms(5, 1) == 5
    names = {c.name for c in JX.all_cases()}
    for NS in (1, 2, 4):
        for G in (2, 3, 4, 8):
            for nblk in (1, G - 1, G, G + 1, 480, 481, 1833):
                for B in (1, 3):
                    assert f"split S{NS} G{G} nblk{nblk} B{B}" in names


def test_sweep_and_split_records_are_distinct_enough():
    """one record dropped or doubled moves every live sum by more than 1000 times its bound; the slack target is NaN; counts are integers"""
    for c in JX.all_cases():
        if not ({"sweep", "split"} & set(c.claims)):
            continue
        g = c.groups[0]
        L = JX.layout(g.NS)
        v = g.rec[:g.B].astype(np.float64)
        assert np.all(np.isnan(g.rec[g.B:])) and np.all(np.isfinite(v))
        bound = (JX.n_terms(g.nblk, g.nsplit) + 4) * 2.0 ** -53 * np.abs(v).sum(axis=1, keepdims=True)
        assert np.all(np.abs(v) > 1000 * bound), c.name
        cnt = v[:, :, L.S + 1]
        assert np.all(cnt == np.round(cnt)) and np.all(cnt > 0) and np.all(cnt == v[:, :, L.NM:L.NM + g.NS].sum(axis=2))
        if "empty_share" in c.claims:
            assert g.nblk < g.nsplit or any(hi <= lo for lo, hi in JX.shares(g.nblk, g.nsplit))
    assert sum("empty_share" in c.claims for c in JX.all_cases()) >= 12


def test_cases_are_what_their_names_claim():
    conds = []
    for c in JX.all_cases():
        ex = JX.exact(c)
        e, g = ex[0][0], c.groups[0]
        js = g.js[0]
        for cl in c.claims:
            key, val = (cl, None) if isinstance(cl, str) else cl
            if key == "tie":
                assert e.cost == SX.F(float(js["cost_cur"])) and not e.decide, c.name
            elif key == "cost_exact":
                assert e.cost == SX.F(float(e.cost)) and e.cost < SX.F(float(js["cost_cur"])) and np.nextafter(float(e.cost), 2) == js["cost_cur"], c.name
            elif key in ("accept", "reject"):
                assert all(x.decide == (key == "accept") for row in ex for x in row), c.name
            elif key == "lam0":
                assert c.it == 0 and e.lam_out == c.lam0 != js["lam"] and js["have_cur"] == 1 and e.decide, c.name
            elif key == "lam_same":
                assert e.lam_out == js["lam"], c.name
            elif key == "lam_down":
                assert e.lam_out == js["lam"] * c.lam_down > c.lam_min, c.name
            elif key == "lam_floored":
                assert js["lam"] * c.lam_down < c.lam_min == e.lam_out and js["lam"] >= c.lam_min, c.name
            elif key == "stored_differs":
                L = JX.layout(g.NS)
                M = js["M"][:L.NP * L.NC].reshape(L.NP, L.NC)
                H = np.array([[float(x) for x in r] for r in e.H])
                assert np.abs(M[:, :L.NP] - H).max() > 0.1 * np.abs(H).max(), c.name
                n = e.pairs[0]
                assert np.abs(c.state[n]["Tcur"] - c.state[n]["Ttry"]).max() > 1e-3, c.name
            elif key == "bad_pivot":
                assert not e.ok and min(float(e.Hs[i][i]) for i in range(6 * g.NS)) < 0 and all(x == 0 for x in e.d), c.name
            elif key == "zero_step":
                assert e.ok and all(x == 0 for x in e.d), c.name
            elif key == "count0":
                assert e.kn == 0 and e.an == 0, c.name
            elif key == "gn_final":
                assert all(x.final for row in ex for x in row), c.name
            elif key in ("cond", "cond_scaled", "cond_beyond"):
                k = JX.cond_of(c)
                assert val / 3 <= k <= val * 3000, (c.name, k)
                if key == "cond_scaled":
                    H = np.array([[float(x) for x in r] for r in e.Hs])
                    assert all(H[6 * s + 3, 6 * s + 3] / H[6 * s, 6 * s] > 1e3 for s in range(g.NS)), c.name
                if c.judged:
                    conds.append((g.NS, k))
                else:
                    assert k > JX.COND_JUDGED_MAX
            elif key == "steps":
                flat = [x for s in val for x in s]
                assert max(abs(float(a) - b) for a, b in zip(e.d, flat)) < 1e-20, c.name
                t2 = [sum(x * x for x in s[3:]) for s in val]
                assert len({tuple(s) for s in val}) == 4 and any(0 < t < 0.09 for t in t2) and any(t >= 0.09 for t in t2) and any(t == 0 for t in t2), c.name
            elif key == "an_records":
                assert e.an == 1 / e.tot[JX.layout(g.NS).S + 1], c.name
            elif key == "an_norms":
                assert all(x.an == (SX.F(g.c_f) / int(g.norms[JX.norm_group(g, b)][0]) if g.norms[JX.norm_group(g, b)][0] else 0) for b, x in enumerate(ex[0])), c.name
            elif key == "two_groups":
                assert ex[0][0].an == ex[0][1].an != ex[0][2].an == ex[0][3].an, c.name
            elif key == "group_zero":
                assert ex[0][2].an == 0 and ex[0][3].an == 0 and ex[0][0].an > 0, c.name
            elif key == "blockdiag":
                for x in ex[0]:
                    for s in range(g.NS):
                        sl = slice(6 * s, 6 * s + 6)
                        H6 = [row[sl] for row in x.Hs[sl]]
                        assert all(x.Hs[i][j] == 0 for i in range(6 * s, 6 * s + 6) for j in range(6 * g.NS) if j // 6 != s), c.name
                        d6, ok = SX.damped_step(H6, x.gs[sl], x.lam_out)
                        assert ok and d6 == x.dF[sl], c.name
            elif key == "pc":
                assert JX.pc_compiled(c) and c.w_pc > 0
                r = np.abs(e.pc[0].r)
                assert r.min() == 0 and np.any((r > 0) & (r < c.pc_eps)) and r.max() > c.pc_eps, (c.name, r)
            elif key == "layout":
                SB = g.NS * g.B
                assert (g.pc_self0, g.pc_part0) == ((0, SB) if val == "fwd" else (SB, 0)), c.name
            elif key == "coal":
                assert g.B % c.c_B == 0 and g.B == c.c_ncall * c.c_B and c.c_ncall in (2, 3), c.name
            elif key in ("sweep", "split", "empty_share", "repeat", "alone_target", "alone_group"):
                pass
            else:
                raise AssertionError(cl)
    for NS in (1, 2, 3, 4):
        ks = [k for s, k in conds if s == NS]
        assert min(ks) < 100 and max(ks) >= 100 * JX.GOLDEN_JOINT_COND_MAX and max(ks) >= 1e8 and max(ks) <= JX.COND_JUDGED_MAX, (NS, ks)
    pcs = [c for c in JX.all_cases() if "pc" in c.claims]
    for variant in (2, 4):
        assert {(dict(x for x in c.claims if isinstance(x, tuple))["layout"], c.it & 1) for c in pcs if c.variant == variant} == {("fwd", 0), ("fwd", 1), ("inv", 0), ("inv", 1)}
        assert {c.NS for c in pcs if c.variant == variant} == {1, 2, 4}
    # retraction: one step either side of se3_exp's switch, neighbouring doubles
    assert SX.X_LO * SX.X_LO < 0.09 <= SX.X_HI * SX.X_HI and SX.X_HI == np.nextafter(SX.X_LO, 1)
    steps = dict(x for x in JX.by_name()["retract a S4"].claims if isinstance(x, tuple))["steps"]
    assert steps[0][5] == SX.X_LO and steps[1][5] == SX.X_HI


def test_judge_passes_the_clean_standin_under_half_of_the_bar(capsys):
    worst = {}
    for c in JX.all_cases():
        fails, meas = JX.judge_case(c, JX.clean_standin)
        assert not fails, fails[:3]
        if JX.wants_m_export(c):
            assert not JX.check_m_export(c, JX.standin)
        assert not JX.check_alone(c, JX.standin)
        if "repeat" in c.claims:
            assert not JX.check_repeat(c, JX.standin)
        if c.judged:
            w = worst.setdefault(c.group, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], meas["ratio_d"]), max(w[1], meas["ratio_T"]), max(w[2], meas["sum"])
    with capsys.disabled():
        for k, w in worst.items():
            print(f"\n    {k:34s} stand-in: step {w[0]:.3f} of the bar, transform {w[1]:.3f}, sums {w[2]:.3f} of the bound", end="")
    assert max(max(w[0], w[1]) for w in worst.values()) < 0.5, worst
    assert sum(JX.wants_m_export(c) for c in JX.all_cases()) >= 40


FAULTS = {
    "drop_last_of_share": lambda c: ("sweep" in c.claims and c.groups[0].nblk in (2, 33)) or c.name in ("split S2 G3 nblk4 B3", "split S4 G8 nblk481 B1"),
    "first_twice": lambda c: ("sweep" in c.claims and c.groups[0].nblk in (1, 9, 33, 65)) or c.name == "split S1 G2 nblk481 B3",
    "partials_G_minus_1": lambda c: c.name in ("split S1 G2 nblk2 B1", "split S4 G8 nblk1833 B3", "split step S2 G2 nblk481"),
    "fp32_acc": lambda c: "sweep" in c.claims and c.groups[0].nblk >= 100,
    "wrong_norm_group": lambda c: "two_groups" in c.claims or "coal" in c.claims,
    "lam_down_on_reject": lambda c: c.name.startswith("lm reject") or c.name.startswith("lm tie mode0"),
    "no_floor": lambda c: "lam_floored" in c.claims,
    "tie_accept": lambda c: "tie" in c.claims,
    "reject_solves_trial": lambda c: c.name.startswith("lm reject"),
    "no_promote_last_gn": lambda c: c.name.startswith("gn it3"),
    "pc_offdiag": lambda c: "pc" in c.claims and c.NS > 1,
    "pose_lin_same_buffer": lambda c: "pc" in c.claims,
    "partner_own_slot": lambda c: "pc" in c.claims,
    "step_of_source0": lambda c: c.name.startswith("gn it") and c.NS > 1 or c.name.startswith("retract"),
    "damp_no_diag": lambda c: c.name.startswith("lm accept S") or c.name.startswith("lm reject"),
    "coal_call0": lambda c: "coal" in c.claims,
    "jtick_left": lambda c: "split" in c.claims and c.groups[0].nblk in (1, 481),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_judge_fails_every_planted_fault(fault):
    cases = [c for c in JX.all_cases() if FAULTS[fault](c)]
    assert cases
    caught = [c.name for c in cases if JX.judge_case(c, _standin_with(fault))[0]]
    assert caught, f"the judge passed the stand-in with fault {fault!r} on {[c.name for c in cases]}"
    if fault not in ("fp32_acc", "first_twice"):
        assert caught == [c.name for c in cases], (fault, sorted(set(c.name for c in cases) - set(caught)))      # caught on EVERY case that reaches the branch


def test_refusal_cases_break_one_rule_each():
    names = [n for n, _, _ in JX.refusal_cases()]
    assert len(names) == len(set(names)) >= 20
    assert len({w for _, _, w in JX.refusal_cases()}) >= 15


def _golden_joint_conds(oracle64):
    from conftest import load_golden
    from oracle.oracle import default_opts
    worst = {}
    for name in ("winloss24x40", "winloss48x160", "winloss28x48", "winloss4src24x40"):
        g = load_golden(name)
        mind, maxd = (float(x) for x in g["min_max_depth"])
        for argmin in (True, False):
            L = oracle64.linearize_dense_ref(g["target"], g["sources"], g["depth_t"][:, 0], g["depth_s"][:, :, 0], g["K"], g["first"],
                                             default_opts(n_iters=1, w_dc=0.15, irls_eps=1e-7), argmin=argmin, min_depth=mind, max_depth=maxd, lambda_depth=1.0)
            for b, H in enumerate(L["H_joint"]):
                worst[(name, argmin, b)] = float(np.linalg.cond(H))
    return worst


def test_golden_condition_number_is_the_oracles(oracle64):
    """GOLDEN_JOINT_COND_MAX recomputed: the largest cond of the float64 oracle's joint reduced systems (the exported H_joint, depth block
    eliminated at the refinement's lambda_depth = 1) over the four window goldens, with and without the min over the sources"""
    worst = _golden_joint_conds(oracle64)
    top = max(worst.values())
    assert abs(top / JX.GOLDEN_JOINT_COND_MAX - 1) < 1e-3, (top, max(worst, key=worst.get))
