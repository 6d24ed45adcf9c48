"""ONE launch of the joint solve kernels (csrc/joint_kernel.h solve_joint_body: k_solve_joint<NS>, the joint role of k_solve_front<NS, PC>, both
roles of k_solve_joint2<NS, PC>) on records and optimiser state given by the test, against exact arithmetic.  Host only: the cases, the exact
reference, the float64 stand-in (the GPU's place-holder in tests/test_joint_solve_exact_inputs_cpu.py, with switchable planted faults), the
float64 yardstick twins and the judge.  tests/test_gpu_joint_solve_exact.py runs the cases through tcsfm_debug_solve_joint.  Record sums as
Fractions, SE(3) in mpmath, pose / constant rules and the sentinel helpers are tests/solve_exact_inputs.py's (imported, not copied).

The reference models what a launch is documented to do, not its operation order: sum the target's records; apply the normaliser (1 / K from
the records, or c_f / K_f of the target's `norms` group); add the pose-consistency blocks to the diagonal 6 x 6 blocks; decide (Gauss-Newton:
always; LM: a strictly lower cost; `it == 0`: lambda0 and no accepted state); apply the damping schedule; solve (M + lambda diag M + 1e-12 I) d
= -g of the ACCEPTED system (a rejected step: the stored one); T_try = exp(d_s) T_accepted per source; write the constants of the next
linearisation; emit pose and stats row.  Sums, normaliser, costs, system and solution are Fractions of the float bits, transcendentals
mpmath at 80 digits.

The judge (judge_case):
  record sums (export, jpart, the stored system of an accepted step)
        per entry |got - exact| <= (n + 4) 2^-53 a sum|v|: an fp64 sum of n terms in any order has error <= (n - 1) 2^-53 sum|v| to first order,
        the assembly (normaliser a, one product, one more sum) adds at most four roundings of a quantity <= a sum|v| -- the derivation of the
        pose test's bound (tests/solve_exact_inputs.py).  n = nblk unsplit; ceil(nblk / G) + G split (a share's terms, then G partials); a
        partial in jpart: its share's count, a = 1.  Entries that carry a pose-consistency block get, on top, the error an fp64 evaluation of
        that block may make (_pc_terms): the residual r_k = p_k + p'_k of two extracted pose components is off by dr_k <= 4 2^-53 (|p_k| +
        |p'_k|) (atan2 / asin to ~2 ulp each, one sum), hence G_k = w r_k / den_k by w dr_k / den_k and D_k = 2 w / den_k by D_k dr_k / den_k where
        |r_k| is not well below eps (den_k = eps otherwise: exact), each plus 128 2^-53 relative for the roundings of the 6 x 6 inverse Jacobian
        (cosines, sines, one reciprocal, sums of same-signed products) and of the two products; the block's entries are sum_k A_ki D_k A_kj and
        sum_k A_ki G_k, so their bounds are the same sums over absolute values.  Mask counts, shares of empty record ranges, the factor a and
        the ticket are exact.
  step delta_out, trial transforms
        E <= 4 E_env + 8 2^-52 max|exact|, E the max-norm error, E_env the LARGEST error among 16 float64 twins of the same float64 system:
        Cholesky and a division-form unpivoted Gauss-Jordan, each on the identity and on seven fixed random symmetric permutations of the
        unknowns.  (One Cholesky twin is no usable yardstick at 12 to 24 unknowns: an honest float64 Gauss-Jordan in the kernel's order exceeds
        4 E(Cholesky) by up to 2.5 x at condition 1e6.)  Margin 4 as in linearize_exact_inputs.py and solve_exact_inputs.py.
  lambda, have_cur, accept_out, trace_decide, cost_cur on the tie cases, jtick, everything a launch does not own: bit for bit
  constants, poses, stats pose: solve_exact_inputs.judge_const / judge_pose (1 ulp32; 4 x the float32 twin of the extraction + 2^-23)

GOLDEN_JOINT_COND_MAX: the largest condition number of the float64 oracle's joint reduced systems (H_joint of linearize_dense_ref, with and
without the min over the sources) on the goldens winloss24x40, winloss48x160, winloss28x48 and winloss4src24x40; recomputed by
tests/test_joint_solve_exact_inputs_cpu.py.  The judged cases reach at least 100 x it."""
import functools
import math
import types
from fractions import Fraction as F

import mpmath as mpm
import numpy as np

import solve_exact_inputs as SX
from solve_exact_inputs import SENT, NSTAT, STAT_POSE, STATE_DT, CONST_DT, X_LO, X_HI, is_sent, coal_index, const_of, pose_T, pose_f32

GOLDEN_JOINT_COND_MAX = 3.831e3      # winloss4src24x40, target 1, min over the sources (24 unknowns)
COND_JUDGED_MAX = 1e10
JMAXS, SPLIT_MAX = 4, 8
NDELTA, NEXPORT = 6 * JMAXS, 2 + 6 * JMAXS
JS_DT = np.dtype([("lam", "f8"), ("cost_cur", "f8"), ("have_cur", "i4"), ("pad", "i4"), ("M", "f8", 6 * JMAXS * (6 * JMAXS + 1))])


def layout(NS):
    npar = 6 * NS
    nh = npar * (npar + 1) // 2
    return types.SimpleNamespace(NS=NS, NP=npar, NC=npar + 1, NH=nh, G=nh, S=nh + npar, SHARE=nh + npar + 3, NM=nh + npar + 3 + NS, NACC=nh + npar + 3 + 2 * NS)


def tri(r, c):
    hi, lo = max(r, c), min(r, c)
    return hi * (hi + 1) // 2 + lo


def split(NS):
    """(PARTS, NBATCH) of the kernel's record sum: threads = (accumulator column, record subset), NBATCH loads per thread and batch"""
    nacc = layout(NS).NACC
    apad = 32 if nacc <= 32 else (128 if nacc <= 128 else (256 if nacc <= 256 else 512))
    parts = 1024 // apad
    return parts, (16 if parts >= 32 else 32)


def sweep_nblk(NS):
    p, nb = split(NS)
    return sorted({1, 2, p - 1, p, p + 1, nb * p - 1, nb * p, nb * p + 1, 2 * nb * p + 3})


def shares(nblk, G):
    """[(lo, hi)] of the G workgroups' record ranges (empty: lo >= hi)"""
    chunk = (nblk + G - 1) // G
    return [(min(k * chunk, nblk), min(nblk, k * chunk + chunk)) for k in range(G)]


def n_terms(nblk, G):
    return nblk if G <= 1 else (nblk + G - 1) // G + G


# ------------------------------------------------------------------------------------------------------------------------------ records
@functools.lru_cache(maxsize=None)
def make_jrecords(seed, NS, B, nblk, colscale=None, gscale=1.0, count=37.0, blockdiag=False):
    """float32 records [B + 1][nblk][NACC] as solve_exact_inputs.make_records makes them: every record three J' W J / J' W r rows plus a component
    distinct per (target, record, accumulator) and 0.2 on the diagonal, so the totals are SPD and no two entries agree; the slack target is
    NaN.  blockdiag: the off-diagonal 6 x 6 blocks are exactly zero (the min over the sources)"""
    L = layout(NS)
    rng = np.random.default_rng(seed)
    rec = np.full((B + 1, nblk, L.NACC), np.nan, np.float64)
    cs = np.ones(L.NP) if colscale is None else np.tile(np.asarray(colscale, float), NS)
    b_, r_, a_ = np.meshgrid(np.arange(B), np.arange(nblk), np.arange(L.NACC), indexing="ij")
    dist = 0.01 * (1.0 + ((b_ * 389 + r_ * 31 + a_ * 7) % 997) / 997.0)
    J = rng.normal(size=(B, nblk, 3, L.NP)) * cs
    w = rng.uniform(0.5, 1.5, size=(B, nblk, 3))
    res = rng.normal(size=(B, nblk, 3)) * gscale
    Hm = np.einsum("nrk,nrki,nrkj->nrij", w, J, J)
    gv = np.einsum("nrk,nrki,nrk->nri", w, J, res)
    for i in range(L.NP):
        for j in range(i + 1):
            a = tri(i, j)
            if blockdiag and i // 6 != j // 6:
                rec[:B, :, a] = 0.0
            else:
                rec[:B, :, a] = Hm[:, :, i, j] + dist[:, :, a] * cs[i] * cs[j] + (0.2 * cs[i] * cs[j] if i == j else 0.0)
        rec[:B, :, L.G + i] = gv[:, :, i] + dist[:, :, L.G + i] * cs[i] * gscale
    rec[:B, :, L.S] = rng.uniform(1.0, 2.0, size=(B, nblk)) + dist[:, :, L.S]
    rec[:B, :, L.S + 2] = rng.uniform(0.5, 1.0, size=(B, nblk)) + dist[:, :, L.S + 2]
    nm = np.zeros((B, nblk))
    for s in range(NS):
        rec[:B, :, L.SHARE + s] = rng.uniform(0.2, 0.6, size=(B, nblk)) + dist[:, :, L.SHARE + s]
        k = count + (np.arange(B)[:, None] * 5 + np.arange(nblk)[None, :] + 3 * s) % 11          # integer mask counts
        rec[:B, :, L.NM + s] = k
        nm += k
    rec[:B, :, L.S + 1] = nm
    out = rec.astype(np.float32)
    out.setflags(write=False)
    return out


def dyadic_records(NS, hdiag, gvec, count=64.0, nblk=4, cost=1.0):
    """records [2][nblk][NACC] whose totals are H = diag(hdiag), g = gvec, cost and the count exactly in fp64 in ANY order: small integers
    times powers of two, the count a power of two, nblk a power of two; record 0 carries the system, every record a share of the cost"""
    L = layout(NS)
    rec = np.full((2, nblk, L.NACC), np.nan, np.float32)
    rec[0] = 0
    for i in range(L.NP):
        rec[0, 0, tri(i, i)] = hdiag[i] * count
        rec[0, 0, L.G + i] = gvec[i] * count
    rec[0, 0, L.S + 1] = count
    rec[0, 0, L.NM:L.NM + NS] = count / NS if NS in (1, 2, 4) else 0
    rec[0, :, L.S] = cost * count / nblk
    return rec


def spd_records(seed, NS, conds, colscale=None, count=64.0):
    """records whose total is H = sum_k 2^-e_k v_k v_k', g = H x0 with small INTEGER vectors v_k, e_k spread over log2(conds): one rank-one term
    per record, exact in float32 (solve_exact_inputs._spd_records for 6 NS unknowns); colscale: per-source integer scales (translation : rotation)"""
    L = layout(NS)
    npar = L.NP
    rng = np.random.default_rng(seed)
    cs = np.ones(npar) if colscale is None else np.tile(np.asarray(colscale, float), NS)
    V = (npar * np.eye(npar) + rng.integers(-1, 2, size=(npar, npar))) * cs[None, :]      # (diagonal 6 NS: the v_k stay nearly orthogonal at 24 unknowns)
    x0 = rng.integers(-3, 4, size=npar) / (64.0 * cs)
    ex = np.round(np.arange(npar) * math.log2(conds) / (npar - 1))
    if colscale is not None:
        ex = ex[np.argsort(np.argsort(-cs, kind="stable"), kind="stable")]        # (the large unknowns carry the large weights)
    rec = np.full((2, npar, L.NACC), np.nan, np.float32)
    rec[0] = 0
    for k in range(npar):
        Hk = np.outer(V[k], V[k]) * 2.0 ** -ex[k] * count
        gk = Hk @ x0
        for i in range(npar):
            for j in range(i + 1):
                rec[0, k, tri(i, j)] = Hk[i, j]
            rec[0, k, L.G + i] = gk[i]
        assert np.array_equal(rec[0, k, :L.NH].astype(np.float64), np.array([Hk[i, j] for i in range(npar) for j in range(i + 1)]))
    rec[0, :, L.S] = 1.5
    rec[0, 0, L.S + 1] = count
    return rec


def make_js(b_alloc, B, NS, seed, lam=0.0, have_cur=0, cost_cur=0.0):
    """JointState [b_alloc]: a stored SPD system [S | -gS] unlike the records' in its first NP (NP + 1) entries, the sentinel behind them"""
    L = layout(NS)
    js = np.zeros(b_alloc, JS_DT)
    js.view(np.uint8)[:] = SENT
    rng = np.random.default_rng(seed + 500)
    for b in range(B):
        Jm = rng.normal(size=(2 * L.NP, L.NP))
        M = np.zeros((L.NP, L.NC))
        M[:, :L.NP] = Jm.T @ Jm / (2 * L.NP) + 0.1 * np.eye(L.NP)
        M[:, L.NP] = rng.normal(size=L.NP) * 0.05
        js[b]["M"][:L.NP * L.NC] = M.reshape(-1)
        js[b]["lam"], js[b]["cost_cur"], js[b]["have_cur"], js[b]["pad"] = lam, cost_cur, have_cur, 0
    return js


def group(NS, B, rec, *, nsplit=1, seed=0, lam=0.0, have_cur=0, cost_cur=0.0, norms=None, norm_B=0, c_f=1.0, export=False, want_part=True):
    rec = np.asarray(rec)
    assert rec.shape[0] == B + 1 and rec.shape[2] == layout(NS).NACC
    return types.SimpleNamespace(NS=NS, B=B, b_alloc=B + 1, nblk=rec.shape[1], nsplit=nsplit, n0=0, rec=rec, js=make_js(B + 1, B, NS, seed, lam, have_cur, cost_cur),
                                 norms=None if norms is None else np.asarray(norms, np.int32), norm_B=norm_B, c_f=float(c_f), pc_self0=0, pc_part0=0,
                                 export=export, want_part=want_part, tick_in=0)


ALL_OUT = ("stats", "pose_out", "trace_decide")


def case(name, grp, groups, *, variant=0, solver=0, n_iters=4, lam0=1e-4, lam_up=10.0, lam_down=0.1, lam_min=1e-5, mode=0, it=0, seed=0, judged=True, claims=(),
         want=ALL_OUT, w_pc=0.0, pc_eps=1e-3, pose_lin=None, c_ncall=0, c_B=0, c_S=0, c_len=()):
    f32 = lambda x: float(np.float32(x))
    c = types.SimpleNamespace(name=name, group=grp, groups=list(groups), variant=variant, NS=groups[0].NS, solver=solver, n_iters=n_iters, lam0=f32(lam0), lam_up=f32(lam_up),
                              lam_down=f32(lam_down), lam_min=f32(lam_min), mode=mode, it=it, judged=judged, claims=tuple(claims), want=tuple(want), w_pc=float(w_pc),
                              pc_eps=float(pc_eps), pose_lin=pose_lin, pc_np=0 if pose_lin is None else pose_lin.shape[1], c_ncall=c_ncall, c_B=c_B, c_S=c_S,
                              c_len=tuple(c_len))
    n = 0
    for g in c.groups:
        g.n0 = n
        n += g.NS * g.B
    c.npairs, c.n_alloc = n, n + 1
    c.state = SX.make_state(c.n_alloc, n, seed)
    c.pconst = SX.make_const(c.n_alloc, n)
    return c


def clone(c, **kw):
    d = types.SimpleNamespace(**vars(c))
    d.state, d.pconst = c.state.copy(), c.pconst.copy()
    d.pose_lin = None if c.pose_lin is None else c.pose_lin.copy()
    d.groups = []
    for g in c.groups:
        h = types.SimpleNamespace(**vars(g))
        h.js = g.js.copy()
        d.groups.append(h)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def pc_compiled(c):
    return c.variant in (2, 4)


def alone(c, gi, b=None):
    """group gi of case c (or its target b only) as a launch of its own through variant 0 with the same nsplit"""
    g = c.groups[gi]
    h = types.SimpleNamespace(**vars(g))
    idx = [s * g.B + x for s in range(g.NS) for x in (range(g.B) if b is None else [b])]
    if b is not None:
        h.B, h.b_alloc = 1, 2
        h.rec = np.concatenate([g.rec[b:b + 1], g.rec[g.B:g.B + 1]])
        h.js = np.concatenate([g.js[b:b + 1], g.js[g.B:g.B + 1]])
        h.norms, h.norm_B = (None, 0) if g.norms is None else (g.norms[(b // g.norm_B if g.norm_B > 0 else 0):][:1].copy(), 0)
    else:
        h.js = g.js.copy()
    h.n0 = 0
    d = clone(c, name=c.name + f"/alone{gi}" + ("" if b is None else f".{b}"), variant=0, w_pc=0.0, pose_lin=None, pc_np=0)
    d.groups = [h]
    d.NS = h.NS
    d.npairs, d.n_alloc = len(idx), len(idx) + 1
    sel = [g.n0 + i for i in idx] + [c.n_alloc - 1]
    d.state, d.pconst = c.state[sel].copy(), c.pconst[sel].copy()
    return d


def new_outputs(c):
    """the arrays of a launch before it: inputs where the kernel updates in place, the sentinel everywhere else"""
    def sent(shape, dt):
        a = np.zeros(shape, dt)
        a.view(np.uint8)[:] = SENT
        return a
    o = dict(state=c.state.copy(), pconst=c.pconst.copy(), pose_lin=None if c.pose_lin is None else c.pose_lin.copy())
    shapes = dict(stats=((c.n_alloc, c.n_iters + 1, NSTAT), np.float32), pose_out=((c.n_alloc, 6), np.float32), trace_decide=((c.n_alloc,), np.int32))
    for k, (shape, dt) in shapes.items():
        o[k] = sent(shape, dt) if k in c.want else None
    o["c_pose_out"] = [sent((c.c_len[i], 6), np.float32) for i in range(c.c_ncall)]
    o["g"] = []
    for g in c.groups:
        L = layout(g.NS)
        q = dict(js=g.js.copy(), delta_out=sent((g.b_alloc, NDELTA), np.float64), accept_out=sent((g.b_alloc,), np.int32),
                 export_out=sent((g.b_alloc, NEXPORT), np.float64) if g.export else None, jpart=None, jtick=None)
        if g.nsplit > 1 or g.want_part:
            q["jpart"] = sent((g.b_alloc, g.nsplit, L.NACC), np.float64)
            q["jtick"] = sent((g.b_alloc,), np.int32)
            if g.nsplit > 1:
                q["jtick"][:g.B] = g.tick_in
        o["g"].append(q)
    return o


# ------------------------------------------------------------------------------------------------------------------- exact reference
def exact_sums(g, b, lo=0, hi=None):
    """(exact sums of records lo .. hi - 1 of target b per accumulator as Fractions, sum|v| per accumulator as floats).  Per column the float32
    values are integers times 2^emin (emin: the lowest bit any of them has); where their int64 sum cannot overflow it is taken in numpy,
    otherwise in Python integers (solve_exact_inputs.exact_sum)"""
    hi = g.nblk if hi is None else hi
    v = g.rec[b, lo:hi].astype(np.float64)
    n = v.shape[0]
    _, e = np.frexp(v)
    emin = np.where(v != 0, e - 24, 10 ** 6).min(axis=0) if n else np.zeros(v.shape[1], int)
    emin = np.where(emin == 10 ** 6, 0, emin)
    sc = np.ldexp(v, -emin[None, :])
    ok = np.abs(sc).max(axis=0) * max(n, 1) < 2.0 ** 62 if n else np.ones(v.shape[1], bool)
    tot = np.where(ok[None, :], sc, 0).astype(np.int64).sum(axis=0)
    out = [F(int(tot[a])) * F(2) ** int(emin[a]) if ok[a] else SX.exact_sum(g.rec[b, lo:hi, a]) for a in range(v.shape[1])]
    return out, np.abs(v).sum(axis=0)


def norm_group(g, b):
    return b // g.norm_B if g.norm_B > 0 else 0


def _frac(x):
    """an mpf as a Fraction to 2^-160 (reference error 7e-49: far below any bound here; short denominators keep the exact solves quick)"""
    return x if isinstance(x, F) else F(int(mpm.floor(mpm.ldexp(x, 160) + 0.5)), 2 ** 160)


def _pc_terms(c, g, b):
    """exact pose-consistency terms of target b: per source H6 [6][6], g6 [6], cost (Fractions), the residual, and the absolute error an fp64
    evaluation may make in each (floats bH, bg, bcost; derivation: module docstring)"""
    out = []
    w, eps = mpm.mpf(c.w_pc), mpm.mpf(c.pc_eps)
    u = 2.0 ** -53
    for s in range(g.NS):
        n = s * g.B + b
        Tm = [mpm.mpf(float(x)) for x in c.state[g.n0 + n]["Ttry"]]
        Tp = [mpm.mpf(float(x)) for x in c.pose_lin[c.it & 1][g.pc_part0 + n]]
        pm, pp = SX.mp_pose_of_T(Tm), SX.mp_pose_of_T(Tp)
        Ai = mpm.inverse(SX.euler_left_jacobian(pm))
        r = [x + y for x, y in zip(pm, pp)]
        den = [max(abs(x), eps) for x in r]
        G, D = [w * x / d for x, d in zip(r, den)], [2 * w / d for d in den]
        H6 = [[_frac(sum(Ai[k, i] * D[k] * Ai[k, j] for k in range(6))) for j in range(6)] for i in range(6)]
        g6 = [_frac(sum(Ai[k, i] * G[k] for k in range(6))) for i in range(6)]
        Aa = np.array([[abs(float(Ai[k, i])) for i in range(6)] for k in range(6)])
        rf, df, Gf, Df = (np.array([float(x) for x in v]) for v in (r, den, G, D))
        dr = 4 * u * np.array([abs(float(a)) + abs(float(b_)) for a, b_ in zip(pm, pp)])
        dG = float(w) * dr / df + 128 * u * np.abs(Gf)
        dD = np.where(np.abs(rf) >= 0.5 * float(eps), Df * dr / df, 0.0) + 128 * u * Df
        out.append(types.SimpleNamespace(H=H6, g=g6, cost=_frac(sum(w * abs(x) / 2 for x in r)), r=[float(x) for x in r], bH=Aa.T @ np.diag(dD) @ Aa, bg=Aa.T @ dG,
                                         bcost=float(0.5 * float(w) * dr.sum() + 16 * u * float(sum(w * abs(x) / 2 for x in r)))))
    return out


PC_SLACK = 1.0


def exact_target(c, gi, b):
    g = c.groups[gi]
    L = layout(g.NS)
    npar = L.NP
    tot, sab = exact_sums(g, b)
    e = types.SimpleNamespace(tot=tot, sab=sab)
    kn = tot[L.S + 1]
    an = 1 / kn if kn > 0 else F(0)
    if g.norms is not None:
        kn = F(int(g.norms[norm_group(g, b)][0]))
        an = F(g.c_f) / kn if kn > 0 else F(0)
    e.an, e.kn = an, kn
    fan = float(an)
    u = (n_terms(g.nblk, g.nsplit) + 4) * 2.0 ** -53
    e.u = u
    H = [[an * tot[tri(i, j)] for j in range(npar)] for i in range(npar)]
    gv = [an * tot[L.G + i] for i in range(npar)]
    e.bH = u * fan * np.array([[sab[tri(i, j)] for j in range(npar)] for i in range(npar)])
    e.bg = u * fan * np.array([sab[L.G + i] for i in range(npar)])
    e.gexp, e.bgexp = list(gv), e.bg.copy()
    e.cost, e.bcost = an * tot[L.S], u * fan * sab[L.S]
    e.share = [an * tot[L.SHARE + s] for s in range(g.NS)]
    e.nm = [tot[L.NM + s] for s in range(g.NS)]
    e.pc = None
    if pc_compiled(c):
        e.pc = _pc_terms(c, g, b)
        for s, p in enumerate(e.pc):
            e.cost += p.cost
            e.bcost += PC_SLACK * p.bcost
            for i in range(6):
                gv[6 * s + i] += p.g[i]
                e.bg[6 * s + i] += PC_SLACK * p.bg[i]
                for j in range(6):
                    H[6 * s + i][6 * s + j] += p.H[i][j]
                    e.bH[6 * s + i, 6 * s + j] += PC_SLACK * p.bH[i, j]
    e.H, e.g = H, gv
    if g.export:
        return e
    js = g.js[b]
    first = c.it == 0 and c.mode == 0
    lam = c.lam0 if first else float(js["lam"])
    have = 0 if first else int(js["have_cur"])
    cost_cur = float(js["cost_cur"])
    e.lam_in, e.final = lam, False
    pairs = [g.n0 + s * g.B + b for s in range(g.NS)]
    e.pairs = pairs
    if c.mode == 1:
        e.decide = e.cost < F(cost_cur)
        e.Tfin = [[mpm.mpf(float(x)) for x in (c.state[n]["Ttry"] if e.decide else c.state[n]["Tcur"])] for n in pairs]
        e.final = True
        return e
    e.decide = c.solver == 0 or not have or e.cost < F(cost_cur)
    if e.decide:
        if c.solver == 1 and have:
            lam = max(lam * c.lam_down, c.lam_min)
        Hs, gs = H, gv
    else:
        lam = lam * c.lam_up
        M = js["M"][:npar * L.NC].reshape(npar, L.NC)
        Hs = [[F(float(M[i, j])) for j in range(npar)] for i in range(npar)]
        gs = [-F(float(M[i, npar])) for i in range(npar)]
    e.lam_out, e.Hs, e.gs = lam, Hs, gs
    d, e.ok = SX.damped_step(Hs, gs, lam)
    e.dF = d
    e.d = [SX.mpf(x) for x in d]
    e.Tacc = [[mpm.mpf(float(x)) for x in (c.state[n]["Ttry"] if e.decide else c.state[n]["Tcur"])] for n in pairs]
    e.Tnew = [SX.mp_mul(SX.mp_se3_exp(e.d[6 * s:6 * s + 6]), e.Tacc[s]) for s in range(g.NS)]
    if c.solver == 0 and c.it == c.n_iters - 1:
        e.final, e.Tfin = True, e.Tnew
    return e


_EXACT = {}


def exact(c):
    if c.name not in _EXACT:
        _EXACT[c.name] = [[exact_target(c, gi, b) for b in range(g.B)] for gi, g in enumerate(c.groups)]
    return _EXACT[c.name]


# ------------------------------------------------------------------------------------------------------------ float64 stand-in, twins
def _gj_kernel_order(A):
    """unpivoted Gauss-Jordan on [A | b] as the kernel eliminates: every row r != k at once, M[r][c] - M[r][k] (1 / piv) M[k][c] -> (d, ok)"""
    M = A.copy()
    n = M.shape[0]
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = M[k, k]
            if not piv > 0.0:
                ok = False
            f = M[:, k] * (1.0 / piv)
            upd = M - np.outer(f, M[k])
            upd[k] = M[k]
            M = upd
        d = M[:, n] / np.diag(M[:, :n])
    return (d, True) if ok else (np.zeros(n), False)


def _gj_division(A):
    M = A.copy()
    n = M.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n):
            f = M[:, k] / M[k, k]
            f[k] = 0.0
            M = M - np.outer(f, M[k])
        return M[:, n] / np.diag(M[:, :n])


def _chol(A):
    n = A.shape[0]
    try:
        Lc = np.linalg.cholesky(A[:, :n])
    except np.linalg.LinAlgError:
        return np.zeros(n)
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, A[:, n]))


@functools.lru_cache(maxsize=None)
def _perms(n):
    rng = np.random.default_rng(20240 + n)
    return [np.arange(n)] + [rng.permutation(n) for _ in range(7)]


def twin_steps(A):
    """the 16 yardstick solutions of the damped float64 system [A | b]: Cholesky and division-form Gauss-Jordan x 8 symmetric permutations"""
    n = A.shape[0]
    out = []
    for p in _perms(n):
        Ap = np.concatenate([A[p][:, p], A[p][:, n:]], axis=1)
        for solver in (_chol, _gj_division):
            d = np.zeros(n)
            with np.errstate(all="ignore"):
                d[p] = solver(Ap)
            out.append(d)
    return out


def _pc64(c, g, b, fault):
    out = []
    for s in range(g.NS):
        n = s * g.B + b
        slot = (g.pc_self0 if fault == "partner_own_slot" else g.pc_part0) + n
        pm, pp = SX.pose64(c.state[g.n0 + n]["Ttry"]), SX.pose64(c.pose_lin[c.it & 1][slot])
        Ai = np.linalg.inv(SX.jac64(pm))
        r = pm + pp
        den = np.maximum(np.abs(r), c.pc_eps)
        out.append((Ai.T @ np.diag(2 * c.w_pc / den) @ Ai, Ai.T @ (c.w_pc * r / den), float(np.sum(0.5 * c.w_pc * np.abs(r)))))
    return out


def standin(c, fault=None, keep=None):
    """the launch in numpy float64, a transcription of the documented steps with the kernel's split sum and Gauss-Jordan order -> outputs as
    new_outputs(); fault: a planted fault; keep: dict that receives the damped systems solved, per (group, target)"""
    o = new_outputs(c)
    for gi, g in enumerate(c.groups):
        L = layout(g.NS)
        npar, NC = L.NP, L.NC
        q = o["g"][gi]
        parts = split(g.NS)[0]
        G = g.nsplit
        for b in range(g.B):
            rows = g.rec[b].astype(np.float32 if fault == "fp32_acc" else np.float64)
            ptl = []
            for lo, hi in shares(g.nblk, G):
                blk = rows[lo:hi]
                if fault == "drop_last_of_share" and hi > lo:
                    blk = blk[:-1]
                t = blk.sum(axis=0, dtype=rows.dtype).astype(np.float64) if len(blk) else np.zeros(L.NACC)
                if fault == "first_twice" and hi > lo and (hi - lo) % parts != 0:
                    t = t + rows[lo].astype(np.float64)
                ptl.append(t)
            tot = np.zeros(L.NACC)
            for k in range(G - 1 if (fault == "partials_G_minus_1" and G > 1) else G):
                tot = tot + ptl[k]
            if G > 1:
                q["jpart"][b] = np.stack(ptl)
                q["jtick"][b] = G if fault == "jtick_left" else 0
            kn = tot[L.S + 1]
            an = 1.0 / kn if kn > 0 else 0.0
            if g.norms is not None:
                grp = norm_group(g, b)
                if fault == "wrong_norm_group" and g.norms.shape[0] > 1:
                    grp = (grp + 1) % g.norms.shape[0]
                kn = float(g.norms[grp][0])
                an = g.c_f / kn if kn > 0 else 0.0
            cost = an * tot[L.S]
            pcs = _pc64(c, g, b, fault) if pc_compiled(c) else None
            if pcs:
                cost += sum(p[2] for p in pcs)
            if g.export:
                q["export_out"][b, 0], q["export_out"][b, 1] = cost, an
                q["export_out"][b, 2:2 + npar] = an * tot[L.G:L.G + npar]
                continue
            js, jo = g.js[b], q["js"][b]
            first = c.it == 0 and c.mode == 0
            lam = c.lam0 if first else float(js["lam"])
            have = 0 if first else int(js["have_cur"])
            pairs = [g.n0 + s * g.B + b for s in range(g.NS)]
            for s, n in enumerate(pairs):
                if o["stats"] is not None:
                    o["stats"][n, c.it, :4] = np.array([cost, an * tot[L.SHARE + s], tot[L.NM + s], lam]).astype(np.float32)
                    o["stats"][n, c.it, STAT_POSE:] = pose_f32(c.state[n]["Ttry"])
            lower = cost <= js["cost_cur"] if fault == "tie_accept" else cost < js["cost_cur"]
            if c.mode == 1:
                q["accept_out"][b] = int(lower)
                for n in pairs:
                    if o["trace_decide"] is not None:
                        o["trace_decide"][n] = int(lower)
                    if lower:
                        o["state"][n]["Tcur"] = c.state[n]["Ttry"]
                    if o["pose_out"] is not None:
                        o["pose_out"][n] = pose_f32(c.state[n]["Ttry"] if lower else c.state[n]["Tcur"])
                continue
            accept = bool(c.solver == 0 or not have or lower)
            if accept and c.solver == 1 and have:
                lam = lam * c.lam_down if fault == "no_floor" else max(lam * c.lam_down, c.lam_min)
            if not accept:
                lam = max(lam * c.lam_down, c.lam_min) if fault == "lam_down_on_reject" else lam * c.lam_up
            M = np.zeros((npar, NC))
            for i in range(npar):
                for j in range(npar):
                    M[i, j] = an * tot[tri(i, j)]
                M[i, npar] = -an * tot[L.G + i]
            if pcs:
                for s, p in enumerate(pcs):
                    t = (s + 1) % g.NS if (fault == "pc_offdiag" and g.NS > 1) else s
                    M[6 * s:6 * s + 6, 6 * t:6 * t + 6] += p[0]
                    M[6 * s:6 * s + 6, npar] -= p[1]
            if accept:
                jo["M"][:npar * NC] = M.reshape(-1)
            elif fault != "reject_solves_trial":
                M = js["M"][:npar * NC].reshape(npar, NC).copy()
            A = M.copy()
            dg = np.diag(M[:, :npar]).copy()
            A[np.arange(npar), np.arange(npar)] += (lam if fault == "damp_no_diag" else lam * dg) + 1e-12
            if keep is not None:
                keep[(gi, b)] = A.copy()
            d, ok = _gj_kernel_order(A)
            jo["lam"] = lam
            if accept:
                jo["cost_cur"], jo["have_cur"] = cost, 1
            q["accept_out"][b] = int(accept)
            q["delta_out"][b, :npar] = d
            last_gn = c.solver == 0 and c.it == c.n_iters - 1
            for s, n in enumerate(pairs):
                S = c.state[n]
                so = o["state"][n]
                Tacc = S["Ttry"] if accept else S["Tcur"]
                if accept:
                    so["Tcur"] = Tacc
                if o["trace_decide"] is not None:
                    o["trace_decide"][n] = int(accept)
                ds = d[0:6] if fault == "step_of_source0" else d[6 * s:6 * s + 6]
                Tnew = SX.mul64(SX.exp64(ds).reshape(12), Tacc)
                so["Ttry"] = Tnew
                if last_gn and fault != "no_promote_last_gn":
                    so["Tcur"] = Tnew
                if pcs is not None:
                    half = (c.it & 1) if fault == "pose_lin_same_buffer" else ((c.it + 1) & 1)
                    o["pose_lin"][half][g.pc_self0 + (n - g.n0)] = Tnew
                k = const_of(S["K"], Tnew, 0.0, 6)
                pc = o["pconst"][n]
                pc["A"], pc["kt"], pc["R"], pc["t"] = k["A"], k["kt"], k["R"], k["t"]
                if last_gn and o["pose_out"] is not None:
                    pose = pose_f32(Tnew)
                    if c.c_ncall > 0:
                        call, li = coal_index(c.c_ncall, c.c_B, c.c_S, n - g.n0)
                        o["c_pose_out"][0 if fault == "coal_call0" else call][li] = pose
                    else:
                        o["pose_out"][n] = pose
                    if o["stats"] is not None:
                        o["stats"][n, c.n_iters, STAT_POSE:] = pose
    return o


_CLEAN, _ENV = {}, {}


def clean_standin(c):
    if c.name not in _CLEAN:
        keep = {}
        _CLEAN[c.name] = (standin(c, keep=keep), keep)
    return _CLEAN[c.name][0]


def envelope(c, gi, b):
    """(E_env of the step, E_env of the trial transforms): the largest error among the 16 float64 twins"""
    key = (c.name, gi, b)
    if key not in _ENV:
        clean_standin(c)
        A = _CLEAN[c.name][1][(gi, b)]
        e = exact(c)[gi][b]
        g = c.groups[gi]
        Ed = ET = 0.0
        for d in twin_steps(A):
            if not e.ok:
                d = np.zeros_like(d)
            Ed = max(Ed, SX.Emax(d, e.d))
            for s in range(g.NS):
                Tacc = np.array([float(x) for x in e.Tacc[s]])
                ET = max(ET, SX.Emax(SX.mul64(SX.exp64(d[6 * s:6 * s + 6]).reshape(12), Tacc), e.Tnew[s]))
        _ENV[key] = (Ed, ET)
    return _ENV[key]


# ---------------------------------------------------------------------------------------------------------------------------- judge
_eq = SX.eq


def cond_of(c, gi=0, b=0):
    """condition number of the damped system the launch solves"""
    e = exact(c)[gi][b]
    H = np.array([[float(x) for x in row] for row in e.Hs])
    return float(np.linalg.cond(H + np.diag(e.lam_out * np.diag(H) + 1e-12)))


def _within(bad, meas, t, got, exv, bnd, what):
    """got [k] floats against exact Fractions with per-entry bounds -> worst error in units of its bound"""
    for i, (a, x, bb) in enumerate(zip(np.asarray(got, np.float64).reshape(-1), exv, np.asarray(bnd, np.float64).reshape(-1))):
        err = abs(F(float(a)) - x) if np.isfinite(a) else math.inf
        if bb > 0 and err != math.inf:
            meas["sum"] = max(meas["sum"], float(err) / bb)
        if not err <= bb:
            bad(t + f"{what}[{i}] off by {float(err):.3e}, bound {bb:.3e}")
            return


def judge_case(c, run, tag=None):
    """-> (failures, measures): run(case) -> outputs of the launch (the GPU, or the stand-in with a fault)"""
    tag = tag or c.name
    out, ex = run(c), exact(c)
    fails, meas = [], dict(ratio_d=0.0, E_d=0.0, ratio_T=0.0, E_T=0.0, sum=0.0, pose=0.0, const=0.0)
    bad = lambda msg: fails.append(f"{tag}: {msg}")
    shim = types.SimpleNamespace(np=6)
    N = c.npairs
    if not is_sent(out["state"][N:]) or not is_sent(out["pconst"][N:]):
        bad("state / pconst of a pair beyond the launch's written")
    for k in ALL_OUT:
        if out[k] is not None and not is_sent(out[k][N:]):
            bad(f"{k} of a pair beyond the launch's written")
    wrote_lin = set()
    want_coal = {}
    for gi, g in enumerate(c.groups):
        L = layout(g.NS)
        npar, NC = L.NP, L.NC
        q = out["g"][gi]
        for k in ("js", "delta_out", "accept_out", "export_out", "jpart", "jtick"):
            if q[k] is not None and not is_sent(q[k][g.B:]):
                bad(f"group {gi}: {k} of a target beyond B written")
        if g.nsplit == 1 and q["jpart"] is not None and not (is_sent(q["jpart"]) and is_sent(q["jtick"])):
            bad(f"group {gi}: nsplit 1 wrote jpart / jtick")
        for b in range(g.B):
            e = ex[gi][b]
            t = f"group {gi} target {b}: "
            js, jo = g.js[b], q["js"][b]
            if g.nsplit > 1:
                if int(q["jtick"][b]) != 0:
                    bad(t + f"jtick is {int(q['jtick'][b])} after the launch, not 0")
                for k, (lo, hi) in enumerate(shares(g.nblk, g.nsplit)):
                    if hi <= lo:
                        if np.any(q["jpart"][b, k] != 0):
                            bad(t + f"empty share {k}: partial not exactly zero")
                        continue
                    ps, pab = exact_sums(g, b, lo, hi)
                    _within(bad, meas, t, q["jpart"][b, k], ps, (hi - lo + 4) * 2.0 ** -53 * pab, f"jpart[{k}]")
            if not is_sent(jo["M"][npar * NC:]):
                bad(t + "js.M beyond NP (NP + 1) written")
            if not is_sent(q["delta_out"][b, npar:]):
                bad(t + "delta_out beyond NP written")
            pairs = [g.n0 + s * g.B + b for s in range(g.NS)]
            if g.export:
                xo = q["export_out"][b]
                _within(bad, meas, t, xo[0:1], [e.cost], [e.bcost], "export cost")
                if F(float(xo[1])) != F(float(e.an)) and not (e.an == 0 and xo[1] == 0):
                    bad(t + f"export factor {xo[1]!r} is not {float(e.an)!r}")
                _within(bad, meas, t, xo[2:2 + npar], e.gexp, e.bgexp, "export g")
                if not is_sent(xo[2 + npar:]):
                    bad(t + "export_out beyond 2 + NP written")
                if not _eq(jo, js) or not is_sent(q["delta_out"][b]) or not is_sent(q["accept_out"][b]):
                    bad(t + "the export path wrote js / delta_out / accept_out")
                for n in pairs:
                    if not _eq(out["state"][n], c.state[n]) or not _eq(out["pconst"][n], c.pconst[n]):
                        bad(t + "the export path wrote state / pconst")
                    for k in ALL_OUT:
                        if out[k] is not None and not is_sent(out[k][n]):
                            bad(t + f"the export path wrote {k}")
                continue
            if int(q["accept_out"][b]) != int(e.decide):
                bad(t + f"accept_out = {int(q['accept_out'][b])}, exact decision {int(e.decide)}")
            for s, n in enumerate(pairs):
                S, so = c.state[n], out["state"][n]
                tp = t + f"source {s}: "
                if out["trace_decide"] is not None and int(out["trace_decide"][n]) != int(e.decide):
                    bad(tp + "trace_decide")
                st_rows = out["stats"][n] if out["stats"] is not None else None
                if st_rows is not None:
                    for i in range(c.n_iters + 1):
                        if i == c.it:
                            continue
                        if i == c.n_iters and c.mode == 0 and e.final and out["pose_out"] is not None:
                            if not is_sent(st_rows[i, :STAT_POSE]):
                                bad(tp + "cost fields of the final stats row written")
                        elif not is_sent(st_rows[i]):
                            bad(tp + f"stats row {i} written by launch {c.it}")
                    SX.judge_pose(bad, meas, tp + "stats pose", st_rows[c.it, STAT_POSE:], SX.mp_pose_of_T([mpm.mpf(float(x)) for x in S["Ttry"]]), pose_f32(S["Ttry"]))
                    if st_rows[c.it, 2] != np.float32(float(e.nm[s])) or st_rows[c.it, 3] != np.float32(e.lam_in):
                        bad(tp + "stats n_mask / lambda")
                    if abs(float(st_rows[c.it, 0]) - float(e.cost)) > 2.0 ** -23 * max(1.0, abs(float(e.cost))):
                        bad(tp + "stats cost")
                    if abs(float(st_rows[c.it, 1]) - float(e.share[s])) > 2.0 ** -23 * max(1.0, abs(float(e.share[s]))):
                        bad(tp + "stats share")
                for k in ("scur", "stry", "s0", "lam", "cost_cur", "M8", "K", "have_cur", "pad"):
                    if not _eq(so[k], S[k]):
                        bad(tp + f"PairState.{k} changed")
            if c.mode == 1:
                if not _eq(jo, js) or not is_sent(q["delta_out"][b]):
                    bad(t + "mode 1 wrote js / delta_out")
                for s, n in enumerate(pairs):
                    S, so = c.state[n], out["state"][n]
                    if not _eq(so["Ttry"], S["Ttry"]) or not _eq(so["Tcur"], S["Ttry"] if e.decide else S["Tcur"]):
                        bad(t + f"source {s}: mode 1: Ttry changed or Tcur is not the kept transform")
                    if not _eq(out["pconst"][n], c.pconst[n]):
                        bad(t + f"source {s}: mode 1 wrote pconst")
                    if out["pose_out"] is not None:
                        SX.judge_pose(bad, meas, t + f"source {s}: pose_out", out["pose_out"][n], SX.mp_pose_of_T(e.Tfin[s]), pose_f32(S["Ttry"] if e.decide else S["Tcur"]))
                continue
            acc = e.decide
            last_gn = c.solver == 0 and c.it == c.n_iters - 1
            if jo["lam"] != e.lam_out or math.copysign(1, jo["lam"]) != math.copysign(1, e.lam_out):
                bad(t + f"lambda {jo['lam']!r} is not {e.lam_out!r}")
            if jo["have_cur"] != (1 if acc else js["have_cur"]) or jo["pad"] != js["pad"]:
                bad(t + "have_cur / pad")
            Mo = jo["M"][:npar * NC].reshape(npar, NC)
            if acc:
                _within(bad, meas, t, Mo[:, :npar], [x for row in e.H for x in row], e.bH, "js.M")
                _within(bad, meas, t, -Mo[:, npar], e.g, e.bg, "js.M rhs")
                if "tie_exact" in c.claims or "cost_exact" in c.claims:
                    if F(float(jo["cost_cur"])) != e.cost:
                        bad(t + f"cost_cur {jo['cost_cur']!r} is not the exactly representable cost {float(e.cost)!r}")
                else:
                    _within(bad, meas, t, [jo["cost_cur"]], [e.cost], [e.bcost + 2.0 ** -52 * abs(float(e.cost))], "cost_cur")
            else:
                for k in ("M", "cost_cur"):
                    if not _eq(jo[k], js[k]):
                        bad(t + f"rejected, but js.{k} changed")
            dgot = q["delta_out"][b, :npar]
            if not e.ok and np.any(dgot != 0):
                bad(t + "a non-positive pivot must give a zero step")
            Eenv_d, Eenv_T = envelope(c, gi, b)
            Ek = SX.Emax(dgot, e.d)
            floor = 8 * 2.0 ** -52 * max(float(abs(x)) for x in e.d)
            bar = 4 * Eenv_d + floor
            meas["ratio_d"], meas["E_d"] = max(meas["ratio_d"], Ek / bar if bar > 0 else (0.0 if Ek == 0 else math.inf)), max(meas["E_d"], Ek)
            if c.judged and not Ek <= bar:
                bad(t + f"step: E {Ek:.3e} > 4 x {Eenv_d:.3e} + {floor:.3e} (condition {cond_of(c, gi, b):.2e})")
            for s, n in enumerate(pairs):
                S, so = c.state[n], out["state"][n]
                tp = t + f"source {s}: "
                Tin = S["Ttry"] if acc else S["Tcur"]
                if not last_gn and not _eq(so["Tcur"], Tin):
                    bad(tp + "Tcur is not the accepted transform")
                if last_gn and not _eq(so["Tcur"], so["Ttry"]):
                    bad(tp + "last Gauss-Newton launch: Tcur is not the new iterate")
                Ek = SX.Emax(so["Ttry"], e.Tnew[s])
                floor = 8 * 2.0 ** -52 * max(float(abs(x)) for x in e.Tnew[s])
                bar = 4 * Eenv_T + floor
                meas["ratio_T"], meas["E_T"] = max(meas["ratio_T"], Ek / bar), max(meas["E_T"], Ek)
                if c.judged and not Ek <= bar:
                    bad(tp + f"trial transform: E {Ek:.3e} > 4 x {Eenv_T:.3e} + {floor:.3e} (condition {cond_of(c, gi, b):.2e})")
                if all(x == 0 for x in e.d[6 * s:6 * s + 6]) and not _eq(so["Ttry"], Tin):
                    bad(tp + "zero step, but the trial transform is not the accepted one")
                # the constants are float32 roundings of K-weighted sums of the transform's entries (|K| <= 64): against the EXACT transform while
                # the error the transform is allowed (the bar) is below 2^-40 -- 64 x 2^-40 is under an fp32 ulp of any constant above 1e-3 --
                # else (the ill-conditioned systems) against the transform that was written
                fine = c.judged and bar <= 2.0 ** -40
                Tc = [SX.frac(x) for x in e.Tnew[s]] if fine else [F(float(x)) for x in so["Ttry"]]
                SX.judge_const(bad, meas, tp, shim, out["pconst"][n], c.pconst[n], S["K"], Tc, mpm.mpf(0))
                if pc_compiled(c):
                    me = g.pc_self0 + (n - g.n0)
                    wrote_lin.add(me)
                    if not _eq(out["pose_lin"][(c.it + 1) & 1][me], so["Ttry"]):
                        bad(tp + "pose_lin's next buffer is not the new trial transform")
                if out["pose_out"] is not None:
                    if c.c_ncall > 0:
                        call, li = coal_index(c.c_ncall, c.c_B, c.c_S, n - g.n0)
                        slot = out["c_pose_out"][call][li]
                        if e.final:
                            want_coal[(call, li)] = n
                    else:
                        slot = out["pose_out"][n]
                    if not e.final:
                        if c.c_ncall == 0 and not is_sent(slot):
                            bad(tp + "pose_out written by a launch that is not the last")
                    else:
                        SX.judge_pose(bad, meas, tp + "pose_out", slot, SX.mp_pose_of_T(e.Tfin[s]), pose_f32(so["Ttry"]))
                        if out["stats"] is not None and not _eq(out["stats"][n][c.n_iters, STAT_POSE:], slot):
                            bad(tp + "final stats row's pose is not pose_out")
    if c.c_ncall > 0:
        if out["pose_out"] is not None and not is_sent(out["pose_out"]):
            bad("a coalesced launch wrote the batch pose_out")
        for i in range(c.c_ncall):
            for li in range(c.c_len[i]):
                if (i, li) not in want_coal and not is_sent(out["c_pose_out"][i][li]):
                    bad(f"per-call output [{i}][{li}] written by no pair of this launch")
    if c.pose_lin is not None:
        if not _eq(out["pose_lin"][c.it & 1], c.pose_lin[c.it & 1]):
            bad("the pose_lin buffer this launch reads was written")
        for m in range(c.pc_np):
            if m not in wrote_lin and not _eq(out["pose_lin"][(c.it + 1) & 1][m], c.pose_lin[(c.it + 1) & 1][m]):
                bad(f"pose_lin slot {m} of no pair of this launch written")
    return fails, meas


def out_equal(a, b, skip=()):
    """outputs of two launches bit for bit -> names that differ"""
    diff = []
    for k in ("state", "pconst", "stats", "pose_out", "trace_decide", "pose_lin"):
        if k not in skip and a[k] is not None and b[k] is not None and not _eq(a[k], b[k]):
            diff.append(k)
    for i, (x, y) in enumerate(zip(a["c_pose_out"], b["c_pose_out"])):
        if not _eq(x, y):
            diff.append(f"c_pose_out[{i}]")
    for gi, (x, y) in enumerate(zip(a["g"], b["g"])):
        for k in x:
            if x[k] is not None and y[k] is not None and not _eq(x[k], y[k]):
                diff.append(f"g{gi}.{k}")
    return diff


def check_alone(c, run, out=None):
    """every group of the launch (two-role launches; PC variants at w_pc = 0) equals the group launched alone through variant 0, bit for bit;
    sweep cases: target 1 of the B = 3 launch equals the target launched alone"""
    out = out or run(c)
    fails = []
    if "alone_target" in c.claims:
        o1 = run(alone(c, 0, 1))
        g = c.groups[0]
        for k in ("export_out", "delta_out", "js", "jpart"):
            if out["g"][0][k] is not None and o1["g"][0][k] is not None and not _eq(out["g"][0][k][1], o1["g"][0][k][0]):
                fails.append(f"{c.name}: target 1's {k} differs from the target launched alone")
        for s in range(g.NS):
            if not _eq(out["state"][s * g.B + 1], o1["state"][s]):
                fails.append(f"{c.name}: target 1's source {s} state differs from the target launched alone")
    if "alone_group" in c.claims:
        for gi, g in enumerate(c.groups):
            o1 = run(alone(c, gi))
            n = g.NS * g.B
            for k in ("state", "pconst", "stats", "pose_out", "trace_decide"):
                if out[k] is not None and not _eq(out[k][g.n0:g.n0 + n], o1[k][:n]):
                    fails.append(f"{c.name}: group {gi}: {k} differs from the group launched alone through variant 0")
            for k, v in out["g"][gi].items():
                if v is not None and not _eq(v, o1["g"][0][k]):
                    fails.append(f"{c.name}: group {gi}: {k} differs from the group launched alone through variant 0")
    return fails


def check_repeat(c, run, out=None, times=3):
    out = out or run(c)
    fails = []
    for i in range(times - 1):
        d = out_equal(out, run(c))
        if d:
            fails.append(f"{c.name}: launch {i + 2} of the same case differs in {d}")
    return fails


def check_m_export(c, run, out=None):
    """js.M's right-hand side of an accepting launch without the pose-consistency term is the export of the same records, bit for bit"""
    out = out or run(c)
    d = clone(c, name=c.name + "/export")
    for g in d.groups:
        g.export = True
    xo = run(d)
    fails = []
    for gi, g in enumerate(c.groups):
        L = layout(g.NS)
        for b in range(g.B):
            M = out["g"][gi]["js"][b]["M"][:L.NP * L.NC].reshape(L.NP, L.NC)
            if not _eq(-M[:, L.NP], xo["g"][gi]["export_out"][b, 2:2 + L.NP]) or not _eq(out["g"][gi]["js"][b]["cost_cur"], xo["g"][gi]["export_out"][b, 0]):
                fails.append(f"{c.name}: group {gi} target {b}: js.M / cost_cur are not the export of the same records")
    return fails


def wants_m_export(c):
    return c.mode == 0 and not pc_compiled(c) and not any(g.export for g in c.groups) and all(e.decide for row in exact(c) for e in row)


def report_line(c, meas, nfail):
    return (f"{c.name:46s} | {c.group:30s} | judged {int(c.judged)} fails {nfail} | d x{meas['ratio_d']:.3f} E {meas['E_d']:.2e} | T x{meas['ratio_T']:.3f} E {meas['E_T']:.2e} | "
            f"sum {meas['sum']:.3f} pose {meas['pose']:.3f} const {meas['const']:.3f}")


# ----------------------------------------------------------------------------------------------------------------------- case lists
def sweep_cases():
    out = []
    for NS in (1, 2, 3, 4):
        for nblk in sweep_nblk(NS):
            g = group(NS, 3, make_jrecords(100 + nblk, NS, 3, nblk), export=True, seed=nblk)
            out.append(case(f"sweep S{NS} nblk{nblk}", f"sweep S{NS}", [g], claims=("sweep", "alone_target"), seed=nblk))
    return out


SPLIT_NBLK = lambda G: sorted({1, G - 1, G, G + 1, 480, 481, 1833})


def split_cases():
    out = []
    for NS in (1, 2, 4):
        for G in (2, 3, 4, 8):
            for nblk in SPLIT_NBLK(G):
                rec3 = make_jrecords(200 + nblk, NS, 3, nblk)
                for B in (1, 3):
                    rec = rec3 if B == 3 else _first_target(200 + nblk, NS, nblk)
                    g = group(NS, B, rec, nsplit=G, export=True, seed=nblk)
                    cl = ("split",) + (("empty_share",) if any(hi <= lo for lo, hi in shares(nblk, G)) else ()) + (("repeat",) if nblk in (G + 1, 481) else ())
                    out.append(case(f"split S{NS} G{G} nblk{nblk} B{B}", f"split sum S{NS}", [g], claims=cl, seed=nblk))
        # ... and through a full step: the last arriver solves what the partials add up to
        for G, nblk in ((2, 481), (3, 2), (8, 9)):
            g = group(NS, 3, make_jrecords(200 + nblk, NS, 3, nblk), nsplit=G, seed=G)
            out.append(case(f"split step S{NS} G{G} nblk{nblk}", f"split sum S{NS}", [g], it=1, claims=("split", "repeat"), seed=G))
    return out


@functools.lru_cache(maxsize=None)
def _first_target(seed, NS, nblk):
    r = make_jrecords(seed, NS, 3, nblk)
    out = np.concatenate([r[:1], r[3:]])
    out.setflags(write=False)
    return out


LM = dict(solver=1, lam_up=10.0, lam_down=0.1, lam_min=1e-5)


def path_cases():
    out = []
    for NS in (1, 2, 3, 4):
        tg, grp = f"S{NS}", f"solver paths S{NS}"
        rec = lambda seed, B=2, nblk=5: make_jrecords(seed, NS, B, nblk)
        for it in (0, 2, 3):
            out.append(case(f"gn it{it} {tg}", grp, [group(NS, 2, rec(300 + it), seed=it, lam=1e-3, have_cur=1, cost_cur=-1.0)], it=it, seed=it,
                            claims=("accept",) + (("gn_final",) if it == 3 else ()) + (("lam0",) if it == 0 else ())))
        out.append(case(f"lm first {tg}", grp, [group(NS, 2, rec(311), seed=11, lam=1e-2, have_cur=1, cost_cur=-5.0)], seed=11, claims=("accept", "lam0"), **LM))
        out.append(case(f"lm accept {tg}", grp, [group(NS, 2, rec(312), seed=12, lam=1e-2, have_cur=1, cost_cur=1e3)], it=1, seed=12, claims=("accept", "lam_down"), **LM))
        out.append(case(f"lm accept floor {tg}", grp, [group(NS, 2, rec(313), seed=13, lam=3e-5, have_cur=1, cost_cur=1e3)], it=1, seed=13,
                        claims=("accept", "lam_floored"), **LM))
        out.append(case(f"lm accept at floor {tg}", grp, [group(NS, 2, rec(317), seed=17, lam=float(np.float32(1e-5)), have_cur=1, cost_cur=1e3)], it=2, seed=17,
                        claims=("accept", "lam_floored"), **LM))
        out.append(case(f"lm no accepted state {tg}", grp, [group(NS, 2, rec(318), seed=18, lam=1e-2, have_cur=0, cost_cur=-5.0)], it=1, seed=18,
                        claims=("accept", "lam_same"), **LM))
        out.append(case(f"lm reject {tg}", grp, [group(NS, 2, rec(314), seed=14, lam=1e-3, have_cur=1, cost_cur=-1.0)], it=2, seed=14, claims=("reject", "stored_differs"), **LM))
        out.append(case(f"lm mode1 kept {tg}", grp, [group(NS, 2, rec(315), seed=15, lam=1e-3, have_cur=1, cost_cur=1e3)], mode=1, it=4, seed=15, claims=("accept",), **LM))
        out.append(case(f"lm mode1 dropped {tg}", grp, [group(NS, 2, rec(316), seed=16, lam=1e-3, have_cur=1, cost_cur=-1.0)], mode=1, it=4, seed=16, claims=("reject",), **LM))
        tie = dyadic_records(NS, [1.0] * (6 * NS), [0.125] * (6 * NS), cost=1.25)
        out.append(case(f"lm tie mode0 {tg}", grp, [group(NS, 1, tie, seed=19, lam=1e-3, have_cur=1, cost_cur=1.25)], it=1, seed=19, claims=("tie", "reject"), **LM))
        out.append(case(f"lm tie mode1 {tg}", grp, [group(NS, 1, tie, seed=20, lam=1e-3, have_cur=1, cost_cur=1.25)], mode=1, it=4, seed=20, claims=("tie", "reject"), **LM))
        out.append(case(f"lm just below {tg}", grp, [group(NS, 1, tie, seed=21, lam=1e-3, have_cur=1, cost_cur=float(np.nextafter(1.25, 2)))], it=1, seed=21,
                        claims=("accept", "cost_exact"), **LM))
        z = dyadic_records(NS, [1.0] * (6 * NS), [0.125] * (6 * NS))
        z[0, :, layout(NS).S + 1] = 0
        out.append(case(f"count 0 {tg}", grp, [group(NS, 1, z, seed=22)], it=1, seed=22, claims=("count0", "zero_step")))
        h = [1.0] * (6 * NS)
        h[6 * NS - 4] = -0.5
        out.append(case(f"negative pivot {tg}", grp, [group(NS, 1, dyadic_records(NS, h, [0.125] * (6 * NS)), seed=23, lam=1e-4, have_cur=1, cost_cur=1e3)], it=1, seed=23,
                        claims=("bad_pivot", "accept"), **LM))
    return out


def norm_cases():
    out = []
    for NS in (1, 2):
        rec = make_jrecords(400 + NS, NS, 4, 6)
        out.append(case(f"norms none S{NS}", "normalisers", [group(NS, 4, rec, seed=1)], it=1, seed=41, claims=("an_records",)))
        out.append(case(f"norms one group S{NS}", "normalisers", [group(NS, 4, rec, seed=2, norms=[[321, 123]], norm_B=0, c_f=0.25)], it=1, seed=42, claims=("an_norms",)))
        out.append(case(f"norms two groups S{NS}", "normalisers", [group(NS, 4, rec, seed=3, norms=[[321, 123], [77, 5]], norm_B=2, c_f=1.0)], it=1, seed=43,
                        claims=("an_norms", "two_groups")))
        out.append(case(f"norms zero count S{NS}", "normalisers", [group(NS, 4, rec, seed=4, norms=[[321, 123], [0, 5]], norm_B=2, c_f=1.0)], it=1, seed=44,
                        claims=("an_norms", "group_zero")))
        out.append(case(f"norms two groups export S{NS}", "normalisers", [group(NS, 4, rec, seed=5, norms=[[321, 123], [77, 5]], norm_B=2, c_f=0.25, export=True)],
                        seed=45, claims=("an_norms", "two_groups")))
    return out


CS = (1, 1, 1, 128, 128, 128)          # column scales 1 : 2^7 per source -> entries 1 : 1.6e4, as translation : rotation


def cond_cases():
    out = []
    for NS in (1, 2, 3, 4):
        grp = f"conditioning S{NS}"
        for cond in (1.0, 1e4, 1e8):
            out.append(case(f"cond {cond:.0e} S{NS}", grp, [group(NS, 1, spd_records(int(math.log10(cond)) + 3, NS, cond), seed=1)], lam0=0.0, seed=51, claims=(("cond", cond),)))
        for cond in (1.0, 1e2, 1e4):
            out.append(case(f"cond {cond:.0e} scaled S{NS}", grp, [group(NS, 1, spd_records(int(math.log10(cond)) + 30, NS, cond, colscale=CS), seed=2)], lam0=0.0, seed=52,
                            claims=(("cond_scaled", cond * 2.0 ** 14),)))
        out.append(case(f"cond 1e13 S{NS} (printed)", f"beyond the judged range S{NS}", [group(NS, 1, spd_records(99, NS, 1e13), seed=3)], lam0=0.0, seed=53, judged=False,
                        claims=(("cond_beyond", 1e13),)))
    return out


def block_cases():
    out = []
    for NS in (2, 4):
        g = group(NS, 2, make_jrecords(600 + NS, NS, 2, 7, blockdiag=True), seed=6)
        out.append(case(f"block diagonal S{NS}", "block structure", [g], it=1, seed=61, claims=("blockdiag",)))
    return out


def retraction_cases():
    """S = 4: the four 16-lane groups of wave 0 carry four different steps, set exactly through the reject path (stored system
    [2^40 I | 2^40 x], lambda 0 from the schedule: 0 x lambda_up)"""
    big = 2.0 ** 40
    sets = {"a": [[0.01, 0.02, 0.03, 0, 0, X_LO], [0.01, 0.02, 0.03, 0, 0, X_HI], [0, 0, 0, 0, 0, 0], [0.05, -0.1, 0.02, 1.0, 2.0, 2.0]],
            "b": [[0.05, 0, 0, 0.6, 0.8, 0], [0, 0, 0, 0, 0, 0], [0.25, -0.5, 0.125, 0, 0, 0], [0.01, 0, 0, 0, X_LO, 0]]}
    out = []
    for nm, steps in sets.items():
        g = group(4, 1, make_jrecords(700, 4, 1, 3), seed=7, lam=0.0, have_cur=1, cost_cur=-1.0)
        M = np.zeros((24, 25))
        M[:, :24] = np.eye(24) * big
        M[:, 24] = np.array(steps).reshape(24) * big
        g.js[0]["M"][:600] = M.reshape(-1)
        out.append(case(f"retract {nm} S4", "retraction", [g], it=1, seed=71, claims=("reject", ("steps", tuple(map(tuple, steps)))), **LM))
    return out


def _pose_lin(npairs, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([pose_T(rng.normal(scale=[0.05, 0.05, 0.05, 0.2, 0.2, 0.2])) for _ in range(npairs)]) for _ in range(2)])


def pc_cases():
    out = []
    for variant in (2, 4):
        for NS in (1, 2, 4):
            for it in (1, 2):
                B = 2
                SB = NS * B
                for order in (("fwd", "inv")[(it + NS // 2) % 2],):       # both production layouts, each at an even and an odd iteration per variant
                    ga = group(NS, B, make_jrecords(800 + NS, NS, B, 5), seed=8, norms=[[300, 200]], c_f=1.0)
                    groups = [ga]
                    slots = 2 * SB + 1
                    if variant == 4:
                        gb = group(1, SB, make_jrecords(850 + NS, 1, SB, 4), seed=9, norms=[[200, 300]], c_f=0.25)
                        groups.append(gb)
                    pl = _pose_lin(slots, 80 + it)
                    c = case(f"pc v{variant} S{NS} it{it} {order}", f"pose consistency v{variant}", groups, variant=variant, it=it, seed=81, w_pc=0.1 / (6 * SB), pc_eps=1e-3,
                             pose_lin=pl, claims=("pc", ("layout", order)))
                    a0, p0 = (0, SB) if order == "fwd" else (SB, 0)
                    ga.pc_self0, ga.pc_part0 = a0, p0
                    if variant == 4:
                        groups[1].pc_self0, groups[1].pc_part0 = p0, a0
                    # pair 0 of group a: partner almost its negative pose -> residual components above eps, below it and exactly zero
                    pz = np.array([0.03, -0.02, 0.0, 0.1, -0.05, 0.2])
                    c.state[0]["Ttry"] = pose_T(pz)
                    c.pose_lin[it & 1][p0] = pose_T(-pz + np.array([2e-4, -3e-4, 0.0, 0.05, 2e-4, -0.1]))
                    out.append(c)
    return out


def coal_cases():
    out = []
    for ncall, cB, NS in ((2, 1, 2), (3, 2, 1), (2, 2, 3)):
        B = ncall * cB
        g = group(NS, B, make_jrecords(900 + ncall, NS, B, 4), seed=9, norms=[[100 + 7 * i, 50] for i in range(ncall)], norm_B=cB, c_f=1.0)
        out.append(case(f"coalesced {ncall}x{cB} S{NS}", "coalesced routing", [g], it=3, seed=91, c_ncall=ncall, c_B=cB, c_S=NS, c_len=(2 * NS * cB,) * ncall,
                        claims=("gn_final", "coal")))
    return out


def role_cases():
    out = []
    for variant in (1, 2, 3, 4):
        for NS in (2, 3):
            for kind in ("gn last", "split"):
                B = 2
                G = 2 if kind == "split" else 1
                ga = group(NS, B, make_jrecords(1000 + NS, NS, B, 9), seed=10, nsplit=G, norms=[[300, 200]], c_f=1.0)
                groups = [ga]
                if variant >= 3:
                    groups.append(group(1, NS * B, make_jrecords(1050 + NS, 1, NS * B, 6), seed=11, nsplit=(3 if kind == "split" else 1), norms=[[200, 300]], c_f=0.25))
                pl = None
                if variant in (2, 4):
                    pl = _pose_lin(2 * NS * B + 1, 100 + NS)
                c = case(f"roles v{variant} S{NS} {kind}", f"two-role launches v{variant}", groups, variant=variant, it=3 if kind == "gn last" else 1, seed=101, pose_lin=pl,
                         w_pc=0.0, claims=("alone_group",) + (("gn_final",) if kind == "gn last" else ()))
                if pl is not None:
                    ga.pc_self0, ga.pc_part0 = 0, NS * B
                    if variant == 4:
                        groups[1].pc_self0, groups[1].pc_part0 = NS * B, 0
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = sweep_cases() + split_cases() + path_cases() + norm_cases() + cond_cases() + block_cases() + retraction_cases() + pc_cases() + coal_cases() + role_cases()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def by_name():
    return {c.name: c for c in all_cases()}


# the launches tcsfm_debug_solve_joint must refuse: (name, case, words of the message of the check that must be the one to fire)
def refusal_cases():
    b = by_name()
    gn, pc, co, sp, rl = b["gn it0 S2"], b["pc v2 S2 it1 fwd"], b["coalesced 2x1 S2"], b["split step S2 G2 nblk481"], b["roles v3 S2 gn last"]

    def grp(c, gi=0, **kw):
        d = clone(c)
        for k, v in kw.items():
            assert hasattr(d.groups[gi], k), k
            setattr(d.groups[gi], k, v)
        return d
    short = grp(b["norms two groups S2"], norms=np.array([[321, 123]], np.int32))
    return [("variant 5", clone(gn, variant=5), "variant must be"), ("NS 5", clone(gn, NS=5), "NS must be"), ("B 0", grp(gn, B=0), "1 <= B <= b_alloc"),
            ("nblk 0", grp(gn, nblk=0), "nblk must be"), ("nsplit 0", grp(gn, nsplit=0), "nsplit out of range"), ("nsplit 9", grp(sp, nsplit=9), "nsplit out of range"),
            ("jtick not zero", grp(sp, tick_in=1), "non-zero jtick"), ("pair outside", clone(gn, n_alloc=3), "pair index is outside"),
            ("norms short", short, "norms is shorter"), ("it > n_iters", clone(gn, it=5), "it <= n_iters"), ("mode 2", clone(gn, mode=2), "mode must be"),
            ("mode 1 gn", clone(gn, mode=1, it=4), "solver must be LM"), ("pc on v0", clone(gn, w_pc=0.01), "no pose-consistency term"),
            ("pc on v3", clone(rl, w_pc=0.01), "no pose-consistency term"), ("pc without pose_lin", clone(pc, pose_lin=None, pc_np=0), "pose_lin and pc_np are required"),
            ("partner outside", grp(pc, pc_part0=6), "partner index is outside"), ("own slot outside", grp(pc, pc_self0=7), "own slot is outside"),
            ("coal outside", clone(co, c_len=(4, 0)), "per-call arrays"), ("coal slot short", clone(co, c_len=(4, 1)), "per-call arrays"),
            ("coal two-role", clone(rl, c_ncall=2, c_B=1, c_S=2, c_len=(4, 4)), "variants 0 to 2 only"), ("groups overlap", grp(rl, 1, n0=2), "pairs overlap")]
