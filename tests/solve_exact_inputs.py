"""ONE launch of the pose solve kernels (csrc/kernels.h solve_body: k_solve, k_solve_lean, the pair role of k_solve_front) on records and
optimiser state given by the test, against exact arithmetic.  Host only: the cases, the exact reference, a float64 twin (the yardstick, and
the GPU's stand-in with switchable planted faults in tests/test_solve_exact_inputs_cpu.py) and the judge.  tests/test_gpu_solve_exact.py
runs the cases through tcsfm_debug_solve.

The reference models what a launch is documented to do -- sum the records, normalise, add the scale prior and the pose-consistency term,
decide (Gauss-Newton: always; LM: a strictly lower cost), damp, solve (H + lambda diag H + 1e-12 I) d = -g, retract T <- exp(d) T, write the
next linearisation's constants, emit the pose -- not the kernel's operation order.  Record sums, normaliser, costs, the system and its
solution are fractions.Fraction of the float bits; exp / sin / cos / atan2 / asin (retraction, pose extraction, the pose-consistency term, the
additive-Euler re-solve) are mpmath at 80 digits; decisions and the damping schedule are Python floats (one multiply, one max).

The judge (judge_case):
  record sums (mode 2 export)   |got - exact| <= (ngrp + 4) 2^-53 (an sum|v_photo| + b_dc sum|v_dc|) per entry: an fp64 sum of ngrp terms in
                                any order plus the roundings of the assembly (normaliser, two products, one sum); n_mask exact
  step d, new trial transform   E(kernel) <= 4 E(float64 twin) + 8 2^-52 max|exact|, E = max |x - exact| over the vector (margin 4 as in
                                tests/linearize_exact_inputs.py; unpivoted Gauss-Jordan and Cholesky are both backward stable on SPD systems)
  lambda, have_cur, decisions, what is written where, what is left alone: bit for bit
  PairConst                     A, kt, R, t within 1 ulp32 (es: 2) of the exact value rounded to fp32; K and the image index unchanged
  pose_out, stats pose, scale   |got - exact| <= 4 E(float32 numpy twin of the extraction) + 2^-23 max(1, |exact|) (max norms over the 6-vector)

GOLDEN_COND_MAX: the largest cond(H) the float64 oracle gives on the golden pairs s8x16 / s24x40 / s48x160 (all poses, 6 and 7 unknowns):
2.752e4 (s48x160 pose 1, 7 unknowns with the scale prior of weight 1 in H).  Left out of it are the pairs whose H cannot have full rank: the
poses with an EMPTY mask (s8x16 poses 3 and 4, s24x40 pose 4: H = 0) and pose 6 of s8x16, whose mask is ONE pixel (three rows: rank 3,
"cond" 4e17, i.e. singular to rounding) -- no solver is judged there; such systems are printed, not judged
(tests/test_solve_exact_inputs_cpu.py recomputes the value).  Judged cases span 1 .. 1e8 > 100 x 2.752e4."""
import functools
import math
import types
from fractions import Fraction as F

import mpmath as mpm
import numpy as np

mp = mpm.mp
mp.dps = 80
GOLDEN_COND_MAX = 2.752e4
COND_JUDGED_MAX = 1e10
HW = 16 * 16                      # the handle the GPU test creates: b_dc = w_dc / (H W)
NSTAT, STAT_POSE = 10, 4
SENT = 0x5A                       # every output byte before the launch
TC_MAX_COAL = 16

STATE_DT = np.dtype([("Tcur", "f8", 12), ("Ttry", "f8", 12), ("scur", "f8"), ("stry", "f8"), ("s0", "f8"), ("lam", "f8"), ("cost_cur", "f8"),
                     ("M8", "f8", 64), ("K", "f8", 9), ("have_cur", "i4"), ("pad", "i4")])
CONST_DT = np.dtype([("A", "f4", 9), ("kt", "f4", 3), ("R", "f4", 9), ("t", "f4", 3), ("fx", "f4"), ("fy", "f4"), ("cx", "f4"), ("cy", "f4"),
                     ("ki0", "f4"), ("ki2", "f4"), ("ki4", "f4"), ("ki5", "f4"), ("es", "f4"), ("img", "i4"), ("pad", "i4", 2)])


def layout(npar):
    nh = npar * (npar + 1) // 2
    return types.SimpleNamespace(NH=nh, HP=0, GP=nh, HD=nh + npar, GD=2 * nh + npar, S=2 * nh + 2 * npar, NACC=2 * nh + 2 * npar + 3)


def live_accs(npar, has_dc):
    L = layout(npar)
    return list(range(L.NACC)) if has_dc else list(range(L.NH + npar)) + [L.S, L.S + 1, L.S + 2]


def split(variant, npar, has_dc):
    """(parts, NB) of the record sum: the threads are (accumulator slot, record subset), a batch is NB loads per thread"""
    nt = 256 if variant == 0 else 1024
    nlive = len(live_accs(npar, has_dc))
    apad = 32 if nlive <= 32 else (64 if nlive <= 64 else 128)
    return nt // apad, (16 if nt >= 1024 else 32)


def sweep_ngrp(variant, npar, has_dc):
    p, nb = split(variant, npar, has_dc)
    return sorted({1, 2, p - 1, p, p + 1, nb * p - 1, nb * p, nb * p + 1, 240, 2 * nb * p + 3})


# ------------------------------------------------------------------------------------------------------------------------------ cases
K0 = np.array([58.0, 0, 31.5, 0, 61.0, 23.25, 0, 0, 1])


def _tri(npar, r, c):
    hi, lo = max(r, c), min(r, c)
    return hi * (hi + 1) // 2 + lo


def make_records(seed, n_alloc, N, ngrp, npar, has_dc, colscale=None, gscale=1.0, count=37.0):
    """float32 records [n_alloc][ngrp][nacc]: every record is a sum of three J' W J / J' W r rows plus a component distinct per (pair, record,
    accumulator) -- a diagonally dominant SPD block for H -- so the totals are SPD and no two records agree anywhere; dead accumulators and the
    slack pairs hold NaN"""
    L = layout(npar)
    rng = np.random.default_rng(seed)
    rec = np.full((n_alloc, ngrp, L.NACC), np.nan, np.float64)
    cs = np.ones(npar) if colscale is None else np.asarray(colscale, float)
    n_, r_, a_ = np.meshgrid(np.arange(N), np.arange(ngrp), np.arange(L.NACC), indexing="ij")
    dist = 0.01 * (1.0 + ((n_ * 389 + r_ * 31 + a_ * 7) % 997) / 997.0)
    for blk, (oh, og) in enumerate(((L.HP, L.GP), (L.HD, L.GD))):
        if blk == 1 and not has_dc:
            continue
        J = rng.normal(size=(N, ngrp, 3, npar)) * cs
        w = rng.uniform(0.5, 1.5, size=(N, ngrp, 3))
        res = rng.normal(size=(N, ngrp, 3)) * gscale
        Hm = np.einsum("nrk,nrki,nrkj->nrij", w, J, J)
        gv = np.einsum("nrk,nrki,nrk->nri", w, J, res)
        for i in range(npar):
            for j in range(i + 1):
                d = dist[:, :, oh + _tri(npar, i, j)] * cs[i] * cs[j]
                rec[:N, :, oh + _tri(npar, i, j)] = Hm[:, :, i, j] + d + (0.2 * cs[i] * cs[j] if i == j else 0.0)
            rec[:N, :, og + i] = gv[:, :, i] + dist[:, :, og + i] * cs[i] * gscale
    rec[:N, :, L.S] = rng.uniform(1.0, 2.0, size=(N, ngrp)) + dist[:, :, L.S]
    rec[:N, :, L.S + 1] = count + (np.arange(N)[:, None] * 5 + np.arange(ngrp)[None, :]) % 11         # integer mask counts
    rec[:N, :, L.S + 2] = rng.uniform(0.5, 1.0, size=(N, ngrp)) + dist[:, :, L.S + 2]
    return rec.astype(np.float32)


def pose_T(pose):
    """pose_vec2mat(-pose): [Rx(-rx) Ry(-ry) Rz(-rz) | -t], 3 x 4 row-major, float64"""
    a, b, c = -pose[3], -pose[4], -pose[5]
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    R = [[cb * cc, -cb * sc, sb], [ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb], [sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb]]
    return np.array([R[i] + [-pose[i]] for i in range(3)]).reshape(12)


def make_state(n_alloc, N, seed, lam=0.0, have_cur=0, cost_cur=0.0, s=(0.0, 0.0, 0.0)):
    st = np.zeros(n_alloc, STATE_DT)
    st.view(np.uint8)[:] = SENT
    rng = np.random.default_rng(seed + 1000)
    for n in range(N):
        st[n]["Tcur"] = pose_T(rng.normal(scale=[0.05, 0.05, 0.05, 0.2, 0.2, 0.2]))
        st[n]["Ttry"] = pose_T(rng.normal(scale=[0.05, 0.05, 0.05, 0.2, 0.2, 0.2]))
        st[n]["scur"], st[n]["stry"], st[n]["s0"] = s
        st[n]["lam"], st[n]["cost_cur"], st[n]["have_cur"], st[n]["pad"] = lam, cost_cur, have_cur, 0
        M8 = rng.normal(size=(8, 8))                       # a stored SPD system [H | -g]; the lanes outside it hold anything
        J = rng.normal(size=(12, 7))
        M8[:7, :7] = J.T @ J / 12 + 0.1 * np.eye(7)
        st[n]["M8"] = M8.reshape(64)
        st[n]["K"] = K0 * (1 + 0.01 * n) * np.array([1, 1, 1, 1, 1, 1, 1, 1, 0]) + np.array([0, 0, 0, 0, 0, 0, 0, 0, 1.0])
    return st


def make_const(n_alloc, N):
    pc = np.zeros(n_alloc, CONST_DT)
    pc.view(np.uint8)[:] = SENT
    for n in range(N):
        for k in ("A", "kt", "R", "t", "es"):
            pc[n][k] = -77.0
        pc[n]["fx"], pc[n]["fy"], pc[n]["cx"], pc[n]["cy"] = 58, 61, 31.5, 23.25
        pc[n]["ki0"], pc[n]["ki2"], pc[n]["ki4"], pc[n]["ki5"] = 1 / 58, -31.5 / 58, 1 / 61, -23.25 / 61
        pc[n]["img"], pc[n]["pad"] = 3 + n, (11, 12)
    return pc


ALL_OUT = ("stats", "lin_out", "delta_out", "accept_out", "trace_decide", "pose_out", "log_scale_out")


def case(name, group, *, variant=0, npar=6, w_dc=0.0, solver=0, param=0, n_iters=4, lam_up=10.0, lam_down=0.1, lam_min=1e-5, prior_scale=0.0,
         mode=0, it=0, N=1, ngrp=5, seed=0, lam=0.0, have_cur=0, cost_cur=0.0, s=(0.0, 0.0, 0.0), want=ALL_OUT, judged=True, claims=(), **kw):
    c = types.SimpleNamespace(name=name, group=group, variant=variant, np=npar, w_dc=float(np.float32(w_dc)), solver=solver, param=param, n_iters=n_iters,
                              lam_up=float(np.float32(lam_up)), lam_down=float(np.float32(lam_down)), lam_min=float(np.float32(lam_min)),
                              prior_scale=float(np.float32(prior_scale)), mode=mode, it=it, N=N, n_alloc=N + 1, ngrp=ngrp, want=tuple(want), judged=judged,
                              claims=tuple(claims), rule=0, grp_fwd=0, n_pairs=0, scale_fwd=1.0, scale_inv=1.0, norms=None, norm_Bt=0, norm_B=0,
                              w_pc=0.0, pc_eps=1e-3, pose_lin=None, pc_np=0, pc_self0=0, pc_part0=0, c_ncall=0, c_B=0, c_S=0, c_n0=0, c_len=(), c_ls=())
    c.has_dc = c.w_dc > 0
    c.rec = kw.pop("rec", None)
    if c.rec is not None:
        c.ngrp = c.rec.shape[1]
    if c.rec is None:
        c.rec = make_records(seed, c.n_alloc, N, ngrp, npar, c.has_dc, colscale=kw.pop("colscale", None), gscale=kw.pop("gscale", 1.0))
    c.state = make_state(c.n_alloc, N, seed, lam=lam, have_cur=have_cur, cost_cur=cost_cur, s=s)
    c.pconst = make_const(c.n_alloc, N)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


def clone(c, **kw):
    d = types.SimpleNamespace(**vars(c))
    d.state, d.pconst, d.rec = c.state.copy(), c.pconst.copy(), c.rec.copy()
    d.pose_lin = None if c.pose_lin is None else c.pose_lin.copy()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def alone(c, n):
    """pair n of case c as a launch of its own (no rule, no pose consistency: those tie the pairs of a call together)"""
    d = clone(c, name=c.name + f"/alone{n}", N=1, n_alloc=2)
    d.rec = np.full((2,) + c.rec.shape[1:], np.nan, np.float32); d.rec[0] = c.rec[n]
    d.state = np.concatenate([c.state[n:n + 1], c.state[c.N:c.N + 1]]); d.pconst = np.concatenate([c.pconst[n:n + 1], c.pconst[c.N:c.N + 1]])
    return d


def new_outputs(c):
    """the output arrays of a launch before it: inputs where the kernel updates in place, the sentinel everywhere else"""
    nst = c.np * c.np + c.np + 4
    shapes = dict(stats=((c.n_alloc, c.n_iters + 1, NSTAT), np.float32), lin_out=((c.n_alloc, nst), np.float64), delta_out=((c.n_alloc, 8), np.float64),
                  accept_out=((c.n_alloc,), np.int32), trace_decide=((c.n_alloc,), np.int32), pose_out=((c.n_alloc, 6), np.float32),
                  log_scale_out=((c.n_alloc,), np.float32))
    o = dict(state=c.state.copy(), pconst=c.pconst.copy(), pose_lin=None if c.pose_lin is None else c.pose_lin.copy())
    for k, (shape, dt) in shapes.items():
        o[k] = None
        if k in c.want:
            o[k] = np.zeros(shape, dt); o[k].view(np.uint8)[:] = SENT
    o["c_pose_out"], o["c_ls_out"] = [], []
    for i in range(c.c_ncall):
        a = np.zeros((c.c_len[i], 6), np.float32); a.view(np.uint8)[:] = SENT
        b = np.zeros((c.c_len[i],), np.float32); b.view(np.uint8)[:] = SENT
        o["c_pose_out"].append(a); o["c_ls_out"].append(b if c.c_ls[i] else None)
    return o


def is_sent(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == SENT))


def coal_index(ncall, cB, cS, n):
    """(call, index of the pair in its call's stacked order): batch pair n over Bt = ncall cB targets, forward n = s Bt + b, inverse S Bt + s Bt + b;
    target b is local target b % cB of call b // cB"""
    Bt = ncall * cB
    inv = n >= cS * Bt
    q = n - cS * Bt if inv else n
    s, b = divmod(q, Bt)
    return b // cB, (cS * cB if inv else 0) + s * cB + b % cB


# ------------------------------------------------------------------------------------------------------------------- exact reference
def _exact_sum(col):
    """exact sum of a float32 column as a Fraction (integers scaled by a power of two)"""
    m, e = np.frexp(col.astype(np.float64))
    mi = (m * 2.0 ** 53).astype(np.int64)
    sh = e.astype(np.int64) - 53
    lo = int(sh.min())
    tot = sum(int(a) << int(b - lo) for a, b in zip(mi, sh))
    return F(tot) * (F(2) ** lo)


def _mpf(x):
    return mpm.mpf(x.numerator) / x.denominator if isinstance(x, F) else mpm.mpf(x)


def _frac(x):
    return x if isinstance(x, F) else F(int(mpm.floor(mpm.ldexp(x, 400) + 0.5)), 2 ** 400)


def mp_pose_of_T(T):
    """the reference's 6-vector of [R | t] = pose_vec2mat(-pose); sin(ry) beyond +-1 through rounding is clamped"""
    sb = max(-1, min(1, T[2]))
    return [-T[3], -T[7], -T[11], -mpm.atan2(-T[6], T[10]), -mpm.asin(sb), -mpm.atan2(-T[1], T[0])]


def mp_T_of_pose(p):
    a, b, c = -p[3], -p[4], -p[5]
    ca, sa, cb, sb, cc, sc = mpm.cos(a), mpm.sin(a), mpm.cos(b), mpm.sin(b), mpm.cos(c), mpm.sin(c)
    R = [[cb * cc, -cb * sc, sb], [ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb], [sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb]]
    return [x for i in range(3) for x in R[i] + [-p[i]]]


def _hat(w):
    return mpm.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def mp_se3_exp(xi):
    rho, phi = mpm.matrix(xi[:3]), xi[3:6]
    t2 = sum(x * x for x in phi)
    if t2 == 0:
        A, B, Cc = mpm.mpf(1), mpm.mpf(1) / 2, mpm.mpf(1) / 6
    else:
        t = mpm.sqrt(t2)
        A, B, Cc = mpm.sin(t) / t, (1 - mpm.cos(t)) / t2, (t - mpm.sin(t)) / (t2 * t)
    Kx = _hat(phi)
    R = mpm.eye(3) + A * Kx + B * Kx * Kx
    v = (mpm.eye(3) + B * Kx + Cc * Kx * Kx) * rho
    return [x for i in range(3) for x in [R[i, 0], R[i, 1], R[i, 2], v[i]]]


def mp_mul(A, B):
    out = []
    for i in range(3):
        for j in range(4):
            out.append(sum(A[4 * i + k] * B[4 * k + j] for k in range(3)) + (A[4 * i + 3] if j == 3 else 0))
    return out


def _euler_left_jacobian(p):
    """A = d(xi_left) / d(pose): T(pose + dp) ~ exp((A dp)^) T(pose); dphi = -Je dr, drho = -dt - [t']x Je dr, t' = -t, Je = [ex | Rx ey | Rx Ry ez] at -r"""
    ax, ay = -p[3], -p[4]
    ca, sa, cb, sb = mpm.cos(ax), mpm.sin(ax), mpm.cos(ay), mpm.sin(ay)
    Je = mpm.matrix([[1, 0, sb], [0, ca, -sa * cb], [0, sa, ca * cb]])
    TJ = _hat([-p[0], -p[1], -p[2]]) * Je
    A = mpm.zeros(6)
    for i in range(3):
        A[i, i] = -1
        for j in range(3):
            A[i, 3 + j], A[3 + i, 3 + j] = -TJ[i, j], -Je[i, j]
    return A


def _pivots_positive(A):
    """every pivot of the elimination without row exchanges positive (exactly: the matrix is positive definite when symmetric)"""
    n = len(A)
    A = [row[:] for row in A]
    for k in range(n):
        if not A[k][k] > 0:
            return False
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            for j in range(k, n):
                A[i][j] -= f * A[k][j]
    return True


def _solve(A, b):
    n = len(A)
    M = [A[i][:] + [b[i]] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: abs(M[i][k]))
        M[k], M[p] = M[p], M[k]
        for i in range(n):
            if i != k and M[i][k] != 0:
                f = M[i][k] / M[k][k]
                M[i] = [x - f * y for x, y in zip(M[i], M[k])]
    return [M[i][n] / M[i][i] for i in range(n)]


def _damped_step(H, g, lam):
    n = len(H)
    A = [[H[i][j] + ((F(lam) * H[i][i] + F(1e-12)) if i == j else 0) for j in range(n)] for i in range(n)]
    if not _pivots_positive(A):
        return [F(0)] * n, False
    return _solve(A, [-x for x in g]), True


def partner_of(c, n):
    return c.pc_part0 + n if c.pc_np > 0 else (n + c.grp_fwd if n < c.grp_fwd else n - c.grp_fwd)


def pc_on(c):
    return c.np == 6 and c.rule and c.w_pc > 0 and c.pose_lin is not None and c.variant in (0, 3)


def exact_pair(c, n):
    """one pair of one launch in exact arithmetic -> namespace"""
    L, npar = layout(c.np), c.np
    live = live_accs(npar, c.has_dc)
    tot = {a: _exact_sum(c.rec[n, :, a]) for a in live}
    sab = {a: float(np.abs(c.rec[n, :, a].astype(np.float64)).sum()) for a in live}
    nmask = tot[L.S + 1]
    an = 1 / nmask if nmask > 0 else F(0)
    if c.rule:
        if c.norms is not None:
            kn = F(int(c.norms[(n % c.norm_Bt) // c.norm_B if c.norm_B > 0 else 0][0 if n < c.grp_fwd else 1]))
        else:
            g0, g1 = (0, c.grp_fwd) if n < c.grp_fwd else (c.grp_fwd, c.n_pairs)
            kn = sum((_exact_sum(c.rec[m, :, L.S + 1]) for m in range(g0, g1)), F(0))
        an = F(c.scale_fwd if n < c.grp_fwd else c.scale_inv) / kn if kn > 0 else F(0)
    b_dc = F(c.w_dc) / HW
    bdc = b_dc if c.has_dc else F(0)
    e = types.SimpleNamespace(nmask=nmask, an=an, cost_photo=an * tot[L.S], cost_dc=b_dc * tot[L.S + 2])
    e.cost = e.cost_photo + e.cost_dc
    fan, fb = float(an), float(bdc)
    H = [[an * tot[L.HP + _tri(npar, i, j)] + (bdc * tot[L.HD + _tri(npar, i, j)] if c.has_dc else 0) for j in range(npar)] for i in range(npar)]
    g = [an * tot[L.GP + i] + (bdc * tot[L.GD + i] if c.has_dc else 0) for i in range(npar)]
    e.bH = np.array([[fan * sab[L.HP + _tri(npar, i, j)] + (fb * sab[L.HD + _tri(npar, i, j)] if c.has_dc else 0) for j in range(npar)] for i in range(npar)])
    e.bg = np.array([fan * sab[L.GP + i] + (fb * sab[L.GD + i] if c.has_dc else 0) for i in range(npar)])
    e.bcost = fan * sab[L.S] + float(b_dc) * sab[L.S + 2]
    e.bphoto, e.bdc = fan * sab[L.S], float(b_dc) * sab[L.S + 2]
    S = c.state[n]
    if npar == 7 and c.mode != 2:
        ds = F(float(S["stry"])) - F(float(S["s0"]))
        ps = F(c.prior_scale)
        e.cost += ps * ds * ds
        H[6][6] += 2 * ps
        g[6] += 2 * ps * ds
    if pc_on(c):
        pT = c.pose_lin[c.it & 1][partner_of(c, n)]
        pm, pp = mp_pose_of_T([mpm.mpf(float(x)) for x in S["Ttry"]]), mp_pose_of_T([mpm.mpf(float(x)) for x in pT])
        Ai = mpm.inverse(_euler_left_jacobian(pm))           # dp = A^-1 dxi
        w, eps = mpm.mpf(c.w_pc), mpm.mpf(c.pc_eps)
        r = [a + b for a, b in zip(pm, pp)]
        den = [max(abs(x), eps) for x in r]
        e.cost += _frac(sum(w * abs(x) / 2 for x in r))
        e.pc_r = [float(x) for x in r]
        G, D = [w * x / d for x, d in zip(r, den)], [2 * w / d for d in den]
        for i in range(6):
            g[i] += _frac(sum(Ai[k, i] * G[k] for k in range(6)))
            for j in range(6):
                H[i][j] += _frac(sum(Ai[k, i] * D[k] * Ai[k, j] for k in range(6)))
    e.H, e.g = H, g
    if c.mode == 2:
        return e
    lam, have, cost_cur = float(S["lam"]), int(S["have_cur"]), float(S["cost_cur"])
    e.lam_out, e.final = lam, False
    if c.mode == 1:
        e.decide = e.cost < F(cost_cur)
        e.Tfin = [mpm.mpf(float(x)) for x in (S["Ttry"] if e.decide else S["Tcur"])]
        e.sfin = mpm.mpf(float(S["stry"] if e.decide else S["scur"]))
        e.final = True
        return e
    e.decide = c.solver == 0 or not have or e.cost < F(cost_cur)
    if e.decide:
        if c.solver == 1 and have:
            lam = max(lam * c.lam_down, c.lam_min)
        Hs, gs = H, g
    else:
        lam = lam * c.lam_up
        M8 = S["M8"].reshape(8, 8)
        Hs = [[F(float(M8[i, j])) for j in range(npar)] for i in range(npar)]
        gs = [-F(float(M8[i, 7])) for i in range(npar)]
    e.lam_out = lam
    e.Hs = Hs
    Tacc = [mpm.mpf(float(x)) for x in (S["Ttry"] if e.decide else S["Tcur"])]
    sacc = mpm.mpf(float(S["stry"] if e.decide else S["scur"]))
    if c.param == 0:
        d, e.ok = _damped_step(Hs, gs, lam)
        e.d = [_mpf(x) for x in d]
        e.Tnew = mp_mul(mp_se3_exp(e.d[:6]), Tacc)
    else:
        pose = mp_pose_of_T(Tacc)
        Af = mpm.eye(npar)
        Af[:6, :6] = _euler_left_jacobian(pose)
        Hm, gm = mpm.matrix([[_mpf(x) for x in row] for row in Hs]), mpm.matrix([_mpf(x) for x in gs])
        Hp, gp = Af.T * Hm * Af, Af.T * gm
        d, e.ok = _damped_step([[_frac(Hp[i, j]) for j in range(npar)] for i in range(npar)], [_frac(gp[i]) for i in range(npar)], lam)
        e.d = [_mpf(x) for x in d]
        e.Tnew = mp_T_of_pose([a + b for a, b in zip(pose, e.d[:6])])
        # delta_out stays the step in the left-perturbation chart (its consumer, the dense update, is SE(3) only); the additive-Euler step
        # itself is judged through the trial transform and the trial scale
        e.d_out = [_mpf(x) for x in _damped_step(Hs, gs, lam)[0]]
    e.snew = sacc + (e.d[6] if npar == 7 else 0)
    e.Tacc, e.sacc = Tacc, sacc
    if c.solver == 0 and c.it == c.n_iters - 1:
        e.final, e.Tfin, e.sfin = True, e.Tnew, e.snew
    return e


_EXACT = {}


def exact(c):
    if c.name not in _EXACT:
        _EXACT[c.name] = [exact_pair(c, n) for n in range(c.N)]
    return _EXACT[c.name]


# ---------------------------------------------------------------------------------------------------------------------- float64 twin
def pose_f32(T):
    """float32 numpy twin of the kernel's pose extraction"""
    T = np.asarray(T, np.float64).astype(np.float32)
    sb = np.float32(min(max(T[2], np.float32(-1)), np.float32(1)))
    return np.array([-T[3], -T[7], -T[11], -np.arctan2(-T[6], T[10]), -np.arcsin(sb), -np.arctan2(-T[1], T[0])], np.float32)


def _pose64(T):
    sb = min(max(T[2], -1.0), 1.0)
    return np.array([-T[3], -T[7], -T[11], -math.atan2(-T[6], T[10]), -math.asin(sb), -math.atan2(-T[1], T[0])])


def _hat64(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _exp64(xi):
    rho, phi = xi[:3], xi[3:6]
    t2 = float(phi @ phi)
    if t2 < 1e-8:
        A, B, Cc = 1 - t2 / 6, 0.5 - t2 / 24, 1 / 6 - t2 / 120
    else:
        t = math.sqrt(t2)
        A, B, Cc = math.sin(t) / t, 2 * math.sin(t / 2) ** 2 / t2, (t - math.sin(t)) / (t2 * t)
        if t < 0.05:
            Cc = 1 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880
    Kx = _hat64(phi)
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) + A * Kx + B * Kx @ Kx
    T[:, 3] = (np.eye(3) + B * Kx + Cc * Kx @ Kx) @ rho
    return T


def _mul64(A, B):
    A, B = np.asarray(A).reshape(3, 4), np.asarray(B).reshape(3, 4)
    out = np.zeros((3, 4))
    out[:, :3] = A[:, :3] @ B[:, :3]
    out[:, 3] = A[:, :3] @ B[:, 3] + A[:, 3]
    return out.reshape(12)


def _jac64(p):
    ax, ay = -p[3], -p[4]
    ca, sa, cb, sb = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
    Je = np.array([[1, 0, sb], [0, ca, -sa * cb], [0, sa, ca * cb]])
    A = np.zeros((6, 6))
    A[:3, :3] = -np.eye(3); A[:3, 3:] = -_hat64(-np.asarray(p[:3])) @ Je; A[3:, 3:] = -Je
    return A


def _chol_step(H, g, lam, fault):
    A = H + np.diag((0.0 if fault == "undamped" else lam) * np.diag(H) + 1e-12)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return np.zeros(len(g)), False
    if not np.all(np.isfinite(Lc)):
        return np.zeros(len(g)), False
    d = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
    if fault == "rcp40":
        d = d * (1 + 2.0 ** -40)
    return d, True


def const_of(K, T, s, npar, dt=np.float64):
    """A = K (R - I) K^-1, kt = K t, R, t (and es = exp(s), 7 unknowns) in float64"""
    K, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 4)
    A = K @ (T[:, :3] - np.eye(3)) @ np.linalg.inv(K)
    return dict(A=A.reshape(9), kt=K @ T[:, 3], R=T[:, :3].reshape(9), t=T[:, 3].copy(), es=(1.0 if s == 0 else math.exp(s)) if npar == 7 else None)


def twin(c, fault=None):
    """the launch in numpy float64 with a Cholesky solve, as the oracle factorises -> outputs as new_outputs(); fault: a planted fault"""
    L, npar = layout(c.np), c.np
    o = new_outputs(c)
    live = live_accs(npar, c.has_dc)
    p_, nb_ = split(c.variant, npar, c.has_dc)
    b_dc = c.w_dc / HW
    bdc = b_dc if c.has_dc else 0.0
    for n in range(c.N):
        rows = c.rec[n].astype(np.float64)
        if fault == "drop_boundary" and c.ngrp > nb_ * p_:
            rows = np.delete(rows, nb_ * p_, axis=0)
        if fault == "neighbour":
            rows = rows.copy(); rows[-1] = c.rec[(n + 1) % c.N, -1] if c.N > 1 else rows[-1]
        tot = np.zeros(L.NACC)
        for a in (range(L.NACC) if fault == "dead_acc" else live):
            tot[a] = rows[:, a].sum()
        nmask = tot[L.S + 1]
        an = 1.0 / nmask if nmask > 0 else 0.0
        if c.rule:
            if c.norms is not None:
                kn = float(c.norms[(n % c.norm_Bt) // c.norm_B if c.norm_B > 0 else 0][0 if n < c.grp_fwd else 1])
            else:
                g0, g1 = (0, c.grp_fwd) if n < c.grp_fwd else (c.grp_fwd, c.n_pairs)
                kn = float(c.rec[g0:g1, :, L.S + 1].astype(np.float64).sum())
            an = (c.scale_fwd if n < c.grp_fwd else c.scale_inv) / kn if kn > 0 else 0.0
        if fault == "rcp40":
            an *= 1 + 2.0 ** -40
        cost_photo, cost_dc = an * tot[L.S], b_dc * tot[L.S + 2]
        cost = cost_photo + cost_dc
        H, g = np.zeros((npar, npar)), np.zeros(npar)
        bd = b_dc if fault == "dead_acc" else bdc
        for i in range(npar):
            for j in range(npar):
                H[i, j] = an * tot[L.HP + _tri(npar, i, j)] + bd * tot[L.HD + _tri(npar, i, j)]
            g[i] = an * tot[L.GP + i] + bd * tot[L.GD + i]
        S = c.state[n]
        if npar == 7 and c.mode != 2:
            ds = S["stry"] - S["s0"]
            cost += c.prior_scale * ds * ds
            H[6, 6] += 2 * c.prior_scale
            g[6] += 2 * c.prior_scale * ds
        if pc_on(c):
            per = c.pc_np if c.pc_np > 0 else c.n_pairs
            pi = partner_of(c, n)
            if fault == "partner_off":
                pi = (pi + 1) % per
            pm, pp = _pose64(S["Ttry"]), _pose64(c.pose_lin[c.it & 1][pi])
            Ai = np.linalg.inv(_jac64(pm))
            r = pm + pp
            den = np.maximum(np.abs(r), c.pc_eps)
            cost += float(np.sum(0.5 * c.w_pc * np.abs(r)))
            H += Ai.T @ np.diag(2 * c.w_pc / den) @ Ai
            g += Ai.T @ (c.w_pc * r / den)
        if c.mode == 2:
            lo = o["lin_out"][n]
            lo[:npar * npar], lo[npar * npar:npar * npar + npar] = H.reshape(-1), g
            lo[npar * npar + npar:] = cost, cost_photo, cost_dc, nmask
            continue
        so = o["state"][n]
        lam = float(S["lam"])
        if o["stats"] is not None:
            o["stats"][n, c.it, :4] = np.array([cost, cost_photo, nmask, lam]).astype(np.float32)
            o["stats"][n, c.it, STAT_POSE:] = pose_f32(S["Ttry"])
        final, Tfin, sfin = False, None, 0.0
        if c.mode == 1:
            keep = cost <= S["cost_cur"] if fault == "tie_accept" else cost < S["cost_cur"]
            for k in ("accept_out", "trace_decide"):
                if o[k] is not None:
                    o[k][n] = int(keep)
            Tfin, sfin = (S["Ttry"], S["stry"]) if keep else (S["Tcur"], S["scur"])
            if keep:
                so["Tcur"], so["scur"] = Tfin, sfin
            final = True
        else:
            lower = cost <= S["cost_cur"] if fault == "tie_accept" else cost < S["cost_cur"]
            accept = bool(c.solver == 0 or not S["have_cur"] or lower)
            M8 = np.zeros((8, 8))
            M8[:npar, :npar], M8[:npar, 7] = H, -g
            if accept:
                if c.solver == 1 and S["have_cur"]:
                    lam = lam * c.lam_down if fault == "no_clamp" else max(lam * c.lam_down, c.lam_min)
                so["M8"] = M8.reshape(64)
            else:
                lam = lam * c.lam_up
                if fault == "m8_not_restored":
                    so["M8"] = M8.reshape(64)
                else:
                    old = S["M8"].reshape(8, 8)
                    H, g = old[:npar, :npar].copy(), -old[:npar, 7]
            Tacc, sacc = (S["Ttry"], S["stry"]) if accept else (S["Tcur"], S["scur"])
            if accept:
                so["Tcur"], so["scur"], so["cost_cur"], so["have_cur"] = Tacc, sacc, cost, 1
            so["lam"] = lam
            for k in ("accept_out", "trace_decide"):
                if o[k] is not None:
                    o[k][n] = int(accept)
            if c.param == 0:
                d, ok = _chol_step(H, g, lam, fault)
                E = _exp64(d[:6]).reshape(12)
                Tnew = _mul64(Tacc, E) if fault == "exp_right" else _mul64(E, Tacc)
            else:
                pose = _pose64(Tacc)
                Af = np.eye(npar); Af[:6, :6] = _jac64(pose)
                d, ok = _chol_step(Af.T @ H @ Af, Af.T @ g, lam, fault)
                Tnew = pose_T(pose + d[:6])
                d_out = _chol_step(H, g, lam, fault)[0]
            snew = sacc + (d[6] if npar == 7 else 0.0)
            if o["delta_out"] is not None:
                o["delta_out"][n, :npar] = d if c.param == 0 else d_out
            so["Ttry"], so["stry"] = Tnew, snew
            last_gn = c.solver == 0 and c.it == c.n_iters - 1
            if last_gn:
                so["Tcur"], so["scur"] = Tnew, snew
            if o["pose_lin"] is not None:
                half = (c.it & 1) if fault == "wrong_half" else ((c.it + 1) & 1)
                o["pose_lin"][half][c.pc_self0 + n if c.pc_np > 0 else n] = Tnew
            k = const_of(S["K"], Tnew, snew, npar)
            pc = o["pconst"][n]
            pc["A"], pc["kt"], pc["R"], pc["t"] = k["A"], k["kt"], k["R"], k["t"]
            if npar == 7:
                pc["es"] = k["es"]
            final, Tfin, sfin = last_gn or fault == "pose_nonfinal", Tnew, snew
        if final and o["pose_out"] is not None:
            pose = pose_f32(Tfin)
            if c.c_ncall > 0:
                call, li = coal_index(c.c_ncall, c.c_B, c.c_S, n + c.c_n0)
                o["c_pose_out"][call][li] = pose
                if npar == 7 and o["c_ls_out"][call] is not None:
                    o["c_ls_out"][call][li] = sfin
            else:
                o["pose_out"][n] = pose
                if o["log_scale_out"] is not None:
                    o["log_scale_out"][n] = sfin
            if o["stats"] is not None and c.mode == 0:
                o["stats"][n, c.n_iters, STAT_POSE:] = pose
    return o


_TWIN = {}


def clean_twin(c):
    if c.name not in _TWIN:
        _TWIN[c.name] = twin(c)
    return _TWIN[c.name]


# ---------------------------------------------------------------------------------------------------------------------------- judge
def _f(x):
    return np.array([float(v) for v in x])


def _Emax(got, ex):
    """max |got - exact| with the difference taken at 80 digits (got: float64 array, ex: mpf list)"""
    if not np.all(np.isfinite(got)):
        return math.inf
    return max(float(abs(mpm.mpf(float(a)) - b)) for a, b in zip(np.asarray(got, np.float64).reshape(-1), ex))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all(a.view(np.uint8) == b.view(np.uint8)))


def cond_of(c, n):
    """condition number of the system the launch solves (damped, as solved)"""
    e = exact(c)[n]
    H = np.array([[float(x) for x in row] for row in e.Hs])
    A = H + np.diag(e.lam_out * np.diag(H) + 1e-12)
    return float(np.linalg.cond(A))


def judge_case(c, run, tag=None):
    """-> (failures, measures): run(case) -> outputs of the launch (the GPU, or the twin with a fault)"""
    tag = tag or c.name
    out, tw, ex = run(c), clean_twin(c), exact(c)
    fails, meas = [], dict(ratio_d=0.0, E_d=0.0, ratio_T=0.0, E_T=0.0, sum=0.0, pose=0.0, const=0.0)
    bad = lambda msg: fails.append(f"{tag}: {msg}")
    npar, N = c.np, c.N
    # pairs beyond N: nothing written anywhere
    if not is_sent(out["state"][N:]) or not is_sent(out["pconst"][N:]):
        bad("state / pconst of a pair beyond N written")
    for k in ALL_OUT:
        if out[k] is not None and not is_sent(out[k][N:]):
            bad(f"{k} of a pair beyond N written")
    # what this launch must leave alone
    emits = [ex[n].final for n in range(N)] if c.mode != 2 else [False] * N
    if c.mode == 2:
        for k in ("state", "pconst"):
            if not _eq(out[k], c.state if k == "state" else c.pconst):
                bad(f"mode 2 wrote {k}")
        for k in ("stats", "delta_out", "accept_out", "trace_decide", "pose_out", "log_scale_out"):
            if out[k] is not None and not is_sent(out[k]):
                bad(f"mode 2 wrote {k}")
        if c.pose_lin is not None and not _eq(out["pose_lin"], c.pose_lin):
            bad("mode 2 wrote pose_lin")
    if c.c_ncall > 0:
        want = {}
        for n in range(N):
            if emits[n]:
                want.setdefault(coal_index(c.c_ncall, c.c_B, c.c_S, n + c.c_n0), n)
        if out["pose_out"] is not None and not is_sent(out["pose_out"]):
            bad("a coalesced launch wrote the batch pose_out")
        if out["log_scale_out"] is not None and not is_sent(out["log_scale_out"]):
            bad("a coalesced launch wrote the batch log_scale_out")
        for i in range(c.c_ncall):
            for li in range(c.c_len[i]):
                if (i, li) not in want:
                    if not is_sent(out["c_pose_out"][i][li]) or (out["c_ls_out"][i] is not None and not is_sent(out["c_ls_out"][i][li])):
                        bad(f"per-call output [{i}][{li}] written by no pair of this launch")
    for n in range(N):
        e, S, so = ex[n], c.state[n], out["state"][n]
        t = f"pair {n}: "
        if c.mode == 2:
            lo, tl = out["lin_out"][n], tw["lin_out"][n]
            k2 = npar * npar
            u = (c.ngrp + 4) * 2.0 ** -53
            items = [("H", lo[:k2], [x for row in e.H for x in row], e.bH.reshape(-1)), ("g", lo[k2:k2 + npar], e.g, e.bg),
                     ("cost", lo[k2 + npar:k2 + npar + 1], [e.cost], [e.bcost]), ("cost_photo", lo[k2 + npar + 1:k2 + npar + 2], [e.cost_photo], [e.bphoto]),
                     ("cost_dc", lo[k2 + npar + 2:k2 + npar + 3], [e.cost_dc], [e.bdc])]
            for name, got, exv, bnd in items:
                for i, (a, b, bb) in enumerate(zip(got, exv, bnd)):
                    err = abs(F(float(a)) - b) if np.isfinite(a) else math.inf
                    if bb > 0 and err != math.inf:
                        meas["sum"] = max(meas["sum"], float(err) / (u * bb))
                    if not err <= u * bb:
                        bad(t + f"{name}[{i}] off by {float(err):.3e}, bound {u * bb:.3e}")
                        break
            if F(float(lo[k2 + npar + 3])) != e.nmask:
                bad(t + f"n_mask {lo[k2 + npar + 3]} is not {float(e.nmask)}")
            continue
        # decisions
        for k in ("accept_out", "trace_decide"):
            if out[k] is not None and int(out[k][n]) != int(e.decide):
                bad(t + f"{k} = {int(out[k][n])}, exact decision {int(e.decide)}")
        st_rows = out["stats"][n] if out["stats"] is not None else None
        if st_rows is not None:
            for i in range(c.n_iters + 1):
                if i == c.it:
                    continue
                if i == c.n_iters and c.mode == 0 and e.final:
                    if not is_sent(st_rows[i, :STAT_POSE]):
                        bad(t + "cost fields of the final stats row written")
                elif not is_sent(st_rows[i]):
                    bad(t + f"stats row {i} written by launch {c.it}")
            sp_ex = mp_pose_of_T([mpm.mpf(float(x)) for x in S["Ttry"]])
            _judge_pose(bad, meas, t + "stats pose", st_rows[c.it, STAT_POSE:], sp_ex, pose_f32(S["Ttry"]))
            if st_rows[c.it, 2] != np.float32(float(e.nmask)) or st_rows[c.it, 3] != np.float32(S["lam"]):
                bad(t + "stats n_mask / lambda")
            if abs(float(st_rows[c.it, 0]) - float(e.cost)) > 2.0 ** -23 * max(1.0, abs(float(e.cost))):
                bad(t + "stats cost")
            if abs(float(st_rows[c.it, 1]) - float(e.cost_photo)) > 2.0 ** -23 * max(1.0, abs(float(e.cost_photo))):
                bad(t + "stats cost_photo")
        if c.mode == 1:
            keep = e.decide
            same = ["Ttry", "stry", "s0", "lam", "cost_cur", "M8", "K", "have_cur", "pad"] + ([] if keep else ["Tcur", "scur"])
            for k in same:
                if not _eq(so[k], S[k]):
                    bad(t + f"mode 1 changed {k}")
            if keep and not (_eq(so["Tcur"], S["Ttry"]) and _eq(so["scur"], S["stry"])):
                bad(t + "mode 1 kept the step but Tcur / scur are not the trial's")
            if not _eq(out["pconst"][n], c.pconst[n]):
                bad(t + "mode 1 wrote pconst")
            if out["delta_out"] is not None and not is_sent(out["delta_out"][n]):
                bad(t + "mode 1 wrote delta_out")
        else:
            acc = e.decide
            last_gn = c.solver == 0 and c.it == c.n_iters - 1
            if so["lam"] != e.lam_out or math.copysign(1, so["lam"]) != math.copysign(1, e.lam_out):
                bad(t + f"lambda {so['lam']!r} is not {e.lam_out!r}")
            if so["have_cur"] != (1 if acc else S["have_cur"]) or so["pad"] != S["pad"] or not _eq(so["K"], S["K"]) or not _eq(so["s0"], S["s0"]):
                bad(t + "have_cur / K / s0")
            if acc:
                if not last_gn and not (_eq(so["Tcur"], S["Ttry"]) and _eq(so["scur"], S["stry"])):
                    bad(t + "accepted, but Tcur / scur are not the incoming trial")
                if st_rows is not None and np.float32(so["cost_cur"]) != st_rows[c.it, 0]:
                    bad(t + "cost_cur is not the stats row's cost")
                if abs(so["cost_cur"] - float(e.cost)) > 64 * 2.0 ** -53 * max(abs(float(e.cost)), 1e-300) + (c.ngrp + 4) * 2.0 ** -53 * e.bcost:
                    bad(t + "cost_cur")
            else:
                for k in ("M8", "Tcur", "scur", "cost_cur"):
                    if not _eq(so[k], S[k]):
                        bad(t + f"rejected, but {k} changed")
            if last_gn and not (_eq(so["Tcur"], so["Ttry"]) and _eq(so["scur"], so["stry"])):
                bad(t + "last Gauss-Newton launch: Tcur / scur are not the new iterate")
            # step and new trial transform
            if out["delta_out"] is not None:
                dgot = out["delta_out"][n]
                if not is_sent(dgot[npar:]):
                    bad(t + "delta_out beyond np written")
                dex = getattr(e, "d_out", e.d)
                Ek, Et = _Emax(dgot[:npar], dex), _Emax(tw["delta_out"][n][:npar], dex)
                floor = 8 * 2.0 ** -52 * max(float(abs(x)) for x in dex)
                if not e.ok and np.any(dgot[:npar] != 0):
                    bad(t + "a non-positive pivot must give a zero step")
                meas["ratio_d"], meas["E_d"] = max(meas["ratio_d"], Ek / Et if Et > 0 else (0.0 if Ek <= floor else math.inf)), max(meas["E_d"], Ek)
                if c.judged:
                    if not Ek <= 4 * Et + floor:
                        bad(t + f"step: E {Ek:.3e} > 4 x {Et:.3e} + {floor:.3e}")
            Ek, Et = _Emax(so["Ttry"], e.Tnew), _Emax(tw["state"][n]["Ttry"], e.Tnew)
            floor = 8 * 2.0 ** -52 * max(float(abs(x)) for x in e.Tnew)
            meas["ratio_T"], meas["E_T"] = max(meas["ratio_T"], Ek / Et if Et > 0 else (0.0 if Ek <= floor else math.inf)), max(meas["E_T"], Ek)
            if c.judged:
                if not Ek <= 4 * Et + floor:
                    bad(t + f"trial transform: E {Ek:.3e} > 4 x {Et:.3e} + {floor:.3e}")
                Es = abs(float(mpm.mpf(float(so["stry"])) - e.snew)) if np.isfinite(so["stry"]) else math.inf
                Ets = abs(float(mpm.mpf(float(tw["state"][n]["stry"])) - e.snew))
                if not Es <= 4 * Ets + 8 * 2.0 ** -52 * max(abs(float(e.snew)), 2.0 ** -60):
                    bad(t + f"trial log scale: E {Es:.3e} > 4 x {Ets:.3e}")
            if npar == 6 and not _eq(so["stry"], S["stry"] if acc else S["scur"]):
                bad(t + "6 unknowns: stry is not the accepted scale")
            if e.ok and all(x == 0 for x in e.d) and not (_eq(so["Ttry"], S["Ttry"] if acc else S["Tcur"])):
                bad(t + "zero step, but the trial transform is not the accepted one")
            if not e.ok and not (_eq(so["Ttry"], S["Ttry"] if acc else S["Tcur"])):
                bad(t + "zero step (pivot), but the trial transform is not the accepted one")
            if c.judged:
                _judge_const(bad, meas, t, c, out["pconst"][n], c.pconst[n], S["K"], [_frac(x) for x in e.Tnew], e.snew)
            else:       # (beyond the judged range the transform itself is not held to exact: the constants as a function of what was written)
                _judge_const(bad, meas, t, c, out["pconst"][n], c.pconst[n], S["K"], [F(float(x)) for x in so["Ttry"]], mpm.mpf(float(so["stry"])))
            if c.pose_lin is not None:
                me = c.pc_self0 + n if c.pc_np > 0 else n
                if not _eq(out["pose_lin"][(c.it + 1) & 1][me], so["Ttry"]):
                    bad(t + "pose_lin's next half is not the new trial transform")
        # the emitted pose
        slot = None
        if out["pose_out"] is not None:
            if c.c_ncall > 0:
                call, li = coal_index(c.c_ncall, c.c_B, c.c_S, n + c.c_n0)
                slot = (out["c_pose_out"][call][li], None if out["c_ls_out"][call] is None else out["c_ls_out"][call][li:li + 1])
            else:
                slot = (out["pose_out"][n], None if out["log_scale_out"] is None else out["log_scale_out"][n:n + 1])
        if slot is not None:
            if not e.final:
                if c.c_ncall == 0 and (not is_sent(slot[0]) or (slot[1] is not None and not is_sent(slot[1]))):
                    bad(t + "pose_out / log_scale_out written by a launch that is not the last")
            else:
                Tk = so["Ttry"] if c.mode == 0 else (S["Ttry"] if e.decide else S["Tcur"])
                _judge_pose(bad, meas, t + "pose_out", slot[0], mp_pose_of_T(e.Tfin), pose_f32(Tk))
                if st_rows is not None and c.mode == 0 and not _eq(st_rows[c.n_iters, STAT_POSE:], slot[0]):
                    bad(t + "final stats row's pose is not pose_out")
                if slot[1] is not None:
                    if npar == 6 and c.c_ncall > 0:
                        if not is_sent(slot[1]):
                            bad(t + "6 unknowns: a per-call log scale written")
                    elif not abs(float(slot[1][0]) - float(e.sfin)) <= 2.0 ** -23 * max(1.0, abs(float(e.sfin))):
                        bad(t + f"log_scale_out {slot[1][0]} vs {float(e.sfin)}")
    if c.pose_lin is not None and c.mode != 2:
        per = c.pc_np if c.pc_np > 0 else c.n_pairs
        mine = {(c.pc_self0 + n if c.pc_np > 0 else n) for n in range(N)}
        if not _eq(out["pose_lin"][c.it & 1], c.pose_lin[c.it & 1]):
            bad("the pose_lin half this launch reads was written")
        for m in range(per):
            if m not in mine and not _eq(out["pose_lin"][(c.it + 1) & 1][m], c.pose_lin[(c.it + 1) & 1][m]):
                bad(f"pose_lin slot {m} of no pair of this launch written")
    return fails, meas


def _judge_pose(bad, meas, t, got, ex, tw32):
    exf = np.array([float(x) for x in ex])
    Et = float(np.max(np.abs(tw32.astype(np.float64) - exf)))
    bound = 4 * Et + 2.0 ** -23 * max(1.0, float(np.max(np.abs(exf))))
    Ek = float(np.max(np.abs(got.astype(np.float64) - exf))) if np.all(np.isfinite(got)) else math.inf
    meas["pose"] = max(meas["pose"], Ek / bound)
    if not Ek <= bound:
        bad(t + f": E {Ek:.3e} > bound {bound:.3e}")


def _judge_const(bad, meas, t, c, pc, pc_in, K, T, s):
    """A, kt, R, t within 1 ulp32 (es: 2) of the exact value rounded to fp32; T (12 Fractions), s (mpf): the exact new trial transform and scale"""
    for k in ("fx", "fy", "cx", "cy", "ki0", "ki2", "ki4", "ki5", "img", "pad"):
        if not _eq(pc[k], pc_in[k]):
            bad(t + f"pconst.{k} changed")
    Kf = [[F(float(K[3 * i + j])) for j in range(3)] for i in range(3)]
    Tf = [[T[4 * i + j] for j in range(4)] for i in range(3)]
    ifx, ify = 1 / Kf[0][0], 1 / Kf[1][1]
    Ki = [[ifx, F(0), -Kf[0][2] * ifx], [F(0), ify, -Kf[1][2] * ify], [F(0), F(0), F(1)]]
    RI = [[Tf[i][j] - (1 if i == j else 0) for j in range(3)] for i in range(3)]
    want = {}
    for i in range(3):
        for j in range(3):
            want[("A", 3 * i + j)] = sum(Kf[i][a] * RI[a][b] * Ki[b][j] for a in range(3) for b in range(3))
            want[("R", 3 * i + j)] = Tf[i][j]
        want[("kt", i)] = sum(Kf[i][a] * Tf[a][3] for a in range(3))
        want[("t", i)] = Tf[i][3]
    for (k, i), v in want.items():
        r32 = np.float32(float(v))
        tol = _ulp32(r32)
        err = abs(float(pc[k][i]) - float(r32)) if np.isfinite(pc[k][i]) else math.inf
        meas["const"] = max(meas["const"], err / tol)
        if not err <= tol:
            bad(t + f"pconst.{k}[{i}] = {pc[k][i]!r}, exact {r32!r}")
    if c.np == 7:
        es = np.float32(float(mpm.exp(s)))
        if not abs(float(pc["es"]) - float(es)) <= 2 * _ulp32(es):
            bad(t + f"pconst.es = {pc['es']!r}, exact {es!r}")
    elif not _eq(pc["es"], pc_in["es"]):
        bad(t + "6 unknowns: pconst.es changed")


# public names of the helpers tests/joint_solve_exact_inputs.py shares with this module
exact_sum, mpf, frac, euler_left_jacobian, damped_step, pivots_positive = _exact_sum, _mpf, _frac, _euler_left_jacobian, _damped_step, _pivots_positive
pose64, exp64, mul64, jac64, Emax, eq, judge_pose, judge_const = _pose64, _exp64, _mul64, _jac64, _Emax, _eq, _judge_pose, _judge_const


# ----------------------------------------------------------------------------------------------------------------------- case lists
def _allowed(variant, npar, w_pc=0.0, param=0):
    return not ((variant >= 1 and param != 0) or (variant in (1, 2) and w_pc > 0) or (variant >= 2 and npar == 7) or (w_pc > 0 and npar == 7))


def sweep_cases():
    out = []
    for variant in range(4):
        for npar in (6, 7):
            for dc in (0, 1):
                if not _allowed(variant, npar):
                    continue
                for ngrp in sweep_ngrp(variant, npar, bool(dc)):
                    out.append(case(f"sweep v{variant} np{npar} dc{dc} ngrp{ngrp}", f"sweep v{variant} np{npar} dc{dc}", variant=variant, npar=npar,
                                    w_dc=0.15 * dc, mode=2, N=3, ngrp=ngrp, seed=ngrp + 7 * dc, prior_scale=1.0, want=("lin_out", "stats", "pose_out"),
                                    claims=("sweep",)))
    return out


def _diag_records(npar, hdiag, gvec, count=64.0, ngrp=5, cost=None):
    """records whose totals are H = diag(hdiag), g = gvec and cost_photo = cost, exactly in any arithmetic when the entries are dyadic (the
    count is a power of two): record 0 carries the system and the count, every record a share of the cost"""
    L = layout(npar)
    rec = np.full((2, ngrp, L.NACC), np.nan, np.float32)
    rec[0, :, :L.NH + npar] = 0
    rec[0, :, L.S:] = 0
    for i in range(npar):
        rec[0, 0, L.HP + _tri(npar, i, i)] = hdiag[i] * count
        rec[0, 0, L.GP + i] = gvec[i] * count
    rec[0, 0, L.S + 1] = count
    rec[0, :, L.S] = (1.0 if cost is None else cost) * count / ngrp
    return rec


def _spd_records(seed, npar, conds, ngrp=8, count=64.0, colscale=None):
    """records whose total is H = sum_k 2^-e_k v_k v_k', g = H x0 with small INTEGER vectors v_k (independent, nearly orthogonal), x0 and
    e_k spread over log2(conds): one rank-one term per record, so float32 holds every record exactly and H is positive definite with
    the intended spread whatever the rounding (a float32 copy of a dense ill-conditioned H would be indefinite from 1e7 on).  colscale:
    integer scales of the unknowns (translation : rotation)"""
    L = layout(npar)
    assert ngrp >= npar
    rng = np.random.default_rng(seed)
    cs = np.ones(npar) if colscale is None else np.asarray(colscale, float)
    V = (4 * np.eye(npar) + rng.integers(-1, 2, size=(npar, npar))) * cs[None, :]
    x0 = rng.integers(-3, 4, size=npar) / (64.0 * cs)
    ex = np.round(np.arange(npar) * math.log2(conds) / (npar - 1))
    if colscale is not None:
        ex = ex[::-1]               # (the large unknowns carry the large weights: scales and spread add up)
    rec = np.full((2, ngrp, L.NACC), np.nan, np.float32)
    rec[0, :, :L.NH + npar] = 0
    for k in range(npar):
        Hk = np.outer(V[k], V[k]) * 2.0 ** -ex[k] * count
        gk = Hk @ x0
        for i in range(npar):
            for j in range(i + 1):
                rec[0, k, L.HP + _tri(npar, i, j)] = Hk[i, j]
            rec[0, k, L.GP + i] = gk[i]
        assert np.array_equal(rec[0, k, :L.NH].astype(np.float64), np.array([Hk[i, j] for i in range(npar) for j in range(i + 1)]))
    rec[0, :, L.S], rec[0, :, L.S + 1], rec[0, :, L.S + 2] = 1.5, 0, 0.25
    rec[0, 0, L.S + 1] = count
    return rec


X_LO = 0.3
while np.nextafter(X_LO, 1) * np.nextafter(X_LO, 1) < 0.09:
    X_LO = float(np.nextafter(X_LO, 1))
while X_LO * X_LO >= 0.09:
    X_LO = float(np.nextafter(X_LO, 0))
X_HI = float(np.nextafter(X_LO, 1))          # fl(X_LO^2) < 0.09 <= fl(X_HI^2): the two steps either side of se3_exp's switch


def path_cases():
    out = []
    lm = dict(solver=1, lam_up=10.0, lam_down=0.1, lam_min=1e-5)
    for npar in (6, 7):
        ps = dict(prior_scale=1.0, s=(0.02, 0.05, 0.01)) if npar == 7 else {}
        tagp = f"np{npar}"
        for it in (0, 2, 3):
            out.append(case(f"gn it{it} {tagp}", f"solver paths {tagp}", npar=npar, it=it, N=2, seed=it, lam=1e-4, claims=("gn_final",) if it == 3 else (), **ps))
        out.append(case(f"lm first {tagp}", f"solver paths {tagp}", npar=npar, seed=11, lam=1e-4, have_cur=0, cost_cur=-5.0, claims=("accept", "lam_same"), **lm, **ps))
        out.append(case(f"lm accept {tagp}", f"solver paths {tagp}", npar=npar, seed=12, lam=1e-2, have_cur=1, cost_cur=1e3, it=1,
                        claims=("accept", "lam_down"), **lm, **ps))
        out.append(case(f"lm accept clamp {tagp}", f"solver paths {tagp}", npar=npar, seed=13, lam=3e-5, have_cur=1, cost_cur=1e3, it=1,
                        claims=("accept", "lam_clamped"), **lm, **ps))
        out.append(case(f"lm reject {tagp}", f"solver paths {tagp}", npar=npar, seed=14, lam=1e-3, have_cur=1, cost_cur=-1.0, it=2, claims=("reject",), **lm, **ps))
        out.append(case(f"lm mode1 kept {tagp}", f"solver paths {tagp}", npar=npar, seed=15, mode=1, it=4, have_cur=1, cost_cur=1e3, claims=("accept",), **lm, **ps))
        out.append(case(f"lm mode1 not kept {tagp}", f"solver paths {tagp}", npar=npar, seed=16, mode=1, it=4, have_cur=1, cost_cur=-1.0, claims=("reject",), **lm, **ps))
        # exact tie: dyadic records, the cost is 1.25 in any arithmetic
        tie = _diag_records(npar, [1.0] * npar, [0.125] * npar, cost=1.25)
        out.append(case(f"lm tie mode0 {tagp}", f"solver paths {tagp}", npar=npar, rec=tie, have_cur=1, cost_cur=1.25, lam=1e-3, it=1, claims=("tie", "reject"), **lm))
        out.append(case(f"lm tie mode1 {tagp}", f"solver paths {tagp}", npar=npar, rec=tie, have_cur=1, cost_cur=1.25, mode=1, it=4, claims=("tie", "reject"), **lm))
        if npar == 7:
            out.append(case("np7 prior 0 accept", "solver paths np7", npar=7, seed=17, lam=1e-2, have_cur=1, cost_cur=1e3, it=1, prior_scale=0.0,
                            s=(0.02, 0.05, 0.01), claims=("accept",), **lm))
        z = _diag_records(npar, [1.0] * npar, [0.125] * npar)
        z[0, :, layout(npar).S + 1] = 0
        out.append(case(f"nmask 0 {tagp}", f"solver paths {tagp}", npar=npar, rec=z, lam=1e-4, claims=("nmask0", "zero_step") if npar == 6 else ("nmask0",), **ps))
        z = _diag_records(npar, [0.0] * npar, [0.0] * npar)
        z[0, :, layout(npar).S:] = 0
        out.append(case(f"all zero {tagp}", f"solver paths {tagp}", npar=npar, rec=z, lam=1e-4, claims=("zero_step",) if npar == 6 else ()))
        h = [1.0] * npar; h[2] = -0.5
        out.append(case(f"negative pivot {tagp}", f"solver paths {tagp}", npar=npar, rec=_diag_records(npar, h, [0.125] * npar), lam=1e-4, have_cur=1,
                        cost_cur=1e3, it=1, claims=("bad_pivot", "accept"), **lm))
        cs = [1, 1, 1, 128, 128, 128] + ([1] if npar == 7 else [])         # column scales 1 : 2^7 -> H entries 1 : 1.6e4, as translation : rotation
        for cond in (1.0, 1e2, 1e4, 1e6, 1e8):
            out.append(case(f"cond {cond:.0e} {tagp}", f"conditioning {tagp}", npar=npar, rec=_spd_records(int(math.log10(cond)) + 3, npar, cond), lam=0.0,
                            claims=(("cond", cond),)))
            if cond <= 1e4:           # (the scales multiply the condition number by 2^14)
                out.append(case(f"cond {cond:.0e} scaled {tagp}", f"conditioning {tagp}", npar=npar, rec=_spd_records(int(math.log10(cond)) + 30, npar, cond, colscale=cs),
                                lam=0.0, claims=(("cond_scaled", cond * 2.0 ** 14),)))
        out.append(case(f"cond 1e13 {tagp} (printed)", f"beyond the judged range {tagp}", npar=npar, rec=_spd_records(99, npar, 1e13), lam=0.0, judged=False,
                        claims=(("cond_beyond", 1e13),)))
        out.append(case(f"euler gn {tagp}", f"additive Euler {tagp}", npar=npar, param=1, seed=21, it=3, lam=1e-4, claims=("gn_final",), **ps))
        out.append(case(f"euler lm reject {tagp}", f"additive Euler {tagp}", npar=npar, param=1, seed=22, lam=1e-3, have_cur=1, cost_cur=-1.0, it=1, claims=("reject",), **lm, **ps))
    out.append(case("np7 scale step", "solver paths np7", npar=7, seed=23, prior_scale=0.5, s=(0.1, -0.2, 0.3), lam=1e-4, it=3, claims=("gn_final", "scale_step")))
    return out


def retraction_cases():
    """the step is set through the reject path: the stored system M8 = [2^40 I | 2^40 x] is solved exactly (lambda 0), so d = x to the bit"""
    out = []
    big = 2.0 ** 40
    steps = [("rot 0", [0.01, -0.02, 0.03, 0, 0, 0], "series"), ("rot 1e-9", [0.01, 0, 0, 0, 1e-9, 0], "series"), ("rot 0.29", [0, 0.02, 0, 0.29 * 0.6, 0, 0.29 * 0.8], "series"),
             ("t2 below 0.09", [0.01, 0.02, 0.03, 0, 0, X_LO], "series"), ("t2 at 0.09", [0.01, 0.02, 0.03, 0, 0, X_HI], "trig"),
             ("rot 1.0", [0.05, 0, 0, 0.6, 0.8, 0], "trig"), ("rot 3.0", [0, 0.05, 0, 1.0, 2.0, 2.0], "trig"), ("pure translation", [0.25, -0.5, 0.125, 0, 0, 0], "series")]
    for name, x, branch in steps:
        c = case(f"retract {name}", "retraction", solver=1, lam=0.0, have_cur=1, cost_cur=-1.0, it=1, seed=31, claims=("reject", ("branch", branch), ("step", tuple(x))))
        M8 = np.zeros((8, 8))
        M8[:6, :6] = np.eye(6) * big
        M8[:6, 7] = np.array(x) * big
        c.state[0]["M8"] = M8.reshape(64)
        out.append(c)
    # the same steps through the accept path of the last Gauss-Newton launch (records), which also emits the pose
    for name, x, branch in steps[2:3] + steps[5:]:
        rec = _diag_records(6, [1.0] * 6, [-v for v in x])
        out.append(case(f"retract gn {name}", "retraction", rec=rec, lam=0.0, it=3, claims=("gn_final", ("branch", branch))))
    return out


def extraction_cases():
    out = []
    for name, sb in (("sin 1 - 5e-8", 1 - 5e-8), ("sin -(1 - 5e-8)", -(1 - 5e-8)), ("sin 1 + ulp", float(np.nextafter(1.0, 2)))):
        c = case(f"extract {name}", "pose extraction", solver=1, mode=1, it=4, have_cur=1, cost_cur=1e3, seed=41, claims=("accept", ("sin", sb)))
        ry = -math.asin(max(-1.0, min(1.0, sb)))
        T = pose_T([0.1, -0.2, 0.3, 0.2, ry, -0.1])
        T[2] = sb
        c.state[0]["Ttry"] = T
        out.append(c)
    return out


def rule_cases():
    out = []
    for nm in (0, 1):
        for scale in (1.0, 0.25):
            c = case(f"rule norms{nm} scale {scale}", "window rule", N=4, seed=51, it=1, lam=1e-4, rule=1, grp_fwd=2, n_pairs=4, scale_fwd=scale, scale_inv=0.25)
            if nm:
                c.norms, c.norm_Bt, c.norm_B = np.array([[321, 123], [77, 0]], np.int32), 2, 1      # pair 3 (inverse, target 1): a group whose count is 0
            out.append(c)
            out.append(clone(c, name=c.name + " export", mode=2))
    c = case("rule empty forward group", "window rule", N=4, seed=52, it=1, lam=1e-4, rule=1, grp_fwd=2, n_pairs=4, scale_inv=0.25, claims=("group0",))
    c.rec[:2, :, layout(6).S + 1] = 0
    out.append(c)
    return out


def pc_cases():
    out = []
    for variant in (0, 3):
        for it in (1, 2):
            rng = np.random.default_rng(60 + it)
            pl = np.stack([np.stack([pose_T(rng.normal(scale=[0.05, 0.05, 0.05, 0.2, 0.2, 0.2])) for _ in range(4)]) for _ in range(2)])
            c = case(f"pc v{variant} unsliced it{it}", f"pose consistency v{variant}", variant=variant, N=4, seed=61, it=it, lam=1e-4, rule=1, grp_fwd=2, n_pairs=4,
                     scale_inv=0.25, w_pc=0.1 / 12, pc_eps=1e-3, pose_lin=pl, claims=("pc",))
            # pair 0: its partner (pair 2) is almost its negative pose: residual components below pc_eps
            p0 = np.array([0.03, -0.02, 0.01, 0.1, -0.05, 0.2])
            c.state[0]["Ttry"] = pose_T(p0)
            c.pose_lin[it & 1][2] = pose_T(-p0 + np.array([2e-4, -3e-4, 1e-4, 0.05, 2e-4, -0.1]))
            out.append(c)
            pls = np.concatenate([pl, pl[:, ::-1]], axis=1)[:, :7]
            d = case(f"pc v{variant} slice it{it}", f"pose consistency v{variant}", variant=variant, N=2, seed=62, it=it, lam=1e-4, rule=1, grp_fwd=0, n_pairs=2,
                     scale_inv=0.25, norms=np.array([[50, 60]], np.int32), w_pc=0.1 / 12, pc_eps=1e-3, pose_lin=pls, pc_np=7, pc_self0=4, pc_part0=1,
                     claims=("pc",))
            out.append(d)
    return out


def coal_cases():
    out = []
    for n0 in (0, 2):
        for npar in (6, 7):
            ps = dict(prior_scale=1.0, s=(0.02, 0.05, 0.01)) if npar == 7 else {}
            out.append(case(f"coalesced n0 {n0} np{npar}", "coalesced routing", npar=npar, N=2, seed=71, it=3, lam=1e-4, c_ncall=2, c_B=1, c_S=1, c_n0=n0,
                            c_len=(2, 2), c_ls=(True, False), claims=("gn_final",), **ps))
    return out


def lean_cases(base):
    """the bookkeeping, solve and retraction of the 1024-thread instantiations: a few of k_solve's cases on variants 1 to 3"""
    b = {c.name: c for c in base}
    out = []
    for variant in (1, 2, 3):
        for tagp in ("np6", "np7"):
            if not _allowed(variant, int(tagp[2])):
                continue
            for nm in (f"gn it0 {tagp}", f"gn it3 {tagp}", f"lm accept {tagp}", f"lm accept clamp {tagp}", f"lm reject {tagp}", f"lm mode1 kept {tagp}",
                       f"lm tie mode0 {tagp}", f"negative pivot {tagp}", f"cond 1e+06 {tagp}"):
                out.append(clone(b[nm], name=f"{nm} v{variant}", group=f"solver paths v{variant} {tagp}", variant=variant))
        for nm in ("retract t2 below 0.09", "retract t2 at 0.09", "retract rot 3.0", "coalesced n0 2 np6", "rule norms1 scale 0.25"):
            out.append(clone(b[nm], name=f"{nm} v{variant}", group=f"solver paths v{variant} np6", variant=variant))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = sweep_cases() + path_cases() + retraction_cases() + extraction_cases() + rule_cases() + pc_cases() + coal_cases()
    cs = cs + lean_cases(cs)
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def by_name():
    return {c.name: c for c in all_cases()}


def check_m8_export(c, run, out=None):
    """M8 of an accepting launch is the mode-2 export of the same records, bit for bit (6 unknowns; 7 with prior_scale = 0)"""
    out = out or run(c)
    exp = run(clone(c, name=c.name + "/export", mode=2))
    fails, k2 = [], c.np * c.np
    for n in range(c.N):
        M8 = out["state"][n]["M8"].reshape(8, 8)
        if not (_eq(M8[:c.np, :c.np], exp["lin_out"][n][:k2].reshape(c.np, c.np)) and _eq(-M8[:c.np, 7], exp["lin_out"][n][k2:k2 + c.np])):
            fails.append(f"{c.name}: pair {n}: M8 is not the mode-2 export")
    return fails


def check_alone(c, run, n=1):
    """item n of the launch is the same pair launched alone, bit for bit (mode 2 export)"""
    a, b = run(c), run(alone(c, n))
    return [] if _eq(a["lin_out"][n], b["lin_out"][0]) else [f"{c.name}: pair {n} differs from the pair launched alone"]


def report_line(c, meas, nfail):
    return (f"{c.name:44s} | {c.group:30s} | judged {int(c.judged)} fails {nfail} | d x{meas['ratio_d']:.2f} E {meas['E_d']:.2e} | T x{meas['ratio_T']:.2f} E {meas['E_T']:.2e} | "
            f"sum {meas['sum']:.3f} pose {meas['pose']:.3f} const {meas['const']:.3f}")


# the launches tcsfm_debug_solve must refuse: (name, case, words of the message of the check that must be the one to fire)
def refusal_cases():
    b = by_name()
    gn, pc, co = b["gn it0 np6"], b["pc v0 unsliced it1"], b["coalesced n0 0 np6"]
    ru = b["rule norms1 scale 1.0"]
    return [("N 0", clone(gn, N=0), "at least 1"), ("ngrp 0", clone(gn, ngrp=0), "at least 1"), ("grp_fwd > n_pairs", clone(ru, grp_fwd=5), "grp_fwd <= n_pairs"),
            ("rule n_pairs != N", clone(ru, n_pairs=3, grp_fwd=2), "window rule"), ("unsliced pc n_pairs != N", clone(pc, rule=0, n_pairs=5), "unsliced"),
            ("partner outside", clone(pc, grp_fwd=3), "partner index"), ("slice partner outside", clone(b["pc v0 slice it1"], pc_part0=6), "partner index"),
            ("norms short", clone(ru, norms=ru.norms[:1].copy()), "norms is shorter"), ("it > n_iters", clone(gn, it=5), "it <= n_iters"),
            ("coal outside", clone(co, c_len=(2, 0)), "per-call arrays"), ("coal n0 outside", clone(co, c_n0=3), "per-call arrays"),
            ("lean euler", clone(b["euler gn np6"], variant=1), "SE(3) chart only"), ("front euler", clone(b["euler gn np6"], variant=2), "SE(3) chart only"),
            ("lean pc", clone(pc, variant=1), "no pose-consistency term"), ("front pc", clone(pc, variant=2), "no pose-consistency term"),
            ("front np7", clone(b["gn it0 np7"], variant=3), "6-DoF pairs only"), ("pc np7", clone(pc, np=7), "term is 6-DoF only"),
            ("mode 2 no lin_out", clone(gn, mode=2, want=("stats",)), "needs lin_out")]


def wants_m8_export(c):
    """accepting iteration steps whose stored system is the raw export: 6 unknowns, or 7 without the scale prior"""
    return c.mode == 0 and (c.np == 6 or c.prior_scale == 0) and all(e.decide for e in exact(c))
