"""Cases, metric and judge of the pixel-by-pixel check of ONE linearisation of the dense mode on the reference's loss
(tcsfm_linearize_dense_window / _sources: k_linearize<FRONT> -> k_dense_joint -> [k_dref_smooth] -> k_solve / k_solve_joint -> k_dref_export_grho
[-> k_dref_scatter_src -> k_dense_joint<1> -> k_dref_export_grho_src]), shared by tests/test_dense_linearize_exact_inputs_cpu.py and
tests/test_gpu_dense_linearize_exact.py.  No GPU here (run_engine is the only function that touches one, and it imports torch itself).

WHY.  The five places that look at this export (test_gpu_dense_reference.py, test_gpu_four_sources.py, the sub-tile cases of
test_gpu_dense_shapes.py, test_gpu_options.py, test_gpu_fd.py) compare g_pose, g_rho and g_rho_src with the float64 oracle to 2e-4 of their
LARGEST entry, because they do not pin the discrete decisions.  g_rho and g_rho_src are per-pixel maps: a pixel whose gradient is entirely
wrong but small passes that bar -- a tile-edge pixel that misses a halo tap of the SSIM adjoint, a pixel that receives only the inverse
pairs' scattered adjoint, the depth-consistency and prior parts wherever the photometric part dominates.  Here the engine's decisions are
recorded (tcsfm_debug_trace, honoured by the export) and replayed in the oracle (Oracle.linearize_dense_ref(bits=...)), so that what is
left is continuous arithmetic, and every pixel and every pose entry is held to the accuracy of an fp32 evaluation of ITS OWN sum.

METRIC, engine against float64 under the engine's own bits (g_*_abs64: beside every entry the oracle's sum over the entry's contributions
of |contribution| -- per source, channel, SSIM-window tap (x and y parts apart), scattered bilinear tap, the weight, depth-consistency,
prior and smoothness terms; the inverse pairs' pose rows per pixel, as Oracle.linearize's gabs):
    E_rho    = max over the pixels of |g_rho - g_rho64| / g_rho_abs64      per target map (also reported: the 99th percentile)
    E_rho_s  = the same per source map (g_rho_src against g_rho_s64 / g_rho_s_abs64)
    E_xi     = max_j |g_pose - g_xi64|_j / g_xi_abs64_j                    per directed pair
    E_fwd, E_inv_photo, E_inv_dc = relative error of scal_out's non-negative terms (forward group = L_fwd + the forward pairs' share of
               L_dc + L_init of the oracle; the inverse pairs' photometric and depth-consistency sums)
    K_f, K_i exact, and equal to the population count of bit 0 of the forward / inverse trace planes (the export exposes the two SUMS over
               the call, not a count per pair: per-pair counts cannot be judged here);
    a pixel whose g_rho_abs64 (g_rho_s_abs64) is zero must be exactly zero in the engine's output.
BOUND.  E <= MARGIN * E(float32 oracle, same inputs, same bits) + A, MARGIN = 4 (the project's two bits); a measure in which the float32
twin is exact keeps A alone.  The float32 oracle computes every term in float but ADDS in double; the kernels add in fp32, and the scatter
adds in fixed point.  A pays for that and for nothing else:  A = D 2^-24 + F.
  D = the number of fp32 additions on the longest path from a term to the first double-precision (or fixed-point) sum, read off the kernels:
    g_rho (additions_rho; dense_joint_body, joint_kernel.h).  An SSIM tap's coefficient enters sA/sB/sC in `gather`, nine taps summed from 0:
        8                  gather: sA[ch] += fm c (the first addition to 0 is exact)
      + 2                  lam = sA + sB yq + sC xq
      + 3                  sx = o_w o_l1x; sx += lam o_gx[ch] for three channels
      + 2                  grow[6] = sx a[6] + sy bb[6] - kdd ddJ[6]        (one addition, one subtraction)
      + 2 S                g_rho += grow[6]; g_rho += inf ddJ[6] for every source behind it (source 0's term passes all of them)
      + 1 + 1              the prior (g_rho += r_init sig_ir pl) and the smoothness term (g_rho += ...), where compiled in: counted always
      + 1                  g_rho -= depth^2 (r_dc Edc - r_eph Eph): the scattered sums
      + 1                  k_dref_export_grho: (float)(a_f (double) jrec): the one rounding of the output
      = 19 + 2 S;   g_rho_src is the same kernel at S = 1 on the inverse pairs without prior and smoothness (counted all the same: 21) and
      k_dref_export_grho_src's fp32 product.
    forward pairs' g_pose (additions_xi): grow[j] as above up to the source's own depth-consistency term: 8 + 2 + 3 + 2 + 1 = 16;
      + 6                  wave butterfly (wave_reduce_store, joint_reduce_add)
      + 3                  the four wave partials of a 256-thread workgroup, in order from 0
      + S                  acc[OFF_G + .] += : the source's own sum, the cross terms of the other sources (source 0) and the Schur term
                           -B g_rho / ((1 + 1e20) D), which the export freezes to ~1e-20 of an entry
      = 25 + S;  k_solve_joint adds the workgroup records in double (solve_joint_body: s += (double)w[k]) and multiplies by a_f in double.
      With the export k_solve_joint sums every record in ONE workgroup: tcsfm_api.hip leaves JointSolveParams::nsplit at 0 on the export
      path (`split_of` is applied behind the export's return), so the split record sum CANNOT be reached by tcsfm_linearize_dense_window at
      any size: there is no such case (the refinement tests at 375 x 1242 run it).
    inverse pairs' g_pose, inv_photo, inv_dc: k_linearize<FRONT>'s block_reduce_publish and k_solve, exactly the pose linearisation's path:
      linearize_exact_inputs.additions(H, W) (13; 28 beyond 256 tiles of 32 x 16, where the last workgroup of a group of RG sums RG records).
    forward group's cost (additions_fwd): v[27] = o_w o_diff per source and extra_cost (the prior's term, S depth-consistency terms, the
      smoothness term: S + 1 additions) through the same 6 + 3 reduction, acc[OFF_SHARE + s], then num += over S sources and
      acc[OFF_S] += num: (S + 1) + 9 + S + 1 = 2 S + 11.
  F = the fixed-point scatter.  Every scattered tap is rounded to 2^-40 (DREF_FIX; front_scatter in kernels.h, k_dref_scatter_src): a
      destination pixel's sum is off by at most n_taps 2^-41 in the scatter's own units BEFORE its factor.  The target maps receive two sums
      (factor b_dc = w_dc / (S B HW) and a_i = 0.25 / K_i, joint_kernel.h: g_rho -= depth^2 (r_dc Edc - r_eph Eph)), the source maps one in
      units of a_f (k_dref_scatter_src; b_dc when K_f = 0):  F(p) = depth(p)^2 (b_dc + a_i) n_taps(p) 2^-41 / g_rho_abs64(p)  and
      F_s(p) = depth_s(p)^2 a_f n_taps_s(p) 2^-41 / g_rho_s_abs64(p); n_taps from the oracle.  It is applied per pixel: the judged quantity is
      max_p (|g - g64|(p) - F(p) g_abs64(p)) / g_abs64(p).
TIES.  At most MAX_TIE_FRAC = 1 % of a case's pixels may be near-ties (TIE = 5e-5) by the oracle's own criteria; no hard flip is allowed
(parity_util.check_flips_every_linearisation on the float64 replay).

CASES (conditions asserted on the CPU by tests/test_dense_linearize_exact_inputs_cpu.py; achieved values in brackets).  The joint kernels'
tiles are 32 x 8 (256 threads), the front launch's 32 x 16.  `default` = argmin 1, automask 1, (w_l1, w_ssim) = (0.15, 0.85), w_dc 0.15,
prior_init 0.1 about a depth0 that differs from depth_t (a smooth 3 % modulation), no smoothness, no pose consistency.  Every case runs the
sources export (g_rho_src) too.  The synthetic motion is scaled by 2 (SEEDS): unscaled, the flow at these sizes is a fraction of a pixel
and the auto-mask leaves pairs with a few per cent of the frame.
    5x9     B1 S2  no argmin, automask 0      sub-tile.  It needs no exemption from the mask floor: without the auto-mask every pair keeps 47 %
    9x40    B1 S1  w_smooth 2                 one row into a second joint-tile row; k_dref_smooth
    16x48   B2 S2                             LEAN S = 2 kernel; half-empty last tile column
    12x36   B1 S3  no argmin                  off-diagonal coupling
    20x36   B2 S4                             five-frame window; ragged both ways
    17x33   B2 S2                             one-pixel sliver tiles in both grids; the tile halo and the frame border coincide
    37x53   B2 S2                             ragged; the option set
    208x640 B1 S2                             the front launch leaves the direct-record path (260 tiles of 32 x 16 > DIRECT_MAX_TILES = 256:
                                              17 groups); the size the pose check uses.  (A 1 x 8193 strip has fewer pixels and is no frame.)
    -- split-record crossing: not reachable by the export (above).
    the option set, at 17x33 and at 37x53, B2 S2: a pairwise covering set (option_rows(), 11 rows: every value of every option meets every
    value of every other option in at least one row, at BOTH shapes) over argmin 1 / 0, automask 1 / 0, (w_l1, w_ssim) in (0.15, 0.85),
    (1, 0), (0, 1), w_dc 0 / 0.15 / W_DC_BIG, prior_init 0 / 0.1, w_smooth 0 / 2, w_pose_consist 0 / 0.5.
    37x53 B1 S2 out of bounds: a yaw that moves the image a quarter of its width, no auto-mask (the mask IS the validity): taps in the
    zero border, inverse samples outside the map [47 %, 31 %, 33 %, 45 % of the four pairs' pixels leave the frame; floor 20 %].
    37x53 B1 S2 scatter fallback: the sources are rendered from cameras ROLLED by FALLBACK_ROLL = 0.3 rad about the optical axis, so that
    the flow varies by more than FM = 6 pixels across a 32 x 16 tile: a share of the inverse pairs' valid taps lies outside the
    (32 + 12) x (16 + 12) LDS window front_scatter places by the tile's centre tap and goes to global memory directly (window_share())
    [13.1 % of the taps, 1454 of them; floor 5 %; the pairs keep 43 %, 43 %, 83 %, 54 % of the frame; floor 25 %].  Roll alone reaches both;
    no depth step is needed.  (It does not stand alone: the scaled motion over a floor a few centimetres below the camera sends 11.6 % of
    the 16x48 case's taps and 20.8 % of the out-of-bounds case's past the window too; the other shape cases send none.)
MASK FLOOR.  Every judged pair keeps MIN_MASK_FRAC = 25 % of the frame [inverse pairs: at least 36 %; forward pairs without the min over
the sources: at least 37 %].  Under the min over the sources a pixel goes to ONE source: the S forward pairs of a target share its selection,
25 % each is out of reach at S = 4 by counting.  There the floor holds for the target's selection [at least 70 %] and every one of its
pairs keeps at least MIN_MASK_FRAC / S [the smallest pair: 0.47 / S].  Near-ties: at most 0.28 % of a case's pixels [bar 1 %]; a pixel no
source sees is no decision and no tie.
W_DC_BIG = 2 is not a training value: the smallest power of two at which the depth-consistency part supplies at least 30 % of g_rho_abs64
on at least a quarter of the masked pixels of every target of every option row that carries it [2: 42 % of the pixels on the weakest rows,
the two that also carry w_smooth = 2, and 100 % on the others; 1: 19 % on those two].

Option values reach the engine as float32; the oracle is given the same float32 values.
TCSFM_TEST_DENSE_LIN_EXACT_REPORT=<file>: judge_case appends one line per case (id, then ratio to the float32 twin and E per measure).
"""
import collections
import functools
import itertools
import os

import numpy as np

import linearize_exact_inputs as LX

MARGIN = 4.0
MEASURES = ("rho", "rho_s", "xi_fwd", "xi_inv", "fwd", "inv_photo", "inv_dc")
TIE = 5e-5                      # ORC_TIE of oracle/tcsfm_oracle.c
MAX_TIE_FRAC = 0.01
MIN_MASK_FRAC = 0.25
W_DC_BIG = 2.0                  # (1: the depth-consistency part reaches 30 % on 19 % of the masked pixels of the rows that also carry w_smooth = 2; 2: 42 %)
MIN_DC_SHARE, MIN_DC_PIXELS = 0.30, 0.25
OOB_MIN_FRAC = 0.20
FALLBACK_MIN_SHARE, FALLBACK_MIN_MASK = 0.05, 0.25
FALLBACK_ROLL = 0.3
MIND, MAXD = 0.06, 2.67

# ---- what the bound pays for (joint_kernel.h, kernels.h, tcsfm_api.hip) --------------------------------------------------------------------
JTILE_W, JTILE_H = 32, 8                    # kJointTileW, kJointTileH: k_dense_joint, 256 threads, one pixel per thread
FTILE_W, FTILE_H = LX.TILE_W, LX.TILE_H     # k_linearize<FRONT>
FM = 6                                      # front_scatter's margin around the tile
DREF_FIX_BITS = 40
WAVE = 64


def additions_rho(S):
    return 8 + 2 + 3 + 2 + 2 * S + 2 + 1 + 1


def additions_xi(S):
    return (8 + 2 + 3 + 2 + 1) + (WAVE.bit_length() - 1) + (JTILE_W * JTILE_H // WAVE - 1) + S


def additions_fwd(S):
    return (S + 1) + (WAVE.bit_length() - 1) + (JTILE_W * JTILE_H // WAVE - 1) + S + 1


def allowances(c):
    """{measure: D 2^-24} (the fixed-point part F is per pixel: judge())"""
    inv = LX.additions(c.H, c.W)
    D = dict(rho=additions_rho(c.S), rho_s=additions_rho(1), xi_fwd=additions_xi(c.S), xi_inv=inv, fwd=additions_fwd(c.S), inv_photo=inv, inv_dc=inv)
    return {k: v * 2.0 ** -24 for k, v in D.items()}


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "kind H W B S argmin automask w_l1 w_ssim w_dc prior w_smooth w_pc seed motion")
WEIGHTS = [(0.15, 0.85), (1.0, 0.0), (0.0, 1.0)]
OPTION_VALUES = collections.OrderedDict(argmin=(1, 0), automask=(1, 0), weights=tuple(WEIGHTS), w_dc=(0.0, 0.15, W_DC_BIG), prior=(0.0, 0.1),
                                        w_smooth=(0.0, 2.0), w_pc=(0.0, 0.5))
# (seed, motion scale).  Motion: unscaled, the flow at these sizes is a fraction of a pixel, the identity reconstruction wins the auto-mask and
# pairs keep a few per cent of the frame; beyond 3 the floor -- a few centimetres below the camera -- passes behind it and validity falls under 50 %
SEEDS = {(5, 9): (95, 2.0), (9, 40): (95, 2.0), (16, 48): (95, 2.0), (12, 36): (95, 2.0), (20, 36): (95, 2.0), (17, 33): (95, 2.0), (37, 53): (95, 2.0),
         (208, 640): (95, 1.0)}


def case(H, W, B, S, kind="plain", **kw):
    seed, motion = SEEDS[(H, W)]
    d = dict(argmin=1, automask=1, weights=WEIGHTS[0], w_dc=0.15, prior=0.1, w_smooth=0.0, w_pc=0.0, seed=seed, motion=motion)
    d.update(kw)
    w = d.pop("weights")
    return Case(kind, H, W, B, S, d["argmin"], d["automask"], w[0], w[1], d["w_dc"], d["prior"], d["w_smooth"], d["w_pc"], d["seed"], d["motion"])


def option_rows():
    """a pairwise covering set over OPTION_VALUES, built greedily and deterministically: rows are taken from the full product in its own
    order, each time the row that covers the most value pairs not yet covered -> list of dicts"""
    names = list(OPTION_VALUES)
    pairs = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in OPTION_VALUES[a] for vb in OPTION_VALUES[b]}
    cover = lambda row: {(a, row[a], b, row[b]) for a, b in itertools.combinations(names, 2)}
    product = [dict(zip(names, v)) for v in itertools.product(*OPTION_VALUES.values())]
    rows = []
    while pairs:
        best = max(product, key=lambda r: len(cover(r) & pairs))       # (max keeps the first of equals)
        rows.append(best)
        pairs -= cover(best)
    return rows


SHAPE_CASES = [case(5, 9, 1, 2, argmin=0, automask=0), case(9, 40, 1, 1, w_smooth=2.0), case(16, 48, 2, 2), case(12, 36, 1, 3, argmin=0),
               case(20, 36, 2, 4), case(17, 33, 2, 2), case(37, 53, 2, 2)]
CROSSING_CASES = [case(208, 640, 1, 2)]
OPTION_SHAPES = [(17, 33), (37, 53)]
OPTION_CASES = [case(H, W, 2, 2, **r) for H, W in OPTION_SHAPES for r in option_rows() if case(H, W, 2, 2, **r) != case(H, W, 2, 2)]
OOB_CASE = case(37, 53, 1, 2, kind="oob", automask=0)
FALLBACK_CASE = case(37, 53, 1, 2, kind="fallback")
CASES = SHAPE_CASES + CROSSING_CASES + OPTION_CASES + [OOB_CASE, FALLBACK_CASE]


def case_id(c):
    s = f"{c.H}x{c.W}-B{c.B}-S{c.S}"
    if c.kind != "plain":
        return s + "-" + c.kind
    if c == case(c.H, c.W, c.B, c.S):
        return s + "-default"
    return s + f"-argmin{c.argmin}-am{c.automask}-l1_{c.w_l1:g}-ssim{c.w_ssim:g}-dc{c.w_dc:g}-prior{c.prior:g}-smooth{c.w_smooth:g}-pc{c.w_pc:g}"


IDS = [case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))
_f32 = LX._f32
oracle = LX.oracle


def oracle_opts(c, **kw):
    from oracle.oracle import default_opts
    d = dict(n_iters=1, automask=c.automask, w_l1=_f32(c.w_l1), w_ssim=_f32(c.w_ssim), w_dc=_f32(c.w_dc), irls_eps=_f32(1e-3),
             w_smooth=_f32(c.w_smooth), w_pose_consist=_f32(c.w_pc))
    d.update(kw)
    return default_opts(**d)


SOURCE_MOTION = (1.0, -1.0, 1.6, -1.6)      # source s moves by a different multiple of one base motion: no two sources are the same image


@functools.lru_cache(maxsize=8)
def inputs(c):
    """dict(tgt [B,3,H,W], srcs [S,B,3,H,W], depth_t [B,H,W], depth_s [S,B,H,W], depth0 [B,H,W], K [B,3,3], pose [2SB,6]), float32.
    depth_t is the scene's depth x 1.02 (the depth-consistency term sees a difference), depth0 a smooth 3 % modulation of depth_t."""
    from tightly_coupled_sfm_amd import synth
    H, W, B, S = c.H, c.W, c.B, c.S
    tg, dt, K = [], [], []
    sr, ds, p0 = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * SOURCE_MOTION[s] * c.motion
            if c.kind == "fallback":
                base[5] += FALLBACK_ROLL * (1.0 if s % 2 == 0 else -1.0)
            p = synth.make_pair(H, W, seed=c.seed + 7 * b, pose_gt=base, dtype=np.float64)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"])
            init = synth.perturb_pose(p["pose_gt"], c.seed + s, sigma_t=0.001 * c.motion, sigma_r=0.0003 * c.motion)
            if c.kind == "oob":        # yaw by what moves the image a quarter of its width (fx ry pixels)
                init[4] += 0.25 * W / p["K"][0, 0] * (1.0 if s % 2 == 0 else -1.0)
            p0[s].append(init)
    fwd = np.concatenate([np.stack(x) for x in p0])
    f = lambda a: np.ascontiguousarray(a, np.float32)
    depth_t = f(np.stack(dt))
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth0 = f(depth_t * (1.0 + 0.03 * np.sin(u / 5.0 + v / 7.0))[None])
    return dict(tgt=f(np.stack(tg)), srcs=f(np.stack([np.stack(x) for x in sr])), depth_t=depth_t, depth_s=f(np.stack([np.stack(x) for x in ds])),
                depth0=depth0, K=f(np.stack(K)), pose=f(np.concatenate([fwd, [synth.invert_pose(x) for x in fwd]])))


def reference(c, precision, bits=None, **kw):
    """the oracle's linearisation of the case (Oracle.linearize_dense_ref's dict), under `bits` [2SB,H,W] or its own decisions"""
    d = inputs(c)
    return oracle(precision).linearize_dense_ref(d["tgt"], d["srcs"], d["depth_t"], d["depth_s"], d["K"], d["pose"], kw.pop("opts", None) or oracle_opts(c),
                                                 argmin=bool(c.argmin), w_init=_f32(c.prior), depth0=kw.pop("depth0", d["depth0"]), min_depth=_f32(MIND),
                                                 max_depth=_f32(MAXD), bits=bits, **kw)


def pair_views(c):
    """(tgt, src, depth_t, depth_s, K, pose) of the 2SB directed pairs, forward pairs source-major, then the inverse pairs"""
    d = inputs(c)
    w = dict(target=d["tgt"], sources=d["srcs"], depth_t=d["depth_t"][:, None], depth_s=d["depth_s"][:, :, None], K=d["K"])
    import parity_util as PU
    return [v + (d["pose"][m],) for m, v in enumerate(PU.window_pair_views(w))]


@functools.lru_cache(maxsize=8)
def _maps(c, precision="f64"):
    return [oracle(precision).photometric(t, s, dt, ds, pose, K, w_l1=_f32(c.w_l1), w_ssim=_f32(c.w_ssim)) for t, s, dt, ds, K, pose in pair_views(c)]


@functools.lru_cache(maxsize=8)
def decisions(c, precision="f64"):
    """the oracle's own decisions of the case -> (mask [2SB,H,W] bool: what linearize_dense_ref sums under, near-tie [2SB,H,W] bool, valid
    [2SB,H,W] bool).  Near-ties as flip_note accepts them: an error within TIE of its auto-mask threshold; under the min over the sources
    the smallest gap among the selection's comparisons (the minimum and the runner-up, the minimum and the smallest threshold), booked on
    source 0's plane.  Forward pairs without argmin carry no auto-mask (optimizer.py:71-73)."""
    ph = _maps(c, precision)
    SB, N = c.S * c.B, 2 * c.S * c.B
    valid = np.stack([p["valid"] > 0.5 for p in ph])
    diff, ae = np.stack([p["diff"] for p in ph]).astype(np.float64), np.stack([p["auto_err"] for p in ph]).astype(np.float64)
    mask = reference(c, precision)["mask"] > 0.5
    tie = np.zeros_like(valid)
    for n in range(N):
        am = c.automask and (n >= SB or c.argmin)
        if am and not (n < SB and c.argmin and c.S > 1):
            tie[n] = valid[n] & (np.abs(diff[n] - ae[n]) < TIE)
    if c.argmin and c.S > 1:
        for b in range(c.B):
            idx = [s * c.B + b for s in range(c.S)]
            srt = np.sort(diff[idx], 0)
            gap = srt[1] - srt[0]
            amin = ae[idx].min(0)
            margin = np.where(np.abs(srt[0] - amin) < gap, np.abs(srt[0] - amin), gap) if c.automask else gap
            tie[idx[0]] = (margin < TIE) & valid[idx].any(0)          # (a pixel no source sees is no decision: both errors are the empty sample's)
    return mask, tie, valid


@functools.lru_cache(maxsize=8)
def own_bits(c, precision="f64"):
    """the oracle's OWN decisions in the trace format [2SB,H,W] uint16: validity, bilinear cell parity and sign codes as refine_record
    (one linearisation) records them per directed pair, bit 0 the mask linearize_dense_ref sums under"""
    orc = oracle(precision)
    mask = decisions(c, precision)[0]
    out = []
    for n, (t, s, dt, ds, K, pose) in enumerate(pair_views(c)):
        bits = orc.refine_record(t, s, dt, ds, pose, K, oracle_opts(c, w_smooth=0.0, w_pose_consist=0.0))[3][0]
        out.append((bits & 0xFFFE) | mask[n].astype(np.uint16))
    return np.stack(out)


def near_tie_fraction(c):
    return float(decisions(c)[1].sum()) / (2 * c.S * c.B * c.H * c.W)


def window_share(c):
    """-> (share of the inverse pairs' valid in-image taps that lie OUTSIDE the LDS window front_scatter places, number of such taps).
    Per inverse pair and 32 x 16 tile: the window is (32 + 2 FM) x (16 + 2 FM), its origin the top-left tap of the tile's centre thread
    (local (16, 8); beyond the frame its pixel is the reflected one: refl_idx) minus (16 + FM, 8 + FM).  Sample positions: the oracle's."""
    d, orc = inputs(c), oracle("f64")
    SB = c.S * c.B
    refl = lambda i, n: min(max(-i if i < 0 else (2 * n - 2 - i if i >= n else i), 0), n - 1)
    out = tot = 0
    valid = decisions(c)[2]
    for m in range(SB):
        ix, iy = orc.sample_positions(d["depth_s"][m // c.B, m % c.B], d["pose"][SB + m], d["K"][m % c.B])
        x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
        for ty in range(0, c.H, FTILE_H):
            for tx in range(0, c.W, FTILE_W):
                cy, cx = refl(ty + FTILE_H // 2, c.H), refl(tx + FTILE_W // 2, c.W)
                ox, oy = x0[cy, cx] - FTILE_W // 2 - FM, y0[cy, cx] - FTILE_H // 2 - FM
                sl = (slice(ty, min(ty + FTILE_H, c.H)), slice(tx, min(tx + FTILE_W, c.W)))
                for k in range(4):
                    xx, yy = x0[sl] + (k & 1), y0[sl] + (k >> 1)
                    live = valid[SB + m][sl] & (xx >= 0) & (xx < c.W) & (yy >= 0) & (yy < c.H)
                    inside = (xx - ox >= 0) & (xx - ox < FTILE_W + 2 * FM) & (yy - oy >= 0) & (yy - oy < FTILE_H + 2 * FM)
                    tot += int(live.sum()); out += int((live & ~inside).sum())
    return (out / tot if tot else 0.0), out


def outside_window_taps(c):
    """[S,B,H,W] uint8, bit t set: scattered tap t of that inverse pixel lies outside front_scatter's LDS window (Oracle's fault_scatter)"""
    d, orc = inputs(c), oracle("f64")
    SB = c.S * c.B
    refl = lambda i, n: min(max(-i if i < 0 else (2 * n - 2 - i if i >= n else i), 0), n - 1)
    drop = np.zeros((SB, c.H, c.W), np.uint8)
    for m in range(SB):
        ix, iy = orc.sample_positions(d["depth_s"][m // c.B, m % c.B], d["pose"][SB + m], d["K"][m % c.B])
        x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
        for ty in range(0, c.H, FTILE_H):
            for tx in range(0, c.W, FTILE_W):
                cy, cx = refl(ty + FTILE_H // 2, c.H), refl(tx + FTILE_W // 2, c.W)
                ox, oy = x0[cy, cx] - FTILE_W // 2 - FM, y0[cy, cx] - FTILE_H // 2 - FM
                sl = (slice(ty, min(ty + FTILE_H, c.H)), slice(tx, min(tx + FTILE_W, c.W)))
                for k in range(4):
                    xx, yy = x0[sl] + (k & 1), y0[sl] + (k >> 1)
                    inside = (xx - ox >= 0) & (xx - ox < FTILE_W + 2 * FM) & (yy - oy >= 0) & (yy - oy < FTILE_H + 2 * FM)
                    drop[m][sl] |= (~inside).astype(np.uint8) << k
    return drop.reshape(c.S, c.B, c.H, c.W)


def dc_share(c, bits=None):
    """per target: the share of its masked pixels on which the depth-consistency part supplies at least MIN_DC_SHARE of g_rho_abs64 (the
    part: g_rho_abs64 minus the same under the same decisions at w_dc = 0; w_dc is part of no decision)"""
    bits = own_bits(c) if bits is None else bits
    a, a0 = reference(c, "f64", bits)["g_rho_abs"], reference(c, "f64", bits, opts=oracle_opts(c, w_dc=0.0))["g_rho_abs"]
    SB = c.S * c.B
    out = []
    for b in range(c.B):
        m = np.any([(bits[s * c.B + b] & 1) > 0 for s in range(c.S)], 0)
        out.append(float((((a[b] - a0[b]) / a[b])[m] >= MIN_DC_SHARE).mean()))
    return out


# ---- judge -----------------------------------------------------------------------------------------------------------------------------
def engine_like(r, c):
    """an oracle result in the form of the engine's (run_engine): what the float32 twin is judged as"""
    return dict(g_rho=np.array(r["g_rho"]), g_rho_src=np.array(r["g_rho_s"]), g_pose=np.array(r["g_xi"]), K_f=r["K_f"], K_i=r["K_i"],
                fwd=r["L_fwd"] + (r["L_dc"] - r["L_dc_inv"]) + r["L_init"], inv_photo=r["L_inv"], inv_dc=r["L_dc_inv"])


def _fixed(c, r64):
    """(F(p) g_rho_abs64(p) [B,H,W], F_s(p) g_rho_s_abs64(p) [S,B,H,W]): the scatter's rounding in the outputs' units"""
    d = inputs(c)
    n, SB = c.H * c.W, c.S * c.B
    b_dc = _f32(c.w_dc) / (SB * n)
    a_i = 0.25 / r64["K_i"] if r64["K_i"] > 0 else 0.0
    a_f = ((1.0 if c.argmin else 0.25) / r64["K_f"]) if r64["K_f"] > 0 else b_dc
    q = 2.0 ** -(DREF_FIX_BITS + 1)
    return d["depth_t"].astype(np.float64) ** 2 * (b_dc + a_i) * r64["n_taps"] * q, d["depth_s"].astype(np.float64) ** 2 * a_f * r64["n_taps_s"] * q


def errors(eng, r64, c):
    """every measure of one result against float64 -> ({measure: E}, {measure: 99th percentile, maps only}, failures of the zero rule)"""
    fix, fix_s = _fixed(c, r64)
    e, p99, zero = {}, {}, []
    for k, g, g64, ab, fx in (("rho", eng["g_rho"], r64["g_rho"], r64["g_rho_abs"], fix), ("rho_s", eng["g_rho_src"], r64["g_rho_s"], r64["g_rho_s_abs"], fix_s)):
        g = np.asarray(g, np.float64)
        live = ab > 0
        if np.any(g[~live] != 0):
            zero.append(f"{k}: {int((g[~live] != 0).sum())} pixels with no contribution are not exactly zero")
        rel = np.maximum(np.abs(g - g64)[live] - fx[live], 0.0) / ab[live]
        e[k], p99[k] = float(rel.max()), float(np.quantile(rel, 0.99))
    SB = c.S * c.B
    rel = np.abs(np.asarray(eng["g_pose"], np.float64) - r64["g_xi"]) / r64["g_xi_abs"]
    e["xi_fwd"], e["xi_inv"] = float(rel[:SB].max()), float(rel[SB:].max())
    ref = engine_like(r64, c)
    for k in ("fwd", "inv_photo", "inv_dc"):
        a, b = float(eng[k]), float(ref[k])
        e[k] = abs(a - b) / b if b > 0 else (0.0 if a == 0 else np.inf)
    return e, p99, zero


def judge(c, eng, r64, r32, bits=None):
    """(engine result, float64 result, float32 result -- the two oracles under the same bits) -> (failures [str], figures {measure: (E,
    E32, bound)}, 99th percentiles)"""
    A = allowances(c)
    e, p99, fails = errors(eng, r64, c)
    e32 = errors(engine_like(r32, c), r64, c)[0]
    figs = {}
    for k in MEASURES:
        bound = MARGIN * e32[k] + A[k]
        figs[k] = (e[k], e32[k], bound)
        if not e[k] <= bound:
            fails.append(f"{k}: E = {e[k]:.3e} > {MARGIN:g} x {e32[k]:.3e} + {A[k]:.2e}")
    SB = c.S * c.B
    counts = (None, None) if bits is None else (int((bits[:SB] & 1).sum()), int((bits[SB:] & 1).sum()))
    for k, nb in zip(("K_f", "K_i"), counts):
        if not (float(eng[k]) == float(r64[k]) and (nb is None or float(eng[k]) == nb)):
            fails.append(f"{k}: engine {float(eng[k])}, trace {nb}, replay {float(r64[k])}")
    return fails, figs, p99


def judge_case(c, eng, bits, tag=None):
    """the engine's result under its trace `bits` [2SB,H,W] -> (failures, summary {measure: (ratio to the float32 twin, E)}).  Resets and
    fills the float64 oracle's flip statistics (linearisation 0)."""
    r32 = reference(c, "f32", bits)
    oracle("f64").flip_stats_reset()
    r64 = reference(c, "f64", bits)
    fails, figs, p99 = judge(c, eng, r64, r32, bits)
    summ = {k: ((e / e32 if e32 > 0 else (0.0 if e == 0 else np.inf)), e) for k, (e, e32, _) in figs.items()}
    rep = os.environ.get("TCSFM_TEST_DENSE_LIN_EXACT_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write("\t".join([tag or case_id(c)] + [f"{summ[k][0]:.2f}" for k in MEASURES] + [f"{summ[k][1]:.2e}" for k in MEASURES] +
                               [f"{p99[k]:.2e}" for k in ("rho", "rho_s")]) + "\n")
    return fails, summ


def todays_bar(eng, r64):
    """the bar of the five existing tests, np.abs(g - ref).max() < 2e-4 * np.abs(ref).max(), on g_pose, g_rho and g_rho_src -> passes?"""
    return all(np.abs(np.asarray(eng[a], np.float64) - r64[b]).max() < 2e-4 * np.abs(r64[b]).max()
               for a, b in (("g_pose", "g_xi"), ("g_rho", "g_rho"), ("g_rho_src", "g_rho_s")))


# ---- the engine side (GPU) --------------------------------------------------------------------------------------------------------------
def engine_opts(c):
    from tightly_coupled_sfm_amd.engine import default_opts
    return default_opts(n_iters=1, automask=c.automask, w_l1=c.w_l1, w_ssim=c.w_ssim, w_dc=c.w_dc, prior_init=c.prior, w_smooth=c.w_smooth,
                        w_pose_consist=c.w_pc, min_depth=MIND, max_depth=MAXD)


def run_engine(e, c, trace, sub=None, order=None):
    """the case's one linearisation on Engine e -> (result dict of numpy arrays, bits [2SB,H,W] uint16 or None).  sub = b: target b's
    window alone (B = 1); order: the call's targets in this order (a permutation of range(B))"""
    import torch
    d = inputs(c)
    sel = list(range(c.B)) if order is None else list(order)
    if sub is not None:
        sel = [sub]
    B = len(sel)
    pose = d["pose"].reshape(2, c.S, c.B, 6)[:, :, sel].reshape(2 * c.S * B, 6)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    if trace:
        e.trace_begin(1, 2 * c.S * B)
    L = e.linearize_dense_window(t(d["tgt"][sel]), t(d["srcs"][:, sel]), t(d["depth_t"][sel][:, None]), t(d["depth_s"][:, sel][:, :, None]), t(d["K"][sel]),
                                 t(pose), engine_opts(c), argmin=bool(c.argmin), depth0=t(d["depth0"][sel][:, None]), sources=True)
    bits = e.trace_end()[0][0] if trace else None
    out = dict(g_rho=L["g_rho"][:, 0].cpu().numpy(), g_rho_src=L["g_rho_src"][:, :, 0].cpu().numpy(), g_pose=np.array(L["g_pose"]),
               K_f=L["K_f"], K_i=L["K_i"], fwd=L["fwd"], inv_photo=L["inv_photo"], inv_dc=L["inv_dc"], loss=L["loss"], a_f=L["a_f"],
               pose_consist=L["pose_consist"])
    return out, bits


def traced_and_production(e, c):
    """the case with the trace on, then off: every output must be the same bits, so that judging the traced run vouches for the production
    instantiations of the kernels -> (result, bits)"""
    tr, bits = run_engine(e, c, True)
    pr, _ = run_engine(e, c, False)
    for k in tr:
        assert np.array_equal(tr[k], pr[k]), ("production kernels differ from the recording ones", case_id(c), k)
    return tr, bits
