"""Cases, metric and judge of the entry-by-entry check of the pose linearisations (k_linearize -> k_solve's record: H, g, cost_photo,
cost_dc, mask count), shared by tests/test_linearize_exact_inputs_cpu.py and tests/test_gpu_linearize_exact.py.  No GPU here (run_engine
and child_main are the only functions that touch one, and they import torch themselves).

WHY.  The linearisation-level tests elsewhere (test_gpu_parity.py, test_gpu_options._assert_lin, the window-rule tests) compare H and g
with the float64 oracle to 2e-4 of their LARGEST entry, because they do not pin the discrete decisions: one flipped mask pixel in 5508
moves H by 1.8e-4 of its largest entry.  That bar cannot see the depth-scale row of a 7-parameter H (H[6][6] / max|H| = 7e-5), nor the
depth-consistency accumulators (0.1 % .. 5 % of H's diagonal).  Here the engine's decisions are recorded (tcsfm_debug_trace, honoured by
tcsfm_linearize / tcsfm_linearize_window) and replayed in the oracle (Oracle.linearize / linearize_window, bits=...), so that what
is left is continuous arithmetic, and every entry is held to the accuracy of an fp32 evaluation of ITS OWN sum.

METRIC, per directed pair, engine against float64 under the engine's own bits:
    E_H     = max_jk |H - H64|_jk / sqrt(H64_jj H64_kk)    per pixel H is positive semidefinite, so by Cauchy-Schwarz sqrt(H_jj H_kk) bounds
                                                           sum |terms| of entry jk: the error relative to what was actually summed
    E_g     = max_j |g - g64|_j / gabs64_j                 gabs_j = sum over the pixels of |the pixel's contribution to g_j| (oracle)
    E_photo = |cost_photo - cost_photo64| / cost_photo64   (non-negative terms); E_dc the same for cost_dc
    n_mask  = population count of bit 0 of the trace, exactly.
BOUND.  E <= MARGIN * E(float32 oracle, same inputs, same bits) + A, MARGIN = 4 (the project's two bits, as in the warp, photometric and
loss gradient tests); a measure in which the float32 twin is exact keeps A alone.  The float32 oracle computes every pixel in float but
ACCUMULATES in double, the kernel accumulates in fp32: A = D * 2^-24 pays for that and for nothing else, D = the number of fp32 additions
on the longest path from a thread's accumulator to the first double-precision sum (additions(), below: read off block_reduce_publish
and k_solve, not measured).

CASES (case conditions asserted on the CPU by tests/test_linearize_exact_inputs_cpu.py).  Tiles are 32 wide, 16 high, 512 threads:
    8x16     1 tile, partial      smallest golden size
    16x32    1 tile, exact        no ragged edge
    17x33    4 tiles              three are one-pixel slivers: the tile halo and the frame's reflect border coincide
    37x53    6 tiles              ragged; fewer tiles than XCDs (q = 0 in the tile remap)
    48x160   15 tiles             nblk & 7 = 7
    256x512  256 tiles            last size on the direct-record path
    208x640  260 tiles            first size on the group-reduction path: 17 groups, the last holds 4; nblk & 7 = 4
Every shape with the default options at N = 3 (distinct items, a handle made for more pairs than the call uses), the two largest also
at N = 1.  At 17x33 and 37x53 the full option set: refine 0 / 1 (non-zero log_scale) x w_dc 0 / 0.15 / W_DC_BIG x (w_l1, w_ssim) in
(0.15, 0.85), (1, 0), (0, 1) x automask 0 / 1, one pose that puts more than 20 % of the frame out of bounds (a quarter-width yaw, no
auto-mask: the mask is the validity and its border), and windows (B = 2, S = 2:
8 directed pairs) with argmin on / off x both window rules x refine 0 / 1.
W_DC_BIG is not a training value: it makes the depth-consistency accumulators a large share of H (at least 30 % of every H64_jj,
asserted), so that their error is not hidden beneath the photometric terms.  15 does not reach that share on these inputs (25 % of the
smallest H64_jj at 17x33, 6 % at 37x53), so it was raised: 128 supplies 74 % and 34 %.

Option values reach the engine as float32; the oracle is given the same float32 values (w_dc = 0.15f is 4e-8 away from 0.15).
TCSFM_TEST_LIN_EXACT_REPORT=<file>: judge_case appends one line per case (id, then ratio to the float32 twin and E for H | g |
cost_photo | cost_dc).
"""
import collections
import functools
import os

import numpy as np

import parity_util as PU

MARGIN = 4.0
MEASURES = ("H", "g", "cost_photo", "cost_dc")
TIE = 5e-5                      # ORC_TIE of oracle/tcsfm_oracle.c: what flip_note accepts as a near-tie
MAX_TIE_FRAC = 0.01             # of a case's pixels may be near-ties (decisions replayed rather than computed)
MIN_MASK_FRAC = 0.25
W_DC_BIG = 128.0                # (15 supplies 25 % of the smallest H64_jj at 17x33 and 6 % at 37x53; 128: 74 % and 34 %)
MIN_DC_SHARE = 0.30
OOB_MIN_FRAC = 0.20
LOG_SCALE = np.array([0.04, 0.03, -0.05, 0.02, -0.03, 0.05, -0.02, 0.01], np.float32)

# ---- the reduction the bound pays for (tightly_coupled_sfm_amd/csrc: tcsfm_api.hip TILE_W / TILE_H / direct_records, kernels.h RG) ------
TILE_W, TILE_H, NT = 32, 16, 512            # k_linearize: one thread per centre pixel of a tile
RG = 16                                     # workgroups per in-launch reduction group
DIRECT_MAX_TILES = 256                      # direct_records(): up to this many tiles k_solve reads one record per workgroup
WAVE = 64


def n_tiles(H, W):
    return -(-W // TILE_W) * -(-H // TILE_H)


def additions(H, W):
    """D: fp32 additions on the longest path from one thread's accumulator to the first double-precision sum.
         PPT - 1                 a thread accumulates PPT = TILE_W TILE_H / NT centre pixels: 1 here, nothing is added per thread
       + log2(64) = 6            wave butterfly (wave_reduce.h): every reduced value went through one addition per lane bit
       + NT / 64 - 1 = 7         block_reduce_publish sums the 8 wave partials of a workgroup in order (0 + x is exact)
       + RG - 1 = 15             only beyond DIRECT_MAX_TILES tiles: the last workgroup of a group of RG sums the group's records
     k_solve then converts every record to double before it adds (solve_body: s += (double)v[j]): nothing more in fp32."""
    ppt = TILE_W * TILE_H // NT
    d = (ppt - 1) + (WAVE.bit_length() - 1) + (NT // WAVE - 1)
    if n_tiles(H, W) > DIRECT_MAX_TILES:
        d += RG - 1
    return d


def allowance(H, W):
    return additions(H, W) * 2.0 ** -24


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "kind H W N max_pairs refine w_dc w_l1 w_ssim automask oob argmin rule seed")
SHAPES = [(8, 16), (16, 32), (17, 33), (37, 53), (48, 160), (256, 512), (208, 640)]
OPTION_SHAPES = [(17, 33), (37, 53)]
WEIGHTS = [(0.15, 0.85), (1.0, 0.0), (0.0, 1.0)]
PAIR_SEED = 4
WINDOW_SEED = {(17, 33): 115, (37, 53): 95}       # (17x33 at seed 95: a forward pair keeps 22 % of the frame under argmin)


def pair_case(H, W, N=3, refine=0, w_dc=0.0, weights=WEIGHTS[0], automask=1, oob=0, seed=PAIR_SEED):
    return Case("pair", H, W, N, N + 2, refine, w_dc, weights[0], weights[1], automask, oob, 0, 0, seed)


def window_case(H, W, argmin, rule, refine, seed=None):
    seed = WINDOW_SEED[(H, W)] if seed is None else seed
    return Case("window", H, W, 8, 10, refine, 0.0, WEIGHTS[0][0], WEIGHTS[0][1], 1, 0, argmin, rule, seed)


DEFAULT_CASES = [pair_case(H, W) for H, W in SHAPES] + [pair_case(H, W, N=1) for H, W in SHAPES[-2:]]
OPTION_CASES = [pair_case(H, W, refine=r, w_dc=d, weights=w, automask=a)
                for H, W in OPTION_SHAPES for r in (0, 1) for d in (0.0, 0.15, W_DC_BIG) for w in WEIGHTS for a in (0, 1)
                if not (r == 0 and d == 0.0 and w == WEIGHTS[0] and a == 1)]          # (that one is the default case)
OOB_CASES = [pair_case(H, W, w_dc=0.15, automask=0, oob=1) for H, W in OPTION_SHAPES]      # (no auto-mask: the mask IS the validity)
WINDOW_CASES = [window_case(H, W, am, rule, r) for H, W in OPTION_SHAPES for am in (1, 0) for rule in (0, 1) for r in (0, 1)]
CASES = DEFAULT_CASES + OPTION_CASES + OOB_CASES + WINDOW_CASES
ADJOINT_CASES = [pair_case(H, W) for H, W in OPTION_SHAPES] + WINDOW_CASES


def case_id(c):
    s = f"{c.kind}-{c.H}x{c.W}-N{c.N}"
    if c.kind == "window":
        return s + f"-argmin{c.argmin}-rule{c.rule}-refine{c.refine}"
    if c == pair_case(c.H, c.W, c.N):
        return s + "-default"
    return s + f"-refine{c.refine}-dc{c.w_dc:g}-l1_{c.w_l1:g}-ssim{c.w_ssim:g}-am{c.automask}" + ("-oob" if c.oob else "")


IDS = [case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))


def _f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def oracle(precision):
    from oracle.oracle import Oracle
    return Oracle(precision)


def oracle_opts(c, **kw):
    """the case's options as the engine sees them (float32 values).  prior_scale = 0: tcsfm_linearize* export the RAW normal equations,
    the oracle's window export would add the scale prior's 2 prior_scale to H[6][6]"""
    from oracle.oracle import default_opts
    d = dict(nparam=6 + c.refine, automask=c.automask, w_l1=_f32(c.w_l1), w_ssim=_f32(c.w_ssim), w_dc=_f32(c.w_dc), irls_eps=_f32(1e-3),
             prior_scale=0.0)
    d.update(kw)
    return default_opts(**d)


# synth's default motion is metric: at 8x16 its flow is a twentieth of a pixel, the source is the target to within the noise and the
# auto-mask keeps 5 % of the frame.  There the motion is scaled so that the flow is a pixel again and the mask condition can hold.
MOTION = {(8, 16): 8.0}


def _batch(N, H, W, seed0):
    """synth.make_batch(N, H, W, seed0) -- the same pairs, seeds and perturbed initial poses -- with the motion scaled by MOTION[(H, W)]"""
    from tightly_coupled_sfm_amd import synth
    k = MOTION.get((H, W))
    if k is None:
        return synth.make_batch(N, H, W, seed0=seed0)
    out = {n: [] for n in ("tgt", "src", "depth_t", "depth_s", "K", "pose_init")}
    for i in range(N):
        gt = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * np.random.default_rng(1000 + seed0 + i).uniform(0.7, 1.3, size=6) * k
        p = synth.make_pair(H, W, seed=seed0 + i, pose_gt=gt)
        for n in ("tgt", "src", "K"):
            out[n].append(p[n])
        out["depth_t"].append(p["depth_t"][None]); out["depth_s"].append(p["depth_s"][None])
        out["pose_init"].append(synth.perturb_pose(p["pose_gt"], seed=seed0 + i))
    return {n: np.ascontiguousarray(np.stack(v)) for n, v in out.items()}


@functools.lru_cache(maxsize=16)
def inputs(c):
    """pair: synth batch dict (tgt, src [N,3,H,W], depth_t, depth_s [N,1,H,W], K [N,3,3], pose [N,6], ls [N]);
    window: dict(target [B,3,H,W], sources [S,B,3,H,W], depth_t [B,1,H,W], depth_s [S,B,1,H,W], K [B,3,3], pose [2SB,6], ls [2SB])"""
    from tightly_coupled_sfm_amd import synth
    ls = LOG_SCALE[:c.N] if c.refine else np.zeros(c.N, np.float32)
    if c.kind == "pair":
        # N = 1: item 1 of the N = 3 batch of the same shape (also what the batch-independence test calls alone)
        b = _batch(3, c.H, c.W, c.seed)
        sl = slice(1, 2) if c.N == 1 else slice(0, c.N)
        d = {k: np.ascontiguousarray(b[k][sl], np.float32) for k in ("tgt", "src", "depth_t", "depth_s", "K")}
        pose = np.array(b["pose_init"][sl], np.float32)
        if c.oob:      # yaw by what moves the image a quarter of its width (fx ry pixels): that strip of every item leaves the source frame
            pose[:, 4] += np.float32(0.25 * c.W / d["K"][:, 0, 0]) * np.float32([1, -1, 1][:c.N])
        d["pose"] = pose
        d["ls"] = ls if c.N > 1 or not c.refine else LOG_SCALE[1:2]
        return d
    import standins
    w = standins.make_window(2, 2, c.H, c.W, seed0=c.seed)
    o64 = oracle("f64")
    out = {k: np.ascontiguousarray(w[k], np.float32) for k in ("target", "sources", "K")}
    out["depth_t"] = o64.disp_to_depth(w["disp_t"], 0.06, 2.67)[1].astype(np.float32)
    out["depth_s"] = o64.disp_to_depth(w["disp_s"], 0.06, 2.67)[1].astype(np.float32)
    out["pose"] = np.ascontiguousarray(w["first"], np.float32)
    out["ls"] = ls
    return out


def pair_views(c):
    """(tgt, src, depth_t, depth_s, K, pose, log_scale) of every directed pair of the case (numpy, [H,W] depth maps)"""
    d = inputs(c)
    if c.kind == "pair":
        return [(d["tgt"][n], d["src"][n], d["depth_t"][n, 0], d["depth_s"][n, 0], d["K"][n], d["pose"][n], float(d["ls"][n])) for n in range(c.N)]
    return [v + (d["pose"][m], float(d["ls"][m])) for m, v in enumerate(PU.window_pair_views(dict(d, first=d["pose"])))]


def _items(r, n):
    keys = ("H", "g", "gabs", "cost", "cost_photo", "cost_dc", "n_mask")
    return [{k: np.array(r[k][m]) for k in keys if k in r} for m in range(n)]


def reference(c, precision, bits=None):
    """the oracle's linearisation of every directed pair of the case -> list of dict(H, g, gabs, cost, cost_photo, cost_dc, n_mask);
    bits [N,H,W] uint16: under these decisions"""
    orc, d = oracle(precision), inputs(c)
    if c.kind == "pair":
        out = []
        for n, (t, s, dt, ds, K, pose, ls) in enumerate(pair_views(c)):
            out.append(orc.linearize(t, s, dt, ds, pose, K, oracle_opts(c), log_scale=ls, bits=None if bits is None else bits[n]))
        return out
    r = orc.linearize_window(d["target"], d["sources"], d["depth_t"][:, 0], d["depth_s"][:, :, 0], d["K"], d["pose"], oracle_opts(c),
                             argmin=bool(c.argmin), rule=c.rule, log_scale=d["ls"].astype(np.float64) if c.refine else None, bits=bits)
    return _items(r, c.N)


def _maps(c, precision="f64"):
    """Oracle.photometric of every directed pair at the case's poses"""
    orc = oracle(precision)
    return [orc.photometric(t, s, dt, ds, pose, K, log_scale=ls, w_l1=_f32(c.w_l1), w_ssim=_f32(c.w_ssim)) for t, s, dt, ds, K, pose, ls in pair_views(c)]


def _decisions(c, precision="f64"):
    """the oracle's own mask decisions -> (mask [N,H,W] bool, near-tie [N,H,W] bool, valid [N,H,W] bool).  A near-tie is what flip_note
    (oracle/tcsfm_oracle.c) accepts as one: an error within TIE of its auto-mask threshold; with the min over the sources the smallest
    gap among the selection's comparisons (two sources' errors, the minimum and the smallest threshold), booked on the target's pixel"""
    ph = _maps(c, precision)
    N = c.N
    valid = np.stack([p["valid"] > 0.5 for p in ph])
    diff, ae = np.stack([p["diff"] for p in ph]).astype(np.float64), np.stack([p["auto_err"] for p in ph]).astype(np.float64)
    SB = N // 2
    fwd_plain = c.kind == "window" and c.rule == 1 and not c.argmin          # REFERENCE rule without argmin: validity alone (optimizer.py:71-73)
    mask, tie = np.zeros_like(valid), np.zeros_like(valid)
    for n in range(N):
        am = c.automask and not (fwd_plain and n < SB)
        mask[n] = valid[n] & ((diff[n] < ae[n]) if am else True)
        tie[n] = valid[n] & (np.abs(diff[n] - ae[n]) < TIE) if am else False
    if c.kind == "window" and c.argmin:
        B, S = 2, 2
        for b in range(B):
            idx = [s * B + b for s in range(S)]
            dmin, smin = diff[idx].min(0), diff[idx].argmin(0)            # (first minimum, as torch.min over the source axis)
            amin, vany = ae[idx].min(0), valid[idx].any(0)
            keep = vany & ((dmin < amin) if c.automask else True)
            gap = np.abs(diff[idx[0]] - diff[idx[1]])
            margin = np.where(np.abs(dmin - amin) < gap, np.abs(dmin - amin), gap) if c.automask else gap
            for s in range(S):
                mask[idx[s]] = keep & (smin == s)
                tie[idx[s]] = (margin < TIE) if s == 0 else False
    return mask, tie, valid


@functools.lru_cache(maxsize=16)
def own_bits(c, precision="f64"):
    """the oracle's OWN decisions of the case's linearisation in the trace format [N,H,W] uint16: validity, bilinear cell parity and sign
    codes as refine_record (n_iters = 1) records them per pair, bit 0 the mask (for the forward pairs of a window: the selection)"""
    orc = oracle(precision)
    mask, _, _ = _decisions(c, precision)
    out = []
    for n, (t, s, dt, ds, K, pose, ls) in enumerate(pair_views(c)):
        bits = orc.refine_record(t, s, dt, ds, pose, K, oracle_opts(c, n_iters=1), log_scale=ls)[3][0]
        out.append((bits & 0xFFFE) | mask[n].astype(np.uint16))
    return np.stack(out)


def near_tie_fraction(c):
    return float(_decisions(c)[1].sum()) / (c.N * c.H * c.W)


# ---- judge -----------------------------------------------------------------------------------------------------------------------------
def errors(r, r64):
    """the four measures of one pair's result against float64 -> dict"""
    H64, g64 = np.asarray(r64["H"], np.float64), np.asarray(r64["g"], np.float64)
    dg = np.sqrt(np.outer(np.diag(H64), np.diag(H64)))
    out = dict(H=float(np.max(np.abs(np.asarray(r["H"], np.float64) - H64) / dg)), g=float(np.max(np.abs(np.asarray(r["g"], np.float64) - g64) / r64["gabs"])))
    for k in ("cost_photo", "cost_dc"):
        a, b = float(r[k]), float(r64[k])
        out[k] = abs(a - b) / b if b > 0 else (0.0 if a == 0 else np.inf)
    return out


def judge(eng, r64, r32, A, n_bits=None):
    """one pair: (engine result, float64 result, float32 result -- the two oracles under the engine's bits), A = allowance(H, W),
    n_bits = population count of bit 0 of the pair's trace -> (failures [str], figures {measure: (E, E32, bound)})"""
    fails, figs = [], {}
    e, e32 = errors(eng, r64), errors(r32, r64)
    for k in MEASURES:
        bound = MARGIN * e32[k] + A
        figs[k] = (e[k], e32[k], bound)
        if not e[k] <= bound:
            fails.append(f"{k}: E = {e[k]:.3e} > {MARGIN:g} x {e32[k]:.3e} + {A:.2e}")
    if n_bits is not None and not (float(eng["n_mask"]) == n_bits == float(r64["n_mask"])):
        fails.append(f"n_mask: engine {float(eng['n_mask'])}, trace {n_bits}, replay {float(r64['n_mask'])}")
    return fails, figs


def engine_items(out, N):
    return _items(out, N)


def judge_case(c, eng_items, bits, tag=None):
    """every pair of a case: the engine's results (list of dicts) under its trace `bits` [N,H,W] -> (failures, summary {measure: (worst
    ratio to the float32 twin, largest E)}).  Resets and fills the float64 oracle's flip statistics (linearisation 0)."""
    oracle("f64").flip_stats_reset()
    r64, r32 = reference(c, "f64", bits), reference(c, "f32", bits)
    A = allowance(c.H, c.W)
    fails, summ = [], {k: (0.0, 0.0) for k in MEASURES}
    for n in range(c.N):
        f, figs = judge(eng_items[n], r64[n], r32[n], A, int((bits[n] & 1).sum()))
        fails += [f"pair {n}: {x}" for x in f]
        for k, (e, e32, _) in figs.items():
            ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else np.inf)
            summ[k] = (max(summ[k][0], ratio), max(summ[k][1], e))
    rep = os.environ.get("TCSFM_TEST_LIN_EXACT_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write("\t".join([tag or case_id(c)] + [f"{summ[k][0]:.2f}" for k in MEASURES] + [f"{summ[k][1]:.2e}" for k in MEASURES]) + "\n")
    return fails, summ


# ---- the engine side (GPU) --------------------------------------------------------------------------------------------------------------
def engine_opts(c):
    from tightly_coupled_sfm_amd.engine import default_opts
    return default_opts(refine=c.refine, automask=c.automask, w_l1=c.w_l1, w_ssim=c.w_ssim, w_dc=c.w_dc, argmin=c.argmin, window_rule=c.rule)


def run_engine(e, c, trace):
    """the case's one linearisation on Engine e -> (list of per-pair dicts, bits [N,H,W] uint16 or None)"""
    import torch
    d = inputs(c)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    ls = t(d["ls"]) if c.refine else None
    if trace:
        e.trace_begin(1, c.N)
    if c.kind == "pair":
        out = e.linearize(t(d["tgt"]), t(d["src"]), t(d["depth_t"]), t(d["depth_s"]), t(d["K"]), t(d["pose"]), engine_opts(c), log_scale=ls)
    else:
        out = e.linearize_window(t(d["target"]), t(d["sources"]), t(d["depth_t"]), t(d["depth_s"]), t(d["K"]), t(d["pose"]), engine_opts(c), log_scale=ls)
    bits = e.trace_end()[0][0] if trace else None
    return engine_items(out, c.N), bits


def traced_and_production(e, c):
    """the case with the trace on, then off: H, g and the four statistics must be the same bits, so that judging the traced run vouches
    for the production instantiation of the kernel (parity_util.traced_and_production does this for refinements) -> (items, bits)"""
    tr, bits = run_engine(e, c, True)
    pr, _ = run_engine(e, c, False)
    for n in range(c.N):
        for k in ("H", "g", "cost", "cost_photo", "cost_dc", "n_mask"):
            assert np.array_equal(tr[n][k], pr[n][k]), ("production kernel differs from the recording one", case_id(c), n, k)
    return tr, bits


def child_main(path, ids):
    """a fresh process (TCSFM_ADJOINT is read once per process): run the named cases, traced == production, results and bits to `path`"""
    from tightly_coupled_sfm_amd.engine import Engine
    out = {}
    for i in ids:
        c = BY_ID[i]
        e = Engine(c.H, c.W, c.max_pairs)
        items, bits = traced_and_production(e, c)
        e.close()
        out[i + "/bits"] = bits
        for k in ("H", "g", "cost", "cost_photo", "cost_dc", "n_mask"):
            out[i + "/" + k] = np.stack([it[k] for it in items])
    np.savez(path, **out)
