/*
 * tcsfm.h -- C ABI of libtcsfm_hip.so, the MI355X (gfx950) photometric pose/depth refinement engine.
 *
 * This is the drop-in boundary for the hot path of utiasSTARS/tightly-coupled-SfM
 * (SURVEY.md section 8a/8b).  The reference is pure Python/PyTorch and has no FFI; every entry
 * point below names the reference function (file:line under /root/reference) it replaces.
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C, no torch types.  All array arguments are fp32, contiguous, NCHW like the reference:
 *       images [N,3,H,W], depth maps [N,1,H,W] (== [N,H,W]), intrinsics [N,3,3] row-major, poses [N,6].
 *   - a "pair" is one DIRECTED frame pair (target, source); the reference stacks forward and inverse
 *     pairs along N the same way (train_mono.py:54-62).
 *   - pose 6-vector = the reference's [tx,ty,tz,rx,ry,rz] (models/stn.py:143-158).  The warp uses
 *     pose_vec2mat(-pose) exactly like the reference call sites (train_mono.py:69, helpers.py:11).
 *   - intrinsics must be pinhole [fx 0 cx; 0 fy cy; 0 0 1] (all of the reference's loaders produce
 *     this form); anything else returns TCSFM_E_INTRINSICS: at once for host pointers and for the first use
 *     of a device buffer (one small blocking copy), and -- when the CONTENTS of an already validated device
 *     buffer change behind the library's back -- from a device-side guard: that call's results are NaN and
 *     the error is returned by the next call on the handle or by tcsfm_synchronize().
 *   - every entry point runs on the handle's device and restores the caller's current device on return.
 *   - pointers are DEVICE pointers unless tcsfm_opts.host_ptrs != 0, in which case the library stages
 *     them through its own device buffers (PCIe-inclusive path).
 *   - every call is asynchronous on the handle's HIP stream when given device pointers, except that
 *     host-pointer calls and calls returning host scalars synchronise that stream before returning.
 *   - return value: 0 = ok, negative = error; tcsfm_last_error() gives the message.  Nothing throws.
 *   - one handle = one device + one stream; calls on a handle are not re-entrant.
 *   - an output must not overlap another array of the same call, a few documented pairs excepted: see "overlapping arguments" below.
 */
#ifndef TCSFM_H
#define TCSFM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tcsfm_ctx *tcsfm_handle;

enum {
    TCSFM_OK = 0,
    TCSFM_E_ARG = -1,        /* bad argument (null pointer, size out of range, ...)   */
    TCSFM_E_HIP = -2,        /* a HIP runtime call failed                              */
    TCSFM_E_INTRINSICS = -3, /* non-pinhole intrinsics                                 */
    TCSFM_E_NOMEM = -4
};

enum { TCSFM_SOLVER_GN = 0, TCSFM_SOLVER_LM = 1 };
enum { TCSFM_PARAM_SE3 = 0,    /* T <- exp(delta^) T, delta = [rho, phi] (liegroups ordering, validate.py:65) */
       TCSFM_PARAM_EULER = 1   /* pose <- pose + delta on the reference's [t, euler] vector                    */ };
enum { TCSFM_REFINE_POSE = 0,        /* 6 DoF                                                  */
       TCSFM_REFINE_POSE_SCALE = 1   /* 6 DoF + log depth-scale shared by both depth maps (7x7) */ };

/* How tcsfm_refine_window / tcsfm_linearize_window combine the 2*S*B directed pairs of a call:
 *   PAIR       every directed pair is its own least-squares problem: normalised by ITS OWN mask count, weighted by ITS OWN
 *              depth-consistency weight map, depth-consistency term w_dc * mean over its own pixels.
 *   REFERENCE  the scalar that is minimised is the reference's compute_optimization_loss itself (optimizer.py:47-86, default
 *              options; pinned by golden G13 = the reference's loss and autograd gradients):
 *                forward term   sum_b sum_p keep dmin W_{source 0} / sum_b sum_p keep   (batch-summed normaliser; the weight map
 *                               of SOURCE 0 multiplies every forward pixel whichever source won it, optimizer.py:69);
 *                               without argmin: 0.25 sum valid W diff / sum valid over all forward pairs, no auto-mask (:71-73)
 *                inverse term   0.25 sum M W diff / sum M over all inverse pairs of the call (:75-79)
 *                depth consist. w_dc * (mean over all forward pairs and pixels + mean over all inverse pairs and pixels) (:83-86)
 *              Every pair still takes its own 6x6 / 7x7 step, with the exact gradient of that scalar w.r.t. its pose (the pose of
 *              source 0 also moves the weight of the pixels the other sources won) and its own block of the curvature model.
 *              The batch is the call's B targets: results depend on how windows are grouped into calls, exactly as the
 *              reference's loss depends on config['minibatch']. */
enum { TCSFM_WINDOW_PAIR = 0, TCSFM_WINDOW_REFERENCE = 1 };

/* the unknown of a target's depth in the dense window mode under TCSFM_WINDOW_REFERENCE:
 * FULL     one inverse depth per pixel (default).
 * QUARTER  the reference's own parametrisation of optimize_depth_pred (optimizer.py:194-198, 235-239): the QUARTER-resolution map
 *          (F.interpolate of the input to (H/4, W/4), bilinear), which every linearisation sees through its x4 bilinear upsampling
 *          (align_corners = False; sigmoid disparity and inverse depth are affine in each other, so it is the same unknown).  H and W
 *          must be multiples of 4.  The call starts from the quarter-resolution projection of the input map -- as the reference does --
 *          and returns the upsampled map; the SSIM prior stays centred on the full-resolution input (`self.target_disparity`, :89-90).
 *          Gradient: the full-resolution one through the transpose of the upsampling (exact; pinned on reference autograd w.r.t. the
 *          quarter-resolution leaf, golden G13 `qinit`).  Curvature: every cell gets the row-sum lumping sum_p U_pc D_p of the pixels'
 *          diagonal model, which majorises U' diag(D) U, so the depth is still eliminated per cell (a 6S x 6S system per target). */
enum { TCSFM_DEPTH_FULL = 0, TCSFM_DEPTH_QUARTER = 1 };

typedef struct tcsfm_opts {
    int32_t n_iters;       /* linearisations per refine call (BASELINE.json: 4)                         */
    int32_t solver;        /* TCSFM_SOLVER_*                                                             */
    int32_t param;         /* TCSFM_PARAM_*                                                              */
    int32_t refine;        /* TCSFM_REFINE_*                                                             */
    int32_t automask;      /* mask = valid * (diff < auto_err), helpers.py:17-19; options['automasking'] */
    int32_t depth_is_disp; /* depth inputs are sigmoid disparities: disp_to_depth is fused (learning_helpers.py:77-86) */
    int32_t host_ptrs;     /* 1: array arguments are host pointers (the call synchronises); 2: PINNED host pointers,
                              asynchronous (tcsfm_refine_window_async only)                                 */
    int32_t argmin;        /* tcsfm_refine_window with S > 1: per-pixel min over the sources, options['diff_img_argmin'] */
    float w_l1, w_ssim;    /* 0.15 / 0.85, train_mono.py:87                                              */
    float w_dc;            /* options['l_depth_consist_weight'] if options['l_depth_consist'] else 0, optimizer.py:83-86 */
    float irls_eps;        /* floor of the IRLS denominators                                             */
    float lambda0, lambda_up, lambda_down, lambda_min; /* Marquardt damping (relative to diag H)        */
    float min_depth, max_depth; /* config['min_depth'], config['max_depth'] (depth_is_disp only)       */
    float prior_scale;     /* POSE_SCALE only: weight of (log_scale - initial)^2.  The photometric cost cannot separate
                              depth scale from |t| (exact gauge); this prior makes the 7-DoF problem well posed.   */
    float lambda_depth;    /* dense mode: Marquardt damping of the per-pixel depth block (default 1.0)                */
    float prior_depth;     /* dense mode: weight of the masked prior sum M ((rho-rho0)/rho0)^2 / sum M (default 10)   */
    int32_t window_rule;   /* TCSFM_WINDOW_*: how the window forms put the directed pairs' costs together (default PAIR) */
    int32_t dense_joint;   /* tcsfm_refine_dense_window with S > 1 (default 1): the S forward pairs of a target share ONE inverse-
                              depth map and are solved JOINTLY (6S x 6S reduced camera system); 0: every forward pair refines its own
                              copy of the target depth (the round-2 behaviour)                                                  */
    float prior_init;      /* dense window mode under TCSFM_WINDOW_REFERENCE: options['l_depth_init_weight'] if options['l_depth_init'] else 0
                              (optimizer.py:89-90): weight of mean SSIM(current, initial sigmoid disparity of the target); default 0.1  */
    int32_t depth_param;   /* TCSFM_DEPTH_*: dense window mode under TCSFM_WINDOW_REFERENCE (default FULL)                             */
    float w_pose_consist;  /* pose window modes AND the dense window mode under TCSFM_WINDOW_REFERENCE, 6-DoF Gauss-Newton on the SE(3) chart:
                              0.1 if options['l_pose_consist'] else 0
                              (default 0, as the reference's drivers) -- w * mean |p_fwd + p_inv| over the S*B x 6 entries of the
                              reference's 6-vectors (optimizer.py:95-96).  Every pair gets the exact gradient w.r.t. its own pose (IRLS on
                              the L1 term, floor irls_eps) and the block-Jacobi majoriser of the curvature, its partner held at the
                              linearisation point; value and gradient pinned on reference autograd (golden G13 `full_pc`).  In the dense
                              mode the term enters the REDUCED pose systems (it does not depend on the maps): the forward pairs' diagonal
                              blocks of their target's joint system, the inverse pairs' own systems; tcsfm_linearize_dense_window exports
                              its value and gradient with the loss; queued calls that carry it are not merged                            */
    float w_smooth;        /* dense window mode under TCSFM_WINDOW_REFERENCE: options['l_smooth_weight'] if options['l_smooth'] else 0 (default
                              0, as the reference's drivers) -- w * get_smooth_loss(target disparity, target image) (optimizer.py:92-93,
                              losses.py:43-61: edge-aware L1 smoothness of the mean-normalised sigmoid disparity).  Exact gradient incl. the
                              normalisation's per-image constant (one more launch per linearisation: k_dref_smooth); curvature = the diagonal
                              majoriser of the edges' IRLS weights; pinned on reference autograd (golden G13 `fullinit_smooth`)           */
    int32_t free_source_depths; /* dense window mode under TCSFM_WINDOW_REFERENCE, either depth_param (default 0): 1 = the SOURCE depth maps
                              are unknowns as well, as in the reference's optimize_depth_pred (optimizer.py:194-198 optimises the disparities of
                              target AND sources; no prior on the sources).  Every inverse pair then is a group of its own -- its pose and the
                              source map it back-projects, per-pixel Schur elimination as in a forward group of one source -- with the adjoint
                              of the forward pair's samples of that map in its gradient (tcsfm_linearize_dense_window_sources); after every
                              step the forward pairs sample the new source maps.  depth_out's inverse slots return the refined source maps.  With
                              depth_param = TCSFM_DEPTH_QUARTER the unknowns are the reference's own leaves: quarter-resolution maps of target and sources */
} tcsfm_opts;

/* per-pair, per-linearisation statistics written by tcsfm_refine: [N][n_iters+1][TCSFM_NSTAT] fp32.
 * Row i < n_iters: the i-th linearisation (cost, photometric part, mask count, damping) and the pose it was evaluated at,
 * i.e. the trajectory of iterates (the analogue of the reference's stacked poses, train_mono.py:71-79).  Row n_iters:
 * Gauss-Newton -- the final pose, cost fields 0 (not evaluated); LM -- the cost check of the last trial step. */
enum { TCSFM_STAT_COST = 0, TCSFM_STAT_COST_PHOTO = 1, TCSFM_STAT_NMASK = 2, TCSFM_STAT_LAMBDA = 3,
       TCSFM_STAT_POSE = 4 /* ..9: the 6-vector the row was evaluated at */, TCSFM_NSTAT = 10 };

/* ---- overlapping arguments -------------------------------------------------------------------
 * Every array argument of a call is a range of bytes (its pointer and the extent its description gives).  A call whose OUTPUT range
 * overlaps an input range or another output range of the SAME call -- partially counts -- is REFUSED with TCSFM_E_ARG before anything is
 * enqueued: tcsfm_last_error() says "<entry>: <out> overlaps <other>", no buffer is touched and the handle stays usable.  The exceptions
 * below are HONOURED: the call returns exactly the bits of the same call on disjoint copies.  NULL arguments and zero-length arrays
 * take part in nothing; inputs may share memory with each other freely.
 *   1. Poses.  pose_out at the base address of pose_in (pose_init for the sequence calls): the initial poses are consumed by the first
 *      launch, the refined ones are written by the last (the sequence calls hold pose_init on the device before the first window is
 *      issued and write pose_out after the last has finished).
 *   2. Dense depth.  depth_out of tcsfm_refine_dense / tcsfm_refine_dense_window (and the _async / _queued forms) may overlap depth_t
 *      or depth_s in any way: the call then leaves depth_out alone until a final stream-ordered copy from the work buffer (a queued
 *      call of this kind is not merged: it flushes what is waiting and runs at once).  depth_out over any other input is refused.
 *   3. Element-wise entries, output at the base address of one input -- where a thread loads everything it needs from the elements it
 *      owns before its first store: the pairs of tcsfm_disp_to_depth and tcsfm_disp_to_depth_backward below.  Every other operator
 *      gathers from neighbours or from projected positions (SSIM, smoothness, warp, photometric) or re-reads an input after a store
 *      (window loss): in-place forms of those are refused, not patched with scratch copies.
 *   4. opts.host_ptrs != 0.  The library stages the arrays: inputs go up before the first launch, outputs come back after the last,
 *      so an output may overlap an INPUT of the call in any way.  Two outputs sharing memory are refused in every mode.  The sequence
 *      calls always take host pointers but STREAM them (frames go up while results come back): only item 1 applies to them.
 *      (A NULL `depths` of a sequence call -- the attached depth network's case -- takes part in nothing, as every NULL argument does.)
 *   5. Overlap between the arguments of two DIFFERENT calls (queued calls waiting for their flush, calls on different lanes) is
 *      outside this contract: the caller's buffers must stay valid and unchanged until the calls that use them have completed.
 * The honoured pairs, entry by entry (`=`: same base address, `~`: any overlap; device pointers):
 *   tcsfm_disp_to_depth: scaled_disp = disp, depth = disp
 *   tcsfm_disp_to_depth_backward: g_disp = disp, g_disp = g_scaled, g_disp = g_depth
 *   tcsfm_refine: pose_out = pose_in
 *   tcsfm_refine_window: pose_out = pose_in
 *   tcsfm_refine_window_async: pose_out = pose_in
 *   tcsfm_refine_window_queued: pose_out = pose_in
 *   tcsfm_refine_window_scale_queued: pose_out = pose_in
 *   tcsfm_refine_dense: pose_out = pose_in, depth_out ~ depth_t, depth_out ~ depth_s
 *   tcsfm_refine_dense_window: pose_out = pose_in, depth_out ~ depth_t, depth_out ~ depth_s
 *   tcsfm_refine_dense_window_async: pose_out = pose_in, depth_out ~ depth_t, depth_out ~ depth_s
 *   tcsfm_refine_dense_window_queued: pose_out = pose_in, depth_out ~ depth_t, depth_out ~ depth_s
 *   tcsfm_refine_sequence: pose_out = pose_init
 *   tcsfm_refine_dense_sequence: pose_out = pose_init
 * (end of the honoured pairs; tcsfm_odometry_sequence takes no initial poses.)  The parameter tables of the networks and of the
 * optimiser (skips_out[5], d_skips[5], grads[], conv_w_g[7] ..., params[]) contribute one range per non-NULL element; the optimiser's
 * parameters are outputs of every step (two tensors of one optimiser must not share memory, a gradient must not lie on a parameter).
 * tcsfm_frames_from_u8 declares its two arrays `const void *src` / `void *dst` (bytes in, floats out) and enforces its one rule itself:
 * dst overlapping src in any way is refused with "tcsfm_frames_from_u8: dst overlaps src"; nothing about it is honoured.  While a U8
 * format is set (tcsfm_sequence_frame_format) the `frames` range of a sequence call is T*3*H*W bytes, not floats -- T*3*src_h*src_w
 * bytes with a frame source set (tcsfm_sequence_frame_source).  tcsfm_resize_u8 is declared and behaves like tcsfm_frames_from_u8:
 * "tcsfm_resize_u8: dst overlaps src".  tcsfm_disp_post_process and tcsfm_depthnet_disp_for_eigen are declared the same way (float32 in,
 * float64 out) and honour nothing either: "tcsfm_disp_post_process: out overlaps l_disp" (or r_disp_mirrored),
 * "tcsfm_depthnet_disp_for_eigen: out overlaps imgs".  So are tcsfm_depth_eval ("tcsfm_depth_eval: metrics_out overlaps disp" or gt) and
 * tcsfm_sequence_depth_eval, whose two arrays are the host's ("tcsfm_sequence_depth_eval: metrics_out overlaps gt"). */

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Allocates all device scratch for up to max_pairs directed pairs of H x W images on `device`.
 * Nothing in the reference corresponds to this: PyTorch owns memory there (optimizer.py:15-27).
 * Frame sizes: 4 <= H, W <= 16384, and every mode takes every such size, ragged against any tile grid -- the joint and
 * reference-loss dense modes included; the one further restriction is the quarter-resolution unknown's (o->depth_param =
 * TCSFM_DEPTH_QUARTER: H and W multiples of 4, otherwise the call returns TCSFM_E_ARG). */
int tcsfm_create(tcsfm_handle *out, int device, int H, int W, int max_pairs);
void tcsfm_destroy(tcsfm_handle h);
const char *tcsfm_last_error(tcsfm_handle h); /* h may be NULL: last create() error */
/* Run on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  NULL is HIP's legacy default
 * stream (stream 0), which is what PyTorch's default stream is.  A fresh handle runs on its own non-blocking stream;
 * tcsfm_use_own_stream() switches back to it. */
int tcsfm_set_stream(tcsfm_handle h, void *hip_stream);
int tcsfm_use_own_stream(tcsfm_handle h);
int tcsfm_synchronize(tcsfm_handle h);
void tcsfm_default_opts(tcsfm_opts *o);
/* bytes of HBM traffic the algorithm must move per pixel per pair per linearisation: 32 */
int tcsfm_algorithmic_bytes_per_pixel(const tcsfm_opts *o);

/* ---- reference-function drop-ins (a1, a5, a7, a12) -------------------------------------------- */

/* disp_to_depth, utils/learning_helpers.py:77-86.  n elements; scaled/depth may be NULL.  Either output may sit on disp ("overlapping
 * arguments"); the two outputs must not share memory. */
int tcsfm_disp_to_depth(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, float *scaled_disp, float *depth);

/* SSIM_Loss.forward(x, y), losses.py:27-41: `planes` = N*C images of H x W each (reflect pad 1, 3x3 means, clamp). */
int tcsfm_ssim(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, float *out);

/* get_smooth_loss(disp, img), losses.py:43-61: edge-aware smoothness of the mean-normalised disparity, disp [N,1,H,W],
 * img [N,3,H,W] -> one scalar (host double; the call synchronises the stream).  Off by default in the reference
 * (options['l_smooth'], run_sequential_optimization.py:87); a logging quantity here, not a term of the Gauss-Newton cost. */
int tcsfm_smooth_loss(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, double *loss_out);

/* backward of disp_to_depth (utils/learning_helpers.py:77-86 under autograd, optimizer.py:241): scaled = a + b disp, depth = 1 / scaled,
 * a = 1 / max_depth, b = 1 / min_depth - a.  The cotangents of scaled_disp and depth (a NULL one is absent and costs nothing; at least
 * one must be given) -> g_disp = b (g_scaled - g_depth / scaled^2), n elements; `scaled` is recomputed as the forward forms it.  g_disp may
 * sit on any one of the three inputs ("overlapping arguments"). */
int tcsfm_disp_to_depth_backward(tcsfm_handle h, const tcsfm_opts *o, int64_t n, const float *disp, const float *g_scaled, const float *g_depth,
        float *g_disp);

/* backward of SSIM_Loss.forward (losses.py:27-41 under autograd; l_depth_init, optimizer.py:90): x, y and the cotangent of the output,
 * `planes` images of H x W each -> the gradients with respect to x and to y (a NULL one is not wanted; at least one must be given).
 * One gather kernel with the reflect-padding multiplicity, no atomics: bit-reproducible, and an output requested alone has the bits it
 * has next to the other.  The clamp of losses.py:41 passes its gradient on the closed interval [0, 1] (torch's convention). */
int tcsfm_ssim_backward(tcsfm_handle h, const tcsfm_opts *o, int planes, const float *x, const float *y, const float *g_out, float *g_x,
        float *g_y);

/* get_smooth_loss (losses.py:43-61; l_smooth, optimizer.py:93) without leaving the device: loss_out is ONE float and stats_out [N,3]
 * doubles (per image: mean disparity, sum of the x terms, sum of the y terms -- what tcsfm_smooth_loss_backward needs), both in device
 * memory (host memory under opts.host_ptrs).  With device pointers the call neither synchronises the stream nor copies to the host: it
 * can be captured.  The value is tcsfm_smooth_loss's to the rounding of a float (the same partial sums, added per image). */
int tcsfm_smooth_loss_device(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, float *loss_out,
        double *stats_out);

/* backward of get_smooth_loss (losses.py:43-61 under autograd) with respect to disp: disp, img, the stats of tcsfm_smooth_loss_device
 * on the same inputs and the cotangent of the scalar (one float, device memory unless opts.host_ptrs) -> g_disp [N,1,H,W].  sgn(0) = 0
 * on an edge between equal disparities; the coupling through the per-image mean is included; img takes no gradient.  One gather kernel. */
int tcsfm_smooth_loss_backward(tcsfm_handle h, const tcsfm_opts *o, int N, const float *disp, const float *img, const double *stats,
        const float *g_loss, float *g_disp);

/* The window loss of the reference's epoch loop, optimizer.py:47-86, as one reduction: the forward term (with `argmin`: the per-pixel
 * minimum over the S sources, weighted by source 0's weight map; without: 0.25 x the mean over all S B maps), 0.25 x the inverse term
 * when `inverse`, and the depth-consistency terms opts.w_dc (1 - mean weight_mask) of the forward and, with `inverse`, the inverse side
 * (w_dc = 0: off).  opts.automask applies the auto-mask (forward: diff_min < min_s auto_err, under `argmin` only; inverse: auto_mask).
 * Every map is [S B,1,H,W], source-major as tcsfm_solve_pose_iteratively's callers stack them; 1 <= S <= 4.  fwd_auto_err is read under
 * argmin && automask only, inv_auto_mask under automask only, the inverse maps when `inverse` only: NULL is accepted where a map is not
 * read.  loss_out is ONE float and stats_out seven doubles N1, D1, N2, D2, W1, W2, n (numerator and denominator of the forward and of
 * the inverse term, the sums of the two weight maps, the element count S B H W): what tcsfm_window_loss_backward needs.  Both are
 * device memory (host memory under opts.host_ptrs); with device pointers the call neither synchronises nor copies to the host: it can
 * be captured.  Products, sums and the final combination are in double with one rounding at the store; no atomics and a grid that
 * depends on the shape only: bit-reproducible.  A zero denominator gives nan / inf as the reference's expression does.  Ties of the
 * minimum go to the lowest source index. */
int tcsfm_window_loss(tcsfm_handle h, const tcsfm_opts *o, int B, int S, int argmin, int inverse, const float *fwd_diff, const float *fwd_valid,
        const float *fwd_weight, const float *fwd_auto_err, const float *inv_diff, const float *inv_valid, const float *inv_weight,
        const float *inv_auto_mask, float *loss_out, double *stats_out);

/* backward of tcsfm_window_loss (optimizer.py:47-86 under autograd): the same inputs, the stats of the forward call and the cotangent
 * of the scalar (one float) -> the gradients with respect to the forward and inverse diff_img and weight_mask, each [S B,1,H,W] (a NULL
 * one is not wanted; at least one must be given).  The masks and auto_err take no gradient.  One element-wise launch that recomputes
 * the minimum, its source and the validity; each value is evaluated in double and rounded once, and an output requested alone has the
 * bits it has next to the others.  Without `inverse` the two inverse gradients are exact zeros. */
int tcsfm_window_loss_backward(tcsfm_handle h, const tcsfm_opts *o, int B, int S, int argmin, int inverse, const float *fwd_diff,
        const float *fwd_valid, const float *fwd_weight, const float *fwd_auto_err, const float *inv_diff, const float *inv_valid,
        const float *inv_weight, const float *inv_auto_mask, const double *stats, const float *g_loss, float *g_fwd_diff,
        float *g_fwd_weight, float *g_inv_diff, float *g_inv_weight);

/* inverse_warp2(src, depth_t, depth_s, -pose, K), models/stn.py:234-273.
 * Outputs (any may be NULL): img_rec [N,3,H,W], valid [N,1,H,W], proj_depth, comp_depth [N,1,H,W]. */
int tcsfm_warp(tcsfm_handle h, const tcsfm_opts *o, int N, const float *src, const float *depth_t, const float *depth_s,
               const float *pose, const float *K, float *img_rec, float *valid, float *proj_depth, float *comp_depth);

/* backward of tcsfm_warp (models/stn.py:234-273 under autograd): the inputs of tcsfm_warp and the cotangents of img_rec, proj_depth and
 * comp_depth (each may be NULL = zero) -> the gradients with respect to depth_t, depth_s [N,1,H,W] and to THIS call's `pose` argument
 * [N,6] (each may be NULL = not wanted; what is not wanted is not computed).  `valid` is not differentiable; the image and the
 * intrinsics take no gradient.  Every requested output is fully written (zeros where nothing flows) and is bit-reproducible: the
 * bilinear cell, the out-of-range sentinel and the Z clamp are recomputed exactly as tcsfm_warp takes them. */
int tcsfm_warp_backward(tcsfm_handle h, const tcsfm_opts *o, int N,
        const float *src, const float *depth_t, const float *depth_s, const float *pose, const float *K,
        const float *g_rec, const float *g_proj_depth, const float *g_comp_depth,
        float *d_depth_t, float *d_depth_s, float *d_pose);

/* backward of the residual assembly behind tcsfm_photometric's differentiable outputs (train_mono.py:84-92, helpers.py:8-23 under
 * autograd), the kernel alone:  diff = mean_c(w_l1 clamp|rec - tgt| + w_ssim SSIM(tgt, rec)),  weight = 1 - clamp(|cd - pd| / (cd + pd)).
 * tgt, img_rec [N,3,H,W], proj_depth, comp_depth [N,1,H,W] and the cotangents of diff and weight [N,1,H,W] (each may be NULL = zero)
 * -> the gradients with respect to img_rec, proj_depth and comp_depth (each may be NULL = not wanted).  A requested output is fully
 * written; without the cotangent that feeds it, it is zeroed and no kernel is launched.  torch's conventions: sgn(0) = 0, a clamp
 * passes its gradient on the closed interval.  One gather kernel, no atomics: bit-reproducible.  w_l1, w_ssim from opts. */
int tcsfm_photometric_maps_backward(tcsfm_handle h, const tcsfm_opts *o, int N,
        const float *tgt, const float *img_rec, const float *proj_depth, const float *comp_depth,
        const float *g_diff, const float *g_weight,
        float *g_rec, float *g_proj_depth, float *g_comp_depth);

/* backward of tcsfm_photometric's differentiable outputs: its inputs and the cotangents of diff, weight [N,1,H,W] and img_rec
 * [N,3,H,W] (each may be NULL = zero) -> the gradients with respect to depth_t, depth_s [N,1,H,W] and to THIS call's `pose` argument
 * [N,6] (the reference's convention, as in tcsfm_photometric; each may be NULL = not wanted).  The warp is run forward into the handle's
 * scratch, then the assembly's backward, then the launches of tcsfm_warp_backward.  The masks, the images and the intrinsics take no
 * gradient; opts.depth_is_disp is refused as in tcsfm_warp_backward.  Bit-reproducible. */
int tcsfm_photometric_backward(tcsfm_handle h, const tcsfm_opts *o, int N,
        const float *tgt, const float *src, const float *depth_t, const float *depth_s, const float *pose, const float *K,
        const float *g_diff, const float *g_weight, const float *g_img_rec,
        float *d_depth_t, float *d_depth_s, float *d_pose);

/* The coupled-iteration input assembly of solve_pose_iteratively, train_mono.py:73-77, fused into the warp:
 * posenet_in [N,6,H,W] = (tgt * valid_mask, img_rec) for the next PoseNet call; valid [N,1,H,W] optional. */
int tcsfm_warp_posenet_input(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                             const float *depth_s, const float *pose, const float *K, float *posenet_in, float *valid);

/* compute_photometric_error, optimization_experiments/helpers.py:8-23 == per-pair residual assembly of
 * solve_pose_iteratively, train_mono.py:82-100.  Outputs (any may be NULL), all [N,1,H,W] except img_rec:
 * diff (diff_img), valid (warp validity, stn.py:268-269), weight (weight_mask), auto_err (auto_mask_error),
 * auto_mask (diff < auto_err), img_rec [N,3,H,W]. */
int tcsfm_photometric(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                      const float *depth_s, const float *pose, const float *K, float *diff, float *valid, float *weight,
                      float *auto_err, float *auto_mask, float *img_rec);

/* The scalar generate_loss_surface sweeps, optimization_experiments/plot_loss_surface.py:31-33,45-47:
 * cost[i] = sum(diff*mask*weight)/sum(mask) (+ w_dc*mean(1-weight)) of ONE pair (first pair of the arrays)
 * under P candidate poses [P,6].  cost_out: P doubles (host pointer always). */
int tcsfm_loss_surface(tcsfm_handle h, const tcsfm_opts *o, const float *tgt, const float *src, const float *depth_t,
                       const float *depth_s, const float *K, int P, const float *poses, double *cost_out);

/* ---- the Gauss-Newton / LM engine (new functionality; north star) ------------------------------ */

/* One linearisation of N pairs at the given poses (and log depth-scales, may be NULL): normal equations
 * for parity tests.  np = 6 or 7 per o->refine.  Host outputs (doubles): Hmat [N,np,np], g [N,np],
 * stats [N,4] = cost, cost_photo, cost_dc, n_mask. */
int tcsfm_linearize(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                    const float *depth_s, const float *pose, const float *log_scale, const float *K,
                    double *Hmat, double *g, double *stats);

/* Window form of tcsfm_linearize: ONE linearisation of the 2*S*B directed pairs of a window (layouts of tcsfm_refine_window)
 * at the given poses, under o->argmin / o->window_rule.  Host outputs (doubles): Hmat [2SB,np,np], g [2SB,np],
 * stats [2SB,4] = cost, cost_photo, cost_dc, n_mask -- under TCSFM_WINDOW_REFERENCE the pairs' costs add up to
 * compute_optimization_loss (optimizer.py:47-86) and g is its gradient w.r.t. each pair's left SE(3) perturbation. */
int tcsfm_linearize_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                           const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *log_scale,
                           double *Hmat, double *g, double *stats);

/* Refine N directed pairs: replaces the epoch loop of DepthOptimizer.optimize_window
 * (optimization_experiments/optimizer.py:217-274) for the pose / pose+scale unknowns with
 * o->n_iters Gauss-Newton (or LM) iterations on the reference's residual.
 *   pose_in       [N,6] initial pose (e.g. PoseNet output);  pose_out [N,6] refined pose (may sit on pose_in: "overlapping arguments" above)
 *   log_scale_in  [N] or NULL (start at 0), log_scale_out [N] or NULL: only read/written when refine == POSE_SCALE
 *   stats_out     [N,n_iters+1,TCSFM_NSTAT] or NULL */
int tcsfm_refine(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                 const float *depth_s, const float *K, const float *pose_in, const float *log_scale_in, float *pose_out,
                 float *log_scale_out, float *stats_out);

/* Window form of tcsfm_refine: the call surface of solve_pose_iteratively / optimize_window (train_mono.py:41-62,
 * optimizer.py:136-160): B target frames with S source frames each, given ONCE --
 *   tgt [B,3,H,W], srcs [S,B,3,H,W], depth_t [B,1,H,W], depth_s [S,B,1,H,W], K [B,3,3] --
 * and refined as 2*S*B directed pairs in the reference's stacked order (train_mono.py:54-62): pair s*B+b reconstructs
 * target b from source s (forward), pair S*B+s*B+b the reverse (inverse).  pose_in / pose_out [2*S*B,6],
 * log_scale_* [2*S*B] or NULL, stats_out [2*S*B,n_iters+1,TCSFM_NSTAT] or NULL, as in tcsfm_refine.
 * With o->argmin and S > 1 the forward pairs of a target use the reference's per-pixel min over the sources
 * (compute_optimization_loss, optimizer.py:47-69): at every linearisation a pixel counts only for the source with the
 * smallest photometric error there, under the union validity mask and the auto-mask of the minima.
 * With the default o->window_rule = TCSFM_WINDOW_PAIR each directed pair is its own least-squares problem: normalised by ITS OWN
 * count of selected pixels, with ITS OWN depth-consistency weight map; TCSFM_WINDOW_REFERENCE minimises the reference's scalar
 * loss itself -- batch-summed normalisers, the weight map of source 0 on every forward pixel (optimizer.py:69), 0.25 x the
 * inverse term -- see the enum above (golden G13).  The selection (which pixels count, for which source) is the reference's
 * under both rules and is pinned on its own maps (golden G4).
 * The handle must have been created with max_pairs >= 2*S*B. */
int tcsfm_refine_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                        const float *depth_t, const float *depth_s, const float *K, const float *pose_in,
                        const float *log_scale_in, float *pose_out, float *log_scale_out, float *stats_out);

/* Dense mode (BASELINE config 5): refine the 6-DoF pose AND the per-pixel inverse depth of the target of N directed
 * pairs: o->n_iters Gauss-Newton iterations, exact depth gradient (equal to reference autograd d loss / d depth), per-pixel
 * Schur elimination of the depth block, 6x6 reduced pose system, back-substitution.  depth_t is the initial target depth
 * (or sigmoid disparity with depth_is_disp); depth_out [N,1,H,W] receives the refined DEPTH.  w_dc must be 0 (the depth prior of
 * opts.prior_depth regularises instead).  With TCSFM_SOLVER_LM the pose block is Marquardt-damped and a trial that does not
 * lower the cost is rolled back -- pose AND depth map -- before the step is recomputed from the accepted linearisation.
 * pose_out may sit on pose_in, and depth_out may overlap depth_t or depth_s in any way ("overlapping arguments"). */
int tcsfm_refine_dense(tcsfm_handle h, const tcsfm_opts *o, int N, const float *tgt, const float *src, const float *depth_t,
                       const float *depth_s, const float *K, const float *pose_in, float *pose_out, float *depth_out,
                       float *stats_out);

/* Window form of tcsfm_refine_dense (the `optimize_depth_pred` mode of optimize_window with its default options,
 * optimizer.py:194-198 + 47-69): B targets x S sources given once as in tcsfm_refine_window; depth_out [2*S*B,1,H,W] in the
 * stacked pair order.
 *   JOINT (o->dense_joint, the default, S = 2 or 3; S >= 4 in this mode runs the per-pair copies below): the reference optimises ONE disparity per frame that every term of the loss
 *     sees (optimizer.py:235-247).  The S forward pairs of target b share one inverse-depth map; unknowns per target = S poses +
 *     the map; cost = the forward term of the reference's loss (min over the sources under o->argmin, or every valid source
 *     without it, :71-73) with every pixel weighted by the depth-consistency map of the source it counts for, + the depth prior.
 *     (optimizer.py:69 multiplies every pixel by the map of source 0; with the depth as an unknown that makes the depth of a pixel
 *     whose SOURCE-0 sample touches the zero padding depend chaotically on the fifth digit of source 0's pose although another
 *     source won it -- measured, DESIGN.md section 2 -- so o->window_rule does not apply here; the pose modes offer it.)
 *     Exact gradient (= reference autograd of that cost w.r.t. the poses AND the shared depth, golden G13 `fwd_ownw`);
 *     per-pixel Schur elimination of the depth -> ONE reduced camera system of 6S x 6S per target (12 x 12 for the KITTI
 *     window; its off-diagonal blocks vanish identically under argmin, where every pixel counts for exactly one source),
 *     back-substitution once per target pixel.  LM accepts / rejects all S poses and the map together.  The S forward slots of
 *     depth_out hold the same refined map; stats rows of the forward pairs: [joint cost of the target, own share, own mask
 *     count, lambda, iterate].  The inverse pairs refine their pose and the depth of THEIR target (source frame (s,b)) as before.
 *   PER-PAIR COPIES (o->dense_joint = 0, or S = 1 where the two coincide): every directed pair refines ITS OWN copy of its
 *     target's depth; with o->argmin the forward pairs use the min over the sources at the current poses and depth copies.
 *   REFERENCE LOSS (o->window_rule = TCSFM_WINDOW_REFERENCE; S = 1 .. 4 -- the five-frame window t-2 .. t+2 included --, Gauss-Newton;
 *     round 4; S >= 5 returns TCSFM_E_ARG): the scalar that is minimised is
 *     the reference's compute_optimization_loss as optimize_depth_pred sees it (optimizer.py:47-90):
 *       c_f / K_f sum M_s W_x diff_s  (forward term: K_f summed over the call's B targets; W_x = the weight map of SOURCE 0 on every
 *                                      selected pixel under o->argmin, c_f = 1; without argmin W_x = W_s, c_f = 0.25, no auto-mask)
 *       + 0.25 / K_i sum M_i W_i diff_i  (inverse pairs, K_i summed over all of them)
 *       + o->w_dc / (S B HW) sum (dd_fwd + dd_inv)  (depth consistency of both directions; w_dc > 0 is allowed in this mode)
 *       + o->prior_init / (B HW) sum SSIM(sigma, sigma_0)  (l_depth_init: SSIM between the target's current and initial sigmoid
 *                                      disparity, sigma = (1/depth - 1/max_depth) / (1/min_depth - 1/max_depth))
 *     Unknowns: the poses of all 2 S B directed pairs and ONE inverse-depth map per target; the source depth maps stay at their
 *     input unless o->free_source_depths is set (the reference lets them drift too, with no prior on them: see that field).  The target depth enters the forward pairs as the
 *     back-projected depth and the inverse pairs as the depth they SAMPLE (stn.py:271): the gradient contains both -- the second as
 *     the adjoint of the bilinear sample, scattered with 64-bit fixed-point atomics (order-independent: results stay bit-
 *     reproducible) -- and equals reference autograd w.r.t. every pose and the shared depth (golden G13 `full`, `fullinit`; see
 *     tcsfm_linearize_dense_window).  Curvature: the joint dense model + the IRLS curvature of the depth-consistency terms + a
 *     diagonal model of the 3x3-coupled prior, w / r^2 (1/d2 + 1/(9 d1)) with the pixel's own SSIM denominators; the sampled-depth
 *     terms are gradient-only.  The inverse pairs take 6 x 6 pose steps under the window rule.  After every step the new map also
 *     replaces the depth the inverse pairs sample.  depth_out: the S forward slots hold the refined map, the inverse slots the
 *     source depths (unchanged; refined under o->free_source_depths).  stats rows of the forward pairs: [forward group's loss (forward + its depth consistency + prior),
 *     own share, own mask count, lambda, iterate]; of the inverse pairs: as tcsfm_refine_window under the rule.
 *     LAUNCHES (round 5): with the source maps fixed an iteration is FOUR dependent launches -- one over all 2 S B directed pairs
 *     (the forward pairs' mask / min-over-sources selection and its count K_f; the inverse pairs' 6 x 6 systems, K_i and the adjoint
 *     scatter, whose two parts are summed without their factors so that no count has to precede it), the joint kernel, one launch
 *     that solves the targets' 6S x 6S systems and the inverse pairs' 6 x 6 systems, the back-substitution (five with the quarter-
 *     resolution unknown) -- and a call issues no memset or copy: csrc/dense_ref_kernel.h.  (A call whose depth_out overlaps depth_t or
 *     depth_s -- honoured, "overlapping arguments" -- ends with one copy: its depth_out is written last.) */
int tcsfm_refine_dense_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                              const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out,
                              float *depth_out, float *stats_out);

/* ONE linearisation of tcsfm_refine_dense_window's REFERENCE-LOSS mode at `pose` and `depth_t` (nothing is updated): the loss and its
 * exact gradients, for pinning against the reference's loss and autograd (golden G13) -- the dense counterpart of
 * tcsfm_linearize_window.  S = 1 .. 4 (S >= 5: TCSFM_E_ARG).  Outputs (HOST pointers, float64): scal_out [8] = loss, forward group (forward term + its depth
 * consistency + prior), inverse photometric term, inverse depth-consistency term, K_f, K_i, a_f = c_f / K_f, the l_pose_consist term
 * (o->w_pose_consist; part of the loss and of g_pose_out, golden G13 `full_pc`);
 * g_pose_out [2*S*B][6] = d loss / d (left SE(3) perturbation of every directed pair's warp transform) in the stacked pair order;
 * g_rho_out [B][H*W] float32 (device or host pointer as o->host_ptrs says) = d loss / d (inverse depth of target b).
 * depth0 [B,1,H,W] (same kind of pointer as depth_t; DEPTH, not disparity) or NULL: the centre of the l_depth_init prior -- the
 * reference's self.target_disparity, the map the optimisation started from (optimizer.py:156,90); NULL: depth_t itself (the state at
 * the first epoch, where the prior and its gradient vanish). */
int tcsfm_linearize_dense_window(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                 const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *depth0,
                                 double *scal_out, double *g_pose_out, float *g_rho_out);

/* The same linearisation with one more output: g_rho_src_out [S][B][H*W] float32 (kind of pointer as o->host_ptrs says) = d loss /
 * d (inverse depth of SOURCE map (s, b)) -- the depth maps tcsfm_refine_dense_window holds fixed, which the reference's optimize_depth_pred
 * optimises as well (optimizer.py:194-198: the quarter-resolution disparities of the target AND of every source are leaves).  A source
 * map is the back-projected depth of its inverse pair (local: photometric term through the SSIM window, the pair's own weight, its depth-
 * consistency term) and the depth its forward pair SAMPLES (stn.py:271: through that pair's depth-consistency term and the weight map it
 * provides -- source 0's multiplies every selected pixel under o->argmin, optimizer.py:69): both parts, the second as the adjoint of the
 * bilinear sample.  S = 1 .. 4 as there.  Equals reference autograd (golden G13 `full_grad_depth_s`; oracle: dref_source_depth_gradient).  With this every leaf
 * of the reference's loss has its exact gradient on the device; making the source maps unknowns of the Gauss-Newton step is not done. */
int tcsfm_linearize_dense_window_sources(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                         const float *depth_t, const float *depth_s, const float *K, const float *pose, const float *depth0,
                                         double *scal_out, double *g_pose_out, float *g_rho_out, float *g_rho_src_out);

/* ScaleRecovery.forward, models/dnet_layers.py:249-327 (the step right after the path in optimize_window,
 * optimizer.py:254-258): camera-height map |P.n| from 8-neighbour surface normals, ground mask, exact lower median of the
 * masked heights over the batch, scale = real_cam_height / median.  pad_to_batch mirrors the reference's padding of a short
 * batch with copies of image 0 (dnet_layers.py:307-311; pass config['minibatch'], or 0 for none).
 * scale_out [1]; optional: median_out [1], height_out / mask_out [N,1,H,W]. */
int tcsfm_scale_recovery(tcsfm_handle h, const tcsfm_opts *o, int N, const float *depth, const float *K, float real_cam_height,
                         int pad_to_batch, float *scale_out, float *median_out, float *height_out, float *mask_out);
/* operator: per-item scales of N depth maps, device pointers, on the handle's stream (asynchronous).  Item n's scale_out[n] and
 * median_out[n] are, bit for bit, what tcsfm_scale_recovery(h, o, 1, depth_n, K_n, real_cam_height, 0, ...) returns for that item
 * alone; count_out[n] is its number of ground pixels, and an item without any gets the quiet NaN in both.  Two launches per call,
 * whatever N: k_ground and k_median_frames (csrc/frame_scale_kernel.h: one workgroup per item runs the whole radix select), against
 * nine launches and a memset per tcsfm_scale_recovery call.  The arrays are declared void like tcsfm_scale_intrinsics': depth is
 * float [N,H*W], K float [N,9], scale_out / median_out float [N], count_out int32 [N].
 *   Refused with TCSFM_E_ARG (tcsfm_last_error says why; nothing is launched, the outputs keep their contents): a NULL depth, K or
 *   scale_out; N < 1 or N > max_pairs; H < 5 or W < 5 ("image too small", as tcsfm_scale_recovery); o->host_ptrs != 0 (a host caller
 *   has the sequence calls: tcsfm_sequence_scale); an output overlapping depth, K or another output ("overlapping arguments").
 *   The intrinsics are checked as tcsfm_scale_recovery checks them. */
int tcsfm_scale_recovery_frames(tcsfm_handle h, const tcsfm_opts *o, int N,
        const void *depth /* float [N,H*W] */, const void *K /* float [N,9] */, float real_cam_height,
        void *scale_out /* float [N] */, void *median_out /* float [N] or NULL */, int *count_out /* [N] or NULL */);

/* ---- PoseNet and the coupled pose loop ----------------------------------------
 * The reference's PoseNet (models/pose_models.py:88-147: seven weight-standardised stride-2 convolutions + GroupNorm(16) + ReLU,
 * 1x1 head, spatial mean, x 0.01) is evaluated `iterations` times per window inside solve_pose_iteratively (train_mono.py:64,77).
 * Here it runs as hand-written gfx950 kernels (fp32 matrix instructions, weight standardisation folded into the loaded weights,
 * GroupNorm + ReLU applied by the consuming layer), so that the whole coupled loop stays inside the library.
 *   tcsfm_posenet_create   activations for up to max_images samples of the handle's H x W
 *   tcsfm_posenet_load     HOST pointers to the parameters of the reference module, in its own layouts: conv_w[l] = conv{l+1}.0.weight
 *                          [cout,cin,k,k], conv_b[l] = conv{l+1}.0.bias [cout] (NULL: 0), gn_w / gn_b[l] = conv{l+1}.1.weight / .bias
 *                          [cout] (NULL: 1 / 0), head_w = pose_pred.weight [6,256(,1,1)], head_b = pose_pred.bias [6]
 *   tcsfm_posenet_forward  pose_model(imgs): imgs [N,6,H,W] (device) -> pose [N,6] (device).  The work split of the layers (K split,
 *                          channel blocks per wave) is chosen from the NUMBER OF IMAGES of the call -- two fixed regimes, N <= 4 and N > 4
 *                          -- and the K split fixes the summation order: results are bit-identical for every N within a regime and
 *                          agree to ~1e-6 relative across the two.  Consequence for the sequence calls below: the PoseNet poses of a
 *                          window depend, at the 1e-6 level, on whether its call holds up to 4 or more images (windows_per_call), and the
 *                          coupled loop's discrete warp-validity decisions can amplify that on individual windows (measured with random
 *                          weights: 3 of 199 windows at 1e-5 .. 1e-2, all others ~1e-6).
 *   tcsfm_solve_pose_iteratively   train_mono.py:41-81 for a window (layouts of tcsfm_refine_window): PoseNet on (tgt | src) /
 *                          (src | tgt), then num_iter-1 rounds of { inverse_warp2 with -pose; PoseNet on (tgt * valid | img_rec);
 *                          pose += correction }.  poses_out [2*S*B,6] = the last iterate; stacked_out [2*S*B,num_iter,6] optional
 *                          (the reference's stacked_poses).  Asynchronous on the handle's stream. */
typedef struct tcsfm_posenet tcsfm_posenet;
int tcsfm_posenet_create(tcsfm_handle h, int max_images, tcsfm_posenet **out);
void tcsfm_posenet_destroy(tcsfm_posenet *pn);
int tcsfm_posenet_load(tcsfm_posenet *pn, const float *const conv_w[7], const float *const conv_b[7], const float *const gn_w[7],
                       const float *const gn_b[7], const float *head_w, const float *head_b);
int tcsfm_posenet_forward(tcsfm_posenet *pn, int N, const float *imgs, float *pose_out);
int tcsfm_solve_pose_iteratively(tcsfm_handle h, tcsfm_posenet *pn, int num_iter, int B, int S, const float *tgt, const float *srcs,
                                 const float *depth_t, const float *depth_s, const float *K, float *poses_out, float *stacked_out);

/* ---- PoseNet: gradient with respect to the input ---------------------------------------------------
 * In the coupled loop every PoseNet call after the first reads (tgt * valid | img_rec), and img_rec is the warp of the source under
 * the current depths and pose: with the network's weights frozen (the reference's default test-time tuning mode) the depths reach
 * the poses through the network's INPUT.  These calls differentiate the network with respect to it (csrc/posenet_grad_kernel.h);
 * the parameters' gradient is the next section's.
 *   tcsfm_posenet_tape_size      floats of the tape of an N-image training forward.  Layout, layer after layer (l = 1..7, npix = oh ow
 *                                of the layer): raw [N][npix][cout] (the reduced convolution output + bias, NHWC), scsh [N][cout][2]
 *                                (GroupNorm scale = rstd gamma, shift = beta - mean scale), mean_rstd [N][16][2] (per group; rstd cannot
 *                                be had from scale where gamma is zero).  The images are not kept.  About 0.96 M floats per image at
 *                                192 x 640.
 *   tcsfm_posenet_forward_train  tcsfm_posenet_forward's launches unchanged (pose_out has its bits) + the tape (device, caller-owned,
 *                                16-byte aligned).
 *   tcsfm_posenet_backward       d_pose [N,6] -> d_imgs [N,6,H,W] (device, planar), with the instance's CURRENT weights (a
 *                                tcsfm_posenet_load between forward and backward is the caller's to prevent).  The ReLU decisions are
 *                                relu(raw * scale + shift) > 0 evaluated by one device function on the taped values; the forward's
 *                                in-register activation can differ from it only where the activation is within an ulp of zero.
 *                                No float atomics: results are bit-reproducible, and an image's gradient depends neither on the other
 *                                images of the call nor on N within a forward regime (N <= 4, N > 4).  The first call after a load
 *                                builds the transposed weight images and, once per instance, the gradient scratch.
 * Both run asynchronously on the handle's stream; N <= max_images. */
int tcsfm_posenet_tape_size(tcsfm_posenet *pn, int N, int64_t *floats_out);
int tcsfm_posenet_forward_train(tcsfm_posenet *pn, int N, const float *imgs, float *pose_out, float *tape);
int tcsfm_posenet_backward(tcsfm_posenet *pn, int N, const float *tape, const float *d_pose, float *d_imgs);

/* ---- PoseNet: gradient with respect to the parameters -----------------------------------------------
 * The reference's optimize_pose_weights_all mode (optimization_experiments/optimizer.py:187-189) puts the pose model's parameters
 * into the optimiser and backpropagates through solve_pose_iteratively into them (csrc/posenet_wgrad_kernel.h).
 *   tcsfm_posenet_load_device    tcsfm_posenet_load from DEVICE pointers (same layouts, same NULL conventions), asynchronous on the
 *                                handle's stream: no host staging and no synchronisation, so that a reload after every optimiser step
 *                                is cheap.  The prepared weights have the bits tcsfm_posenet_load gives for the same values; the
 *                                backward's transposed weight images are rebuilt at the next backward.  Both loads keep a copy of the
 *                                raw weights per owning instance (the chain rule through the weight standardisation reads it).
 *   tcsfm_posenet_param_backward one backward walk: every layer's dz feeds the data gradient and the parameter gradients.
 *                                imgs [N,6,H,W]: the images of the forward (the tape does not hold them), read only when
 *                                conv_w_g[0] is asked for.  d_imgs may be NULL (then layer 1's data gradient is skipped); when given
 *                                it has the bits of tcsfm_posenet_backward.  Every gradient pointer and every table may be NULL:
 *                                work nobody asked for is skipped, down to stopping the walk at the lowest layer that is needed.
 *                                Outputs (device) are OVERWRITTEN, in the reference's layouts: conv_w_g[l] [cout,cin,k,k] (the
 *                                gradient of the RAW weight, conv2d_wn's standardisation differentiated), conv_b_g / gn_w_g /
 *                                gn_b_g[l] [cout], head_w_g [6,256], head_b_g [6].  Exact fp32 products on the matrix cores, per-channel
 *                                and per-filter sums in double, no float atomics, fixed summation order: bit-reproducible.  Uses
 *                                the instance's CURRENT weights, as tcsfm_posenet_backward does.  N <= max_images; lane clones are
 *                                refused. */
int tcsfm_posenet_load_device(tcsfm_posenet *pn, const float *const conv_w[7], const float *const conv_b[7], const float *const gn_w[7],
                              const float *const gn_b[7], const float *head_w, const float *head_b);
int tcsfm_posenet_param_backward(tcsfm_posenet *pn, int N, const float *imgs, const float *tape, const float *d_pose, float *d_imgs,
                                 float *const conv_w_g[7], float *const conv_b_g[7], float *const gn_w_g[7], float *const gn_b_g[7],
                                 float *head_w_g, float *head_b_g);

/* ---- depth network --------------------------------------------------------------------------------
 * The reference's depth network (models/depth_w_access.py with num_scales = 1, the default of run_mono_training.py): a ResNet18
 * encoder on (x - 0.45) / 0.22 (conv1 7x7/2 + BN + ReLU -> skip 0, maxpool 3x3/2, layer1..layer4 of BasicBlocks -> skips 1..4;
 * BatchNorm with its running statistics) and a U-Net decoder (for i = 0..4: ELU(conv3x3_reflect(nearest_up2(x))) (+ skip 3-i for
 * i < 4), ELU(conv3x3_reflect(.)); then feature_convs.0 32 -> 8 ELU and predict_disps.0 8 -> 1 sigmoid).  Hand-written gfx950
 * kernels in exact fp32 (matrix instructions), BatchNorm folded into the weights at load time, padding / up-sampling /
 * normalisation / mirroring applied while the operands are gathered.  The work split of every layer depends on the handle's
 * H x W only: an image's outputs are bit-identical whatever N and whichever other images share the call.
 *   tcsfm_depthnet_create   activations for up to max_images images of the handle's H x W; refuses (TCSFM_E_ARG) an H or W that is
 *                           not a multiple of 32 (the reference's skip additions fail there too)
 *   tcsfm_depthnet_load     n HOST tensors of the reference module's state_dict: names[i], data host_ptrs[i] (float32, contiguous),
 *                           shape shapes[4 i .. 4 i + 3] (unused trailing dimensions 0).  Needs encoder.encoder.{conv1, bn1,
 *                           layer*.*.{conv1,bn1,conv2,bn2}, layer{2,3,4}.0.downsample.{0,1}}.*, depth_upconvs.{i}.1.conv.*,
 *                           iconvs.{i}.0.conv.*, feature_convs.0.0.conv.*, predict_disps.0.0.conv.*; other names (fc.*,
 *                           num_batches_tracked) are ignored.  A missing or mis-shaped tensor, and a num_scales > 1 model
 *                           (feature_convs.1.* present, or predict_disps.0 not 8 input channels), is refused; the error names the key.
 *   tcsfm_depthnet_encode   imgs [N,3,H,W] planar (device); flip != 0 mirrors every image horizontally first (bit-identical to the
 *                           mirrored input).  skips_out[k] (device, caller-owned) receive the encoder features NHWC:
 *                           skip k = [N, H >> (k+1), W >> (k+1), C_k], C = 64, 64, 128, 256, 512
 *   tcsfm_depthnet_decode   skips_in[5] in that layout (device) -> disp_out [N,1,H,W] (device)
 *   tcsfm_depthnet_forward  encode + decode with the instance's own skip buffers
 * All calls are asynchronous on the handle's stream, except load, which waits for the stream before it replaces the weights. */
typedef struct tcsfm_depthnet tcsfm_depthnet;
int tcsfm_depthnet_create(tcsfm_handle h, int max_images, tcsfm_depthnet **out);
void tcsfm_depthnet_destroy(tcsfm_depthnet *dn);
int tcsfm_depthnet_load(tcsfm_depthnet *dn, int n, const char *const names[], const float *const host_ptrs[], const int64_t *shapes);
int tcsfm_depthnet_encode(tcsfm_depthnet *dn, int N, const float *imgs, int flip, float *const skips_out[5]);
int tcsfm_depthnet_decode(tcsfm_depthnet *dn, int N, const float *const skips_in[5], float *disp_out);
int tcsfm_depthnet_forward(tcsfm_depthnet *dn, int N, const float *imgs, int flip, float *disp_out);

/* ---- depth network: training (weight tuning) ----------------------------------------------------------------------------
 * The exact fp32 gradient of the network above (BatchNorm with its running statistics, num_scales = 1) for the reference's
 * test-time weight tuning (Adam on the encoder's, all or the decoder's weights) and bottleneck tuning (gradients of the skips).
 * A training forward runs the kernels of tcsfm_depthnet_encode / _decode unchanged (its skips and disparity are bit-identical to
 * theirs) and keeps the activations the backward needs in a caller-owned tape; the backward reads the tape only.
 *   tcsfm_depthnet_load_device    as tcsfm_depthnet_load (same names, checks and refusals), but the tensors are DEVICE pointers and
 *                                 the call is asynchronous on the handle's stream: the parameters are copied into the instance and
 *                                 re-folded on the device (float64, the host fold's bits).  Call it again after every parameter
 *                                 update (an optimiser step); there is no host round trip.  The training calls below need it.
 *   tcsfm_depthnet_tape_size      floats of the encoder's and the decoder's tapes for N images (about 6.5 M and 17.4 M per 640 x 192
 *                                 image)
 *   tcsfm_depthnet_encode_train   imgs [N,3,H,W] -> skips_out[5] (as tcsfm_depthnet_encode, no mirroring) and the encoder tape
 *   tcsfm_depthnet_decode_train   skips_in[5] -> disp_out [N,1,H,W] and the decoder tape
 *   tcsfm_depthnet_decode_backward  decoder tape, d_disp [N,1,H,W] -> d_skips[k] [N,h_k,w_k,C_k] NHWC for every non-NULL entry (d_skips
 *                                 itself may be NULL), and the gradients of the n_grads decoder parameters names[i] (state_dict names)
 *                                 into grads[i] (device, reference layout [co,ci,kh,kw] / [c]); outputs are overwritten
 *   tcsfm_depthnet_encode_backward  encoder tape, d_skips[5] (NULL entries: zero) -> gradients of the n_grads encoder parameters
 * Only what is requested is computed: a parameter that is not named gets no kernel, and the data gradient stops below the lowest
 * requested parameter or skip.  Running statistics have no gradient (refused, as are unknown names and names of the other half).
 * Calls with N > max_images run in groups of max_images; weight gradients of the groups are summed in group order.  Weight gradients
 * are reduced in a fixed order (no float atomics): two calls on the same inputs give the same bits, and an image's skip gradients do
 * not depend on the other images of the call.  All calls are asynchronous on the handle's stream. */
int tcsfm_depthnet_load_device(tcsfm_depthnet *dn, int n, const char *const names[], const float *const dev_ptrs[], const int64_t *shapes);
int tcsfm_depthnet_tape_size(tcsfm_depthnet *dn, int N, int64_t *enc_floats, int64_t *dec_floats);
int tcsfm_depthnet_encode_train(tcsfm_depthnet *dn, int N, const float *imgs, float *const skips_out[5], float *tape);
int tcsfm_depthnet_decode_train(tcsfm_depthnet *dn, int N, const float *const skips_in[5], float *disp_out, float *tape);
int tcsfm_depthnet_decode_backward(tcsfm_depthnet *dn, int N, const float *tape, const float *d_disp, float *const d_skips[5], int n_grads,
                                   const char *const names[], float *const grads[]);
int tcsfm_depthnet_encode_backward(tcsfm_depthnet *dn, int N, const float *tape, const float *const d_skips[5], int n_grads,
                                   const char *const names[], float *const grads[]);

/* ---- the optimiser step of the weight-tuning loop ----------------------------------------------------------------------------
 * The reference builds torch.optim.Adam (or SGD) over the parameters its switches select and steps it once per epoch
 * (optimization_experiments/optimizer.py:211-214, 266-268); for every window it starts again from a deep copy of the network
 * (:176-191).  Here both live behind the C ABI (csrc/optim_kernel.h): a caller of this header runs the whole tuning loop without
 * PyTorch, and a window is started by putting the parameters back instead of copying the network.
 *   tcsfm_optim_create     an optimiser of `kind` over n tensors: params[i] is a DEVICE pointer to numel[i] contiguous floats, owned by
 *                          the caller and updated in place (4-byte alignment is enough; numel[i] = 0 is legal, does nothing, and its
 *                          pointer may be NULL).  The moments (Adam) and the snapshot live in arenas owned by the optimiser, zeroed
 *                          when they are allocated (the moments here, the snapshot's by the first tcsfm_optim_snapshot).
 *   tcsfm_optim_step       ONE launch over all tensors: grads[i] (device, numel[i] floats, read only) and lr[i] are per tensor and per
 *                          call, which covers parameter groups and schedules.  grads[i] = NULL skips tensor i and leaves its step
 *                          count where it was -- torch's rule for `p.grad is None` (for numel[i] = 0 nothing is read: any non-NULL
 *                          pointer counts as a gradient).  TCSFM_OPTIM_ADAM is torch.optim.Adam with weight_decay = 0 and
 *                          amsgrad = False, per element in fp32 without contraction:
 *                              m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 *                          with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t and t the tensor's own step count; 1 - beta1, 1 - beta2, lr / bc1
 *                          and sqrt(bc2) are computed in double and rounded once -- which is why lr, beta1, beta2 and eps are doubles,
 *                          as they are in torch: 1 - (float)0.999 is 1.3e-5 off 1 - 0.999, and exp_avg_sq with it.  TCSFM_OPTIM_SGD is torch.optim.SGD(params) as the
 *                          reference calls it (no momentum, no weight decay): p -= lr g; beta1, beta2 and eps are ignored.  One thread
 *                          owns an element: results are bit-reproducible.  Asynchronous on the handle's stream and launched plainly,
 *                          outside tcsfm_set_graph_replay's captures; the tables of a step are staged per step, so steps issued back to
 *                          back without a synchronisation each use their own gradient pointers and scalars (the gradient BUFFERS must
 *                          stay valid and unchanged until their step has run).  After a step the networks that read the parameters are
 *                          reloaded with tcsfm_depthnet_load_device / tcsfm_posenet_load_device: there is no other reload path.
 *   tcsfm_optim_snapshot   keep a copy of every parameter's current values (a later snapshot replaces it)
 *   tcsfm_optim_restore    parameters back to the snapshot's bits, moments zero, step counts zero: the optimiser and its tensors are
 *                          what they were when the snapshot was taken by a fresh optimiser.  Refused before the first snapshot.
 *                          Both are asynchronous on the handle's stream (the first snapshot allocates and waits for the stream once).
 *   tcsfm_optim_get_state  tensor i's exp_avg / exp_avg_sq (numel[i] floats each, to a host or a device pointer; NULL: not wanted; an SGD
 *                          optimiser has none and refuses non-NULL pointers) and its step count; waits for the handle's stream.
 * TCSFM_E_ARG with a tcsfm_last_error text for: n < 1, a NULL parameter of numel > 0, a negative numel, a pointer that is not 4-byte
 * aligned, an unknown kind, restore before snapshot.  Destroy the optimiser before its handle. */
typedef struct tcsfm_optim tcsfm_optim;
#define TCSFM_OPTIM_ADAM 0
#define TCSFM_OPTIM_SGD 1
int tcsfm_optim_create(tcsfm_handle h, int kind, int n, float *const params[], const int64_t numel[], tcsfm_optim **out);
void tcsfm_optim_destroy(tcsfm_optim *o);
int tcsfm_optim_step(tcsfm_optim *o, const float *const grads[], const double lr[], double beta1, double beta2, double eps);
int tcsfm_optim_snapshot(tcsfm_optim *o);
int tcsfm_optim_restore(tcsfm_optim *o);
int tcsfm_optim_get_state(tcsfm_optim *o, int i, float *exp_avg_out, float *exp_avg_sq_out, int64_t *step_out);

/* ---- lanes: several refinements in flight (streaming a sequence) ----------------------------------
 * The reference's driver refines one window after another (run_sequential_optimization.py:186-247: DataLoader batch -> H2D ->
 * optimize_window); consecutive windows do not depend on each other.  A B=1 refinement leaves the GPU idle between its short
 * kernels, and a host-pointer call spends more time on PCIe than on the refinement, so the library can keep several calls in
 * flight: lane k >= 1 owns a HIP stream and a full set of scratch buffers (lane 0 is the handle itself).
 *   tcsfm_set_lanes          1..8 lanes (allocates / frees the lanes' scratch; default 1).  MEASURED HAZARD (round 4, ROCm 7.2 / MI355X,
 *                            scripts/lane_order_probe.py): how well lanes overlap depends on the order in which the PROCESS created
 *                            its HIP streams.  A handle (and its lanes) created before the process's first device work -- an upload, a
 *                            kernel -- gives four lanes that are slower than one (10 000 against 13 500 frame-pairs/s; created after
 *                            the inputs are on the card: 22 000-26 000), and so do five or more lanes in any order: create the handle
 *                            after the first upload, and use at most four lanes.
 *   tcsfm_refine_window_async   tcsfm_refine_window on `lane`, asynchronously.  Device pointers (host_ptrs = 0): the lane first
 *                            waits for the work queued on the handle's stream at call time (the producers of the inputs).
 *                            Pinned host pointers (host_ptrs = 2): the copies run on the lane's stream -- they overlap the other
 *                            lanes' kernels -- and the call does NOT synchronise; read the outputs after tcsfm_lane_synchronize.
 *   tcsfm_lane_wait          the handle's stream waits (on the device, not the host) for the lane's last call
 *   tcsfm_lane_synchronize   the host waits for the lane's last call; reports a pending TCSFM_E_INTRINSICS of that lane
 *   tcsfm_lane_event         marks the current end of the lane's work with an event (owned by the library; one of a ring of 64
 *                            per lane, so a mark stays valid until 64 later marks of that lane) -- for callers that recycle
 *                            input buffers: tcsfm_stream_wait_event(stream, mark) makes e.g. their copy stream wait, on the
 *                            device, until the lane has consumed the buffer */
int tcsfm_set_lanes(tcsfm_handle h, int n_lanes);
/* Round 5: tcsfm_set_lanes MEASURES whether lanes pay in this process (24 B=1 refinements of the handle's own kernels on stand-in images, one
 * after the other on the handle's stream, then round-robin over all lanes; ~5 ms).  If they do not -- the hazard above -- the handle falls back: lane calls (tcsfm_refine_window_async, the
 * sequence calls, the merged sequences' second stream) run on the handle's own stream, one after the other, results unchanged, one line on
 * stderr.  tcsfm_lane_probe reports the outcome: *serial = 1 when the fallback is active, and the two probe times in ms.  The queued calls
 * (tcsfm_set_coalesce) keep the chip busy either way.  TCSFM_LANE_PROBE=0 in the environment skips the probe. */
int tcsfm_lane_probe(tcsfm_handle h, int *serial, float *one_stream_ms, float *two_streams_ms);
/* Debug aid (no reference counterpart; GPU AddressSanitizer is not available on the target pool): with TCSFM_DEBUG_GUARDS=1 in the environment
 * when the library is loaded, every device allocation of the library carries a 4 KB pattern band in front of it and behind it.  This call
 * synchronises the device, reads all bands back and reports (stderr, once per allocation) those a kernel wrote into: *n_allocations = live
 * allocations checked (-1: guards are off), *n_damaged = how many have a damaged band.  The GPU test suite runs with the guards on. */
int tcsfm_debug_check_guards(int *n_allocations, int *n_damaged);
/* ... and its self-test: writes four bytes past the end of a scratch allocation of its own and says whether the bands caught it
 * AND the check an entry runs over allocations it frees itself (tcsfm_debug_solve) counted that allocation and not an intact one
 * (*detected = 1 / 0; -1: guards are off) */
int tcsfm_debug_guard_selftest(int *detected);
/* Read-out of the PoseNet's most recent evaluation on `pn`, for layer-by-layer tests (layer = 1..7):
 *   tcsfm_debug_posenet_layer   raw_out [N, oh*ow, cout] (device, NHWC) = the layer's raw convolution output (+ bias; K-split partial sums
 *                               already combined), scsh_out [N, cout, 2] (device) = the GroupNorm (scale, shift) pairs its consumer applies:
 *                               a = relu(raw * scale + shift).  Either may be NULL.  N <= the images of that evaluation.  Ordered on the
 *                               handle's stream.
 *   tcsfm_debug_posenet_split   the layer's output size and the work split an N-image call uses (tcsfm_posenet_forward): output-channel
 *                               blocks of 16 per wave, K split, pixel blocks of 16 per wave.  Any out-pointer may be NULL. */
int tcsfm_debug_posenet_layer(tcsfm_posenet *pn, int layer, int N, float *raw_out, float *scsh_out);
int tcsfm_debug_posenet_split(tcsfm_posenet *pn, int layer, int N, int *oh, int *ow, int *nb, int *ks, int *pb);
/* Read-out of one layer (1..7) of a tcsfm_posenet_forward_train tape over N images: raw_out [N, oh*ow, cout], scsh_out [N, cout, 2],
 * mean_rstd_out [N, 16, 2] as taped, and act_out [N, oh*ow, cout] = the activation relu(raw * scale + shift) as the backward's own
 * device function evaluates it: act_out > 0 are exactly the ReLU decisions tcsfm_posenet_backward takes.  Any out-pointer may be NULL. */
int tcsfm_debug_posenet_tape_layer(tcsfm_posenet *pn, int N, const float *tape, int layer, float *raw_out, float *scsh_out,
                                   float *mean_rstd_out, float *act_out);
/* Read-out of the depth network's work split, for layer-by-layer tests: convolution `layer` in evaluation order (0 = conv1; per
 * BasicBlock conv1, conv2 and, in a stride-2 block, the 1x1 downsample; depth_upconvs.i, iconvs.i for i = 0..4; feature_convs.0 --
 * 33 - 2 = 31 entries, the max pool and the head have no split) -> kernel size, output size and the k_dn_conv instance it launches:
 * output-channel blocks of 16 per wave, pixel blocks of 16 per wave, waves sharing K.  conv1 runs k_dn_conv1 whatever nb / pb / kw
 * say.  The split depends on the handle's H and W only.  Any out-pointer may be NULL. */
int tcsfm_debug_depthnet_split(tcsfm_depthnet *dn, int layer, int *ks, int *oh, int *ow, int *nb, int *pb, int *kw);
int tcsfm_refine_window_async(tcsfm_handle h, int lane, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                              const float *depth_t, const float *depth_s, const float *K, const float *pose_in,
                              const float *log_scale_in, float *pose_out, float *log_scale_out, float *stats_out);
/* the dense mode (tcsfm_refine_dense_window) on a lane: same ordering rules */
int tcsfm_refine_dense_window_async(tcsfm_handle h, int lane, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                    const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out,
                                    float *depth_out, float *stats_out);
/* ---- coalesced calls (round 4): queued B-window calls of one shape run as ONE launch sequence ------------------------
 * The robust way of keeping the chip busy with small calls: lanes depend on how the runtime places their hardware queues (see
 * tcsfm_set_lanes), a merged launch sequence does not.  tcsfm_refine_window_queued takes the arguments of tcsfm_refine_window
 * (device pointers, no statistics outputs; tcsfm_refine_window_scale_queued carries the log depth-scales of TCSFM_REFINE_POSE_SCALE) and only NOTES the call; when `max_calls` calls of the same
 * shape (B, S) and options are waiting -- or at tcsfm_flush / tcsfm_synchronize, or when a call of another shape arrives -- they run as
 * one pack / (linearise, solve) x n_iters sequence over all their directed pairs on the handle's stream: the kernels reach every
 * call's own buffers through a pointer table (k_pack_coal) and every call's refined poses go to its own pose_out.  Per window the
 * results are the bits of tcsfm_refine_window run on its own (the kernels are batch-independent under TCSFM_WINDOW_PAIR; a call under
 * TCSFM_WINDOW_REFERENCE, whose loss couples the windows of a call, is never merged with others and runs at once).  The caller's
 * buffers must stay valid and unchanged until the flush that runs them has been issued AND has completed on the handle's stream.
 * ORDER (round 5): a queued call is never overtaken.  Every other entry point that puts work on the handle's stream (tcsfm_refine*,
 * tcsfm_refine_dense*, the *_async and sequence calls, tcsfm_linearize*, the drop-ins, the PoseNet calls) first launches what is
 * waiting and orders the handle's stream behind the merged sequences that ran on lanes; tcsfm_set_stream does so on the OLD stream
 * before it switches (the queued calls were noted behind that stream's producers), tcsfm_use_own_stream likewise, and tcsfm_destroy
 * runs what is waiting before it tears the handle down (queued calls are never dropped).
 *   tcsfm_set_coalesce(h, max_calls)   0 / 1: off (every queued call runs at once); up to 16; the handle's max_pairs bounds the merged
 *                                      sequence as well (2 S B x calls <= max_pairs)
 *   tcsfm_set_coalesce_lanes(h, n)     merged sequences alternate over n of the handle's streams (1: the handle's own, the default;
 *                                      up to the lanes of tcsfm_set_lanes): sequence k runs on lane k mod n, behind everything queued
 *                                      on the handle's stream when it is issued.  The 20-workgroup solve kernels of one sequence then
 *                                      overlap the chip-filling launches of the other (same bits).  A sequence issued on a lane is
 *                                      ordered before later work of the handle's stream only by tcsfm_flush / tcsfm_synchronize.
 *   tcsfm_flush(h)                     launch what is waiting (asynchronous) and order the handle's stream behind every merged sequence
 *                                      issued so far, whichever lane ran it
 *   tcsfm_coalesce_counts              launch sequences issued / calls they carried, since the handle was created */
int tcsfm_set_coalesce(tcsfm_handle h, int max_calls);
int tcsfm_set_coalesce_lanes(tcsfm_handle h, int n_streams);
int tcsfm_refine_window_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                               const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out);
/* the same with the depth-scale unknown (TCSFM_REFINE_POSE_SCALE): log_scale_in [2*S*B] or NULL (0), log_scale_out [2*S*B] or NULL */
int tcsfm_refine_window_scale_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                     const float *depth_t, const float *depth_s, const float *K, const float *pose_in,
                                     const float *log_scale_in, float *pose_out, float *log_scale_out);
int tcsfm_flush(tcsfm_handle h);
int tcsfm_coalesce_counts(tcsfm_handle h, int *batches, int *calls);
/* The dense counterpart (arguments of tcsfm_refine_dense_window, device pointers, no statistics): queued per-pair Gauss-Newton dense calls
 * with ONE source per target (S = 1, TCSFM_WINDOW_PAIR) of the same shape and options are merged like the pose calls -- every call's
 * refined poses and depth maps go to its own outputs, bit-identical to the call on its own.  Round 5: calls under TCSFM_WINDOW_REFERENCE (the
 * reference's own loss, optimizer.py:47-90; S <= 4, Gauss-Newton, fixed source maps, per-pixel or quarter-resolution unknown) are merged as
 * well: that loss couples the windows of ONE call through its batch normalisers, so inside the merged sequence every call is a normaliser
 * group of its own (mask counts, per-map weights) and its results are the bits of the call run alone.  Any other dense call (the joint mode
 * for S > 1 under TCSFM_WINDOW_PAIR, LM, free_source_depths) flushes what is waiting and runs at once.  Pose calls and dense calls are never
 * merged with each other. */
int tcsfm_refine_dense_window_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                     const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out,
                                     float *depth_out);

/* The reference's sequential driver loop as ONE call (run_sequential_optimization.py:186-247: for every window DataLoader batch ->
 * H2D in process_sample_batch, data/kitti_loader.py:60-98 -> optimize_window, strictly one window after the other).
 * Window w = the S + 1 consecutive frames w .. w+S, w = 0 .. T-S-1: its target is frame w + target_pos (target_pos = -1: the middle
 * one, (S+1)/2, as the reference's loaders choose it -- data/kitti_loader.py:271-273 -- i.e. the LATER frame of a two-frame window;
 * 0: the first), its sources are the other frames in order -> its 2*S directed pairs in the stacked order of train_mono.py:54-62
 * (forward pairs, then inverse pairs).  All array arguments are HOST pointers here (pinned memory makes the
 * copies asynchronous; pageable memory works, slower), whatever opts.host_ptrs says:
 *   frames [T,3,H,W], depths [T,1,H,W] (or disparities, opts.depth_is_disp), K [3,3] (one camera for the sequence),
 *   pose_init / pose_out [T-S, 2*S, 6], log_scale_out [T-S, 2*S] or NULL (TCSFM_REFINE_POSE_SCALE; the scale starts at 0).
 * Every frame crosses PCIe once, on a high-priority copy stream of the handle, four frames per copy, into a device ring of `ring`
 * frames (0 = default; at least windows_per_call + S + 4, or S + 2 with one window per call and single-frame copies); the calls are
 * issued round robin on the handle's lanes (tcsfm_set_lanes; 2-3 lanes: HIP maps a process's streams onto four hardware queues
 * unless GPU_MAX_HW_QUEUES is raised before the first HIP call, and the call's copy and pack streams take queues too; create the
 * handle AFTER the process's first device work -- see tcsfm_set_lanes) from the ring by pointer; a slot is recycled -- on the device, by events -- once every call reading it has
 * finished.  windows_per_call (0 = default 8, capped by max_pairs / (2 S)): the targets and every source of consecutive windows
 * are runs of the ring, so one call refines that many windows at once (the kernels fill the chip).  The call returns when all
 * windows are done (it synchronises).  Under o->window_rule = TCSFM_WINDOW_PAIR (the default) results are bit-identical to one
 * tcsfm_refine_window call per window, whatever the lanes, the ring and windows_per_call.  Under TCSFM_WINDOW_REFERENCE the
 * reference's batch-summed normalisers (optimizer.py:69,79) are taken over the windows of ONE CALL: windows_per_call plays the
 * role of the reference's config['minibatch'] (run_sequential_optimization.py:186 hands optimize_window a DataLoader batch of that
 * many windows), results depend on it exactly as the reference's loss depends on the minibatch, and are bit-identical to
 * tcsfm_refine_window calls over the same groups of windows; windows_per_call = 1 gives the per-window loss.
 * depths == NULL: every frame's depth comes from the depth network attached with tcsfm_sequence_depthnet (below); with nothing
 * attached a NULL depths is refused like any other NULL input.
 * pose_out may sit on pose_init; no other output may overlap another array of the call ("overlapping arguments"). */
int tcsfm_refine_sequence(tcsfm_handle h, const tcsfm_opts *o, int T, int S, const float *frames, const float *depths, const float *K,
                          const float *pose_init, float *pose_out, float *log_scale_out, int ring, int windows_per_call, int target_pos);
/* The same loop with the reference's pose initialisation inside it: for every window the coupled PoseNet loop of
 * train_mono.py:64-80 (tcsfm_solve_pose_iteratively, `num_iter` network evaluations: config['iterations'], 4 in the reference's
 * scripts) produces the initial poses on the window's lane, then the window is refined -- what optimize_window does per window
 * (optimizer.py:136-297).  The depth network's per-frame output is the `depths` argument (depths, not disparities) -- or, with
 * depths == NULL and a network attached (tcsfm_sequence_depthnet below), is computed inside the call: frames in, poses out, the
 * first pass of optimizer.py:142-160 included.
 * `pn`: a loaded PoseNet of this handle with max_images >= 2*S; the lanes run copies of it that share its weights.
 * pose_init_out [T-S, 2*S, 6] (or NULL) receives the PoseNet poses, pose_out the refined ones.  Bit-identical to one
 * tcsfm_solve_pose_iteratively + tcsfm_refine_window per CALL's windows (windows_per_call of them as one batch; the PoseNet's
 * work split -- hence its rounding -- depends on the number of images, see tcsfm_posenet_forward: per-window calls agree to 1e-5). */
int tcsfm_odometry_sequence(tcsfm_handle h, tcsfm_posenet *pn, int num_iter, const tcsfm_opts *o, int T, int S, const float *frames,
                            const float *depths, const float *K, float *pose_init_out, float *pose_out, float *log_scale_out, int ring,
                            int windows_per_call, int target_pos);
/* The dense mode (tcsfm_refine_dense_window: pose + per-pixel inverse depth with the Schur complement, BASELINE config 5) over a
 * sequence, same streaming and batching: depth_out [T-S, 2*S, H, W] (host) receives every directed pair's refined depth map.
 * Bit-identical to one tcsfm_refine_dense_window call per window.  depths == NULL: as for tcsfm_refine_sequence. */
int tcsfm_refine_dense_sequence(tcsfm_handle h, const tcsfm_opts *o, int T, int S, const float *frames, const float *depths, const float *K,
                                const float *pose_init, float *pose_out, float *depth_out, int ring, int windows_per_call, int target_pos);
/* Attaches a depth network to the handle's sequence calls (dn = NULL detaches): while one is attached, the three calls above accept
 * depths == NULL and compute every frame's depth on the device, once per frame, as the frame's chunk lands in the ring:
 * disp_to_depth(net(frame), o->min_depth, o->max_depth)[1], as optimizer.py:146-158 does -- the bits of tcsfm_depthnet_forward with
 * flip = 0 followed by tcsfm_disp_to_depth (the network's last kernel writes the depth; no disparity plane exists), so a frames-only
 * call returns the bits of the same call on depths computed that way and passed in.  The depths never cross PCIe: a quarter fewer
 * bytes go up per frame.  The stage runs on the call's pack stream, on a copy of the network that shares `dn`'s weights (a later
 * tcsfm_depthnet_load / _load_device of `dn` is seen by it) and owns its activations -- allocated here, for dn's max_images images, and
 * freed with `dn`; chunks of more frames run in groups.
 *   dn must be a loaded depth network of this handle (TCSFM_E_ARG otherwise; tcsfm_last_error says so).
 *   A non-NULL depths is used as given, whatever is attached.  depths == NULL with opts.depth_is_disp is refused (the stage produces
 *   depths), and needs 0 < o->min_depth < o->max_depth.
 *   tcsfm_depthnet_destroy of the attached network detaches it. */
int tcsfm_sequence_depthnet(tcsfm_handle h, tcsfm_depthnet *dn);
/* 8-bit camera frames.  Cameras, decoders and image files deliver interleaved 8-bit RGB; the reference turns it into floats on the host
 * (utils/custom_transforms.py:62-76 ArrayToTensor: transpose to C x H x W, .float() / 255).  tcsfm_sequence_frame_format sets how the
 * three sequence calls above read their `frames` argument -- a sticky setting of the handle, like tcsfm_sequence_depthnet; a new handle
 * is TCSFM_FRAMES_F32_CHW.  While a U8 format is set, `frames` is read as `const uint8_t *` in that layout (the prototypes stay as they
 * are: cast the pointer); the overlap check takes it as T*3*H*W BYTES.  The bytes cross PCIe as they are (a quarter of the float
 * frames' bytes: 7 instead of 16 B/pixel with depths given, 3 instead of 12 B/pixel with a depth network attached) into a device byte
 * ring, and a kernel on the call's pack stream writes the float ring before anything else reads it -- the pack cache, the PoseNet loop,
 * the depth-network stage and the dense mode are unchanged.  Each byte b becomes float32(b / 255), correctly rounded (a true fp32
 * division, the value torch.from_numpy(im).float() / 255 computes): a U8 call returns the bits of the float call on u8 / 255.
 *   An unknown format: TCSFM_E_ARG, tcsfm_last_error says so, the setting is unchanged.  A NULL handle: TCSFM_E_ARG.
 * tcsfm_frames_from_u8 is the same kernel as an operator, for callers of the window entries, who hold device pointers: N >= 1 frames of
 * `format` (TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC; TCSFM_FRAMES_F32_CHW is refused) at DEVICE pointer src (N*3*H*W bytes, any
 * address) -> planar float32 [N,3,H,W] at DEVICE pointer dst (aligned for float), on the handle's stream (asynchronous).  o->host_ptrs must be 0: a host
 * caller has the sequence calls.  dst overlapping src is refused ("overlapping arguments"). */
#define TCSFM_FRAMES_F32_CHW 0   /* default: [T,3,H,W] float32 in [0,1]                                  */
#define TCSFM_FRAMES_U8_CHW  1   /* [T,3,H,W] uint8                                                       */
#define TCSFM_FRAMES_U8_HWC  2   /* [T,H,W,3] uint8, interleaved RGB as cameras deliver it                */
int tcsfm_sequence_frame_format(tcsfm_handle h, int format);
int tcsfm_frames_from_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, const void *src, void *dst);
/* Camera-size frames.  No camera delivers the H x W the solver and the networks work at; the reference shrinks every frame on the host
 * with Pillow, Image.resize((W, H), Image.ANTIALIAS) -- Lanczos, support 3 (data/scannet_test_loader.py:157-170 inside the run-time
 * loader, data/create_kitti_odometry_data.py:56-65, data/create_kitti_eigen_data.py:30-35) -- and scales the intrinsics.  Pillow's 8-bit
 * resize is integer arithmetic (22-bit fixed-point coefficients, int32 sums, a clip to a byte after each of its two passes), and
 * k_resize_u8 (csrc/resize_u8_kernel.h) returns ITS BYTES EXACTLY.
 * tcsfm_sequence_frame_source is a sticky setting of the handle, like tcsfm_sequence_frame_format; (0, 0) means none and is the default.
 * While it is set AND a U8 format is set, the three sequence calls read `frames` as [T,src_h,src_w,3] (TCSFM_FRAMES_U8_HWC) or
 * [T,3,src_h,src_w] (TCSFM_FRAMES_U8_CHW) bytes; the overlap check takes it as T*3*src_h*src_w bytes.  The bytes cross PCIe at source
 * size into the byte ring, and the chunk's first launch on the pack stream is k_resize_u8 in k_frames_u8's place: it writes the float
 * ring and its mirror slots with float32(b / 255) of Pillow's bytes, so the call returns the bits of the same call on frames resized by
 * Pillow on the host.  Everything behind it is unchanged.  K keeps its meaning: the intrinsics of the H x W images
 * (tcsfm_scale_intrinsics makes them from the camera's).
 *   Refusals (TCSFM_E_ARG, tcsfm_last_error says why, the setting is unchanged): a negative size; exactly one of the two zero; a source
 *   beyond the kernel's tile -- more than 8 times H or W along that axis, or a side above 32768.  Upscaling is allowed, as Pillow allows
 *   it.  A NULL handle: TCSFM_E_ARG.  A sequence call with a source set and TCSFM_FRAMES_F32_CHW: TCSFM_E_ARG.
 * tcsfm_resize_u8 is the same kernel as an operator, on the handle's stream (asynchronous): N >= 1 frames of `format`
 * (TCSFM_FRAMES_U8_HWC or TCSFM_FRAMES_U8_CHW) and size src_h x src_w at DEVICE pointer src (any address) -> H x W frames at DEVICE
 * pointer dst: dst_format == format gives Pillow's bytes in the source's layout, dst_format == TCSFM_FRAMES_F32_CHW the planar
 * float32 [N,3,H,W] of b / 255 (dst aligned for float).  o->host_ptrs must be 0.  The same size limits.  dst overlapping src in any way
 * is refused ("tcsfm_resize_u8: dst overlaps src"); nothing about it is honoured. */
int tcsfm_sequence_frame_source(tcsfm_handle h, int src_h, int src_w);
int tcsfm_resize_u8(tcsfm_handle h, const tcsfm_opts *o, int format, int N, int src_h, int src_w, const void *src, int dst_format, void *dst);
/* Metric scale.  The poses of the three sequence calls are in the depth network's unit; the reference's sequential driver turns a
 * window's translations into metres with the DNet ground-plane scale of the window's TARGET depth (optimizer.py:254-256;
 * run_sequential_optimization.py:224-227: 30 * scale_factor * t).  tcsfm_sequence_scale is a sticky setting of the handle, like
 * tcsfm_sequence_frame_format: real_cam_height > 0 switches the stage on, 0 (the default) off.  While it is on, every frame of a
 * sequence call gets scale = real_cam_height / (exact lower median of its ground pixels' camera heights) -- tcsfm_scale_recovery_frames
 * on the ring's own depth planes, on the call's pack stream, once per chunk of frames (two launches: k_ground, k_median_frames): behind
 * the depth-network stage when depths == NULL, behind the chunk's copy when depths are given.  The depths never leave the device for it.
 * The scale is PER FRAME: it does not depend on the lanes, on windows_per_call or on the ring.  It is the scale of the depths the windows
 * START from: the reference's scale_factor_init, and -- with frozen networks and TCSFM_REFINE_POSE, which leave the depths alone -- also
 * its scale_factor; a caller with TCSFM_REFINE_POSE_SCALE divides frame f's scale by exp(log_scale) of the pair whose depth it scaled.
 * Everything else of the call is unchanged: pose_out, pose_init_out, log_scale_out and depth_out are the bits of the call with the
 * stage off.  The prototypes of the sequence calls stay as they are: the results are fetched afterwards.
 *   tcsfm_sequence_scale   refuses a negative, NaN or infinite height (TCSFM_E_ARG, the setting is unchanged).  A NULL handle: TCSFM_E_ARG.
 *   A sequence call with the stage on is refused (TCSFM_E_ARG, tcsfm_last_error says why) with opts.depth_is_disp -- the stage needs
 *   depths -- and with H < 5 or W < 5.
 *   tcsfm_sequence_scales  results of the LAST sequence call that ran with the stage on: HOST arrays of T entries by frame index
 *                          (scale_out float [T]; median_out float [T] or NULL; count_out int32 [T] or NULL: ground pixels; a frame
 *                          without any has NaN scale and median).  The handle keeps them until the next sequence call; a call that
 *                          fails, or runs with the stage off, leaves none.  T must be that call's T: otherwise, or with nothing kept,
 *                          TCSFM_E_ARG.  Window w's factor is depth unit (30) * scale[w + tp], tp the target's position as above. */
int tcsfm_sequence_scale(tcsfm_handle h, float real_cam_height);
int tcsfm_sequence_scales(tcsfm_handle h, int T, void *scale_out /* float [T] */, void *median_out /* float [T] or NULL */,
        int *count_out /* [T] or NULL */);
/* Structure.  The reference's sequential driver also keeps every window's disparity (run_sequential_optimization.py:215-220, 257-267:
 * optimized_results['disp_opt'], the input of paper_plots_and_data/evaluate_depth_eigen.py) -- helpers.get_disp_for_eigen
 * (optimization_experiments/helpers.py:35-49): the network on the frame and on its mirror image, disp_to_depth's scaled_disp of both,
 * the second un-flipped, the two blended by batch_post_process_disparity (utils/learning_helpers.py:115-123).  tcsfm_sequence_disparity
 * is a sticky setting of the handle, like tcsfm_sequence_scale; TCSFM_SEQ_DISP_OFF is the default.  While a mode is on, each of the three
 * sequence calls, run with depths == NULL and a network attached (tcsfm_sequence_depthnet), keeps every frame's disparity in a device
 * store of the handle, indexed by the frame number (T*H*W floats or doubles, grown when a call needs more, freed with the handle):
 *   TCSFM_SEQ_DISP_PLAIN  the depth stage's head stores the scaled disparity next to the depth: one more store, no more launches.  The
 *                         bits of tcsfm_depthnet_forward with flip = 0 followed by tcsfm_disp_to_depth's scaled_disp.
 *   TCSFM_SEQ_DISP_POST   a second pass of the network over the mirrored frame and the blend kernel follow the first pass, per group
 *                         of the network's max_images frames, on the call's pack stream before the chunk is handed to the lanes.
 *                         float64, the bits of tcsfm_depthnet_disp_for_eigen on the frame alone: they do not depend on the lanes, on
 *                         windows_per_call, on the ring or on the chunking.
 * Everything else of the call is unchanged: pose_out, pose_init_out, log_scale_out, depth_out and tcsfm_sequence_scales' results are the
 * bits of the call with the stage off.  The prototypes of the sequence calls stay as they are: the planes are fetched afterwards.
 *   tcsfm_sequence_disparity    an unknown mode: TCSFM_E_ARG, the setting is unchanged.  A NULL handle: TCSFM_E_ARG.
 *   A sequence call with the stage on is refused (TCSFM_E_ARG, tcsfm_last_error says why) with depths != NULL -- the stage keeps the
 *   network's own output --, with no network attached, and with min_depth / max_depth out of order.
 *   tcsfm_sequence_disparities  planes first .. first + count - 1 of the LAST sequence call that ran with the stage on, copied to the
 *                               HOST array `out` [count,H,W] -- float32 (PLAIN) or float64 (POST); *mode_out (or NULL) says which --
 *                               synchronously.  T must be that call's T, 0 <= first, count >= 1, first + count <= T: otherwise, or
 *                               with nothing kept, TCSFM_E_ARG.  A call that fails, or runs with the stage off, leaves nothing.
 * The operators, for callers who hold device pointers (asynchronous, on the handle's stream; o->host_ptrs must be 0; the array
 * parameters are declared void like tcsfm_frames_from_u8's: float32 in, float64 out, aligned for their types):
 *   tcsfm_disp_post_process        the blend alone.  l_disp [N,H,W] float32: scaled disparity of the frames; r_disp_mirrored [N,H,W]
 *                                  float32: of the mirrored frames, STILL mirrored (the kernel reads it reversed); out [N,H,W] float64:
 *                                      r = r_disp_mirrored[n][y][W-1-x];  m = float32(0.5 * (l + r))
 *                                      out = ((r_mask[x] * l + l_mask[x] * r) + ((1.0 - l_mask[x]) - r_mask[x]) * m)
 *                                  in float64, every operation rounded on its own, r_mask[x] = l_mask[W-1-x]: NumPy's evaluation of
 *                                  the reference's line on float32 planes, bit for bit.
 *   tcsfm_depthnet_disp_for_eigen  get_disp_for_eigen of N >= 1 device-resident frames imgs [N,3,H,W] float32 -> out [N,H,W] float64,
 *                                  in groups of the instance's max_images (o->min_depth, o->max_depth: disp_to_depth's); the planes of
 *                                  one group are the instance's own scratch.  The sequence stage's code path.
 *   out overlapping an input is refused ("overlapping arguments").
 * tcsfm_flip_ramp (host, no GPU needed): l_mask_out [W] doubles, W >= 2 (TCSFM_E_ARG otherwise):
 *     lin[i] = i * (1.0 / (W - 1)), lin[W-1] = 1.0 -- np.linspace(0, 1, W) --;  l_mask[i] = 1.0 - min(max(20.0 * (lin[i] - 0.05), 0.0), 1.0) */
#define TCSFM_SEQ_DISP_OFF   0
#define TCSFM_SEQ_DISP_PLAIN 1   /* scaled_disp of every frame, float32: disp_to_depth(net(frame))[0]              */
#define TCSFM_SEQ_DISP_POST  2   /* get_disp_for_eigen of every frame, float64: straight + mirrored pass, blended */
int tcsfm_sequence_disparity(tcsfm_handle h, int mode);
int tcsfm_sequence_disparities(tcsfm_handle h, int T, int first, int count, void *out /* HOST [count,H,W], float32 (PLAIN) or float64 (POST) */,
                               int *mode_out /* or NULL */);
int tcsfm_disp_post_process(tcsfm_handle h, const tcsfm_opts *o, int N, const void *l_disp /* float32 [N,H,W] */,
                            const void *r_disp_mirrored /* float32 [N,H,W] */, void *out /* float64 [N,H,W] */);
int tcsfm_depthnet_disp_for_eigen(tcsfm_depthnet *dn, const tcsfm_opts *o, int N, const void *imgs /* float32 [N,3,H,W] */,
                                  void *out /* float64 [N,H,W] */);
int tcsfm_flip_ramp(int W, void *l_mask_out /* double [W] */);
/* Evaluation.  What the reference does with those planes is paper_plots_and_data/evaluate_depth_eigen.py:133-177: resize each plane to
 * the ground truth's size, depth_unit / disp, mask and crop, median scaling, clip, seven error metrics per frame.  One launch evaluates N
 * frames, one workgroup per frame; no resized plane is written and, for the sequence form, no plane leaves the device.  Per frame
 * TCSFM_NEVAL doubles: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio (1.0 with median scaling off), n_valid (masked pixels),
 * n_median (masked pixels with gt < max_depth: the median's subset).  n_valid == 0: the seven metrics are NaN; n_median == 0 with
 * scaling on: ratio and the metrics are NaN.  The arithmetic, float64 with every operation rounded on its own:
 *   resize   bilinear, half-pixel centres, edges clamped: per axis scale = 1.0 / (n_dst / n_src), f = float32((d + 0.5) * scale - 0.5),
 *            s = floor(f), f = float32(f - s), (s < 0: s = 0, f = 0), (s >= n_src - 1: s = n_src - 1, f = 0), weights float32(1 - f) and
 *            f promoted to double, second tap min(s + 1, n_src - 1); the horizontal pass first.  This restates OpenCV's INTER_LINEAR; bit
 *            equality with cv2.resize is not claimed, and the exact-2x shrink (where OpenCV averages areas) is not special-cased.  A
 *            float32 plane is promoted first (exact).  Disparities must be positive and finite.
 *   mask     TCSFM_EVAL_EIGEN: gt > min_depth && gt < max_depth (float32 compares) inside rows [int(0.40810811 gt_h), int(0.99189189 gt_h))
 *            and columns [int(0.03594771 gt_w), int(0.96405229 gt_w)) (tcsfm_depth_eval_crop: y0, y1, x0, x1; host, no GPU);
 *            TCSFM_EVAL_EIGEN_BENCHMARK: gt > 0, the whole plane.
 *   scaling  ratio = float64(median(gt)) / median(pred) over the subset, np.median's: the middle element or the mean of the two middle
 *            ones in the array's own type (float32 for gt); pred *= ratio.  Then np.clip(pred, 0, max_depth), pred < min_depth -> min_depth.
 *   metrics  compute_errors on float64(gt); log(gt) is a float64 log (the reference's is a float32 one).  Sums in a fixed order: the
 *            results are bit-reproducible and do not depend on lds_pairs.
 * lds_pairs: how many masked pixels (each one (gt, pred) pair) the workgroup's list in LDS may hold (< 0: the default, its maximum); a
 * frame with more scans its crop again in every pass, with the same results.
 *   tcsfm_depth_eval           disp [N,H,W] (H, W the handle's) float32 (disp_is_f64 = 0) or float64, gt, metrics_out: DEVICE pointers;
 *                              asynchronous on the handle's stream; o->host_ptrs must be 0.
 *   tcsfm_sequence_depth_eval  planes first .. first + count - 1 of the store left by the LAST sequence call that ran with
 *                              tcsfm_sequence_disparity on (PLAIN or POST) against HOST ground truth of ONE size (KITTI's sizes differ
 *                              between drives: the caller groups frames by size); gt is staged in groups, the call returns synchronously.
 *                              T, first, count: tcsfm_sequence_disparities' rules.
 * Refused with TCSFM_E_ARG (tcsfm_last_error says why, nothing is launched, the outputs keep their contents): a NULL pointer, N < 1,
 * gt_h or gt_w < 1, an unknown protocol, !(0 < min_depth < max_depth), a depth_unit that is not positive and finite, metrics_out
 * overlapping an input ("overlapping arguments"); for the sequence form nothing kept, another T, a range outside [0, T). */
#define TCSFM_EVAL_EIGEN 0
#define TCSFM_EVAL_EIGEN_BENCHMARK 1
#define TCSFM_NEVAL 10
typedef struct tcsfm_depth_eval_opts {
    int32_t protocol, median_scaling;
    float min_depth, max_depth;
    double depth_unit;
    int32_t lds_pairs; /* <0: default */
} tcsfm_depth_eval_opts;
void tcsfm_depth_eval_default_opts(tcsfm_depth_eval_opts *e); /* EIGEN, 1, 1e-3, 80, 30.0, -1 */
int tcsfm_depth_eval_crop(int protocol, int gt_h, int gt_w, int *crop_out /* 4 ints: y0, y1, x0, x1 */);
int tcsfm_depth_eval(tcsfm_handle h, const tcsfm_opts *o, const tcsfm_depth_eval_opts *e, int N, int disp_is_f64,
                     const void *disp /* DEVICE [N,H,W] */, int gt_h, int gt_w, const void *gt /* DEVICE float32 [N,gt_h,gt_w] */,
                     void *metrics_out /* DEVICE double [N][TCSFM_NEVAL] */);
int tcsfm_sequence_depth_eval(tcsfm_handle h, const tcsfm_depth_eval_opts *e, int T, int first, int count, int gt_h, int gt_w,
                              const void *gt /* HOST float32 [count,gt_h,gt_w] */, void *metrics_out /* HOST double [count][TCSFM_NEVAL] */);
int tcsfm_lane_wait(tcsfm_handle h, int lane);
int tcsfm_lane_synchronize(tcsfm_handle h, int lane);
int tcsfm_lane_event(tcsfm_handle h, int lane, void **event_out);
int tcsfm_stream_wait_event(tcsfm_handle h, void *hip_stream, void *event);

/* ---- graph replay of repeated calls -------------------------------------------------------------------
 * A B = 1 refinement is nine short launches; with several calls in flight the HOST's launch rate (about 42 us per call), not the
 * kernels (about 40 us per call), sets the throughput, and on a slow host it alone does.  tcsfm_set_graph_replay(h, n > 0) lets the
 * handle and its lanes keep up to n captured calls each: a tcsfm_refine / tcsfm_refine_window / tcsfm_refine_dense / tcsfm_refine_dense_window
 * (also through the _async forms) with DEVICE pointers whose arguments -- options, sizes and every pointer -- equal those of an earlier
 * call is captured as one HIP graph the second time it is seen and replayed with a single hipGraphLaunch from the third time on
 * (least recently used entry evicted).  Same kernels, same order, same arguments: results are bit-identical to plain launches.
 * Calls with host pointers, under tcsfm_debug_trace / tcsfm_profile_begin, or on HIP's NULL stream are launched plainly.
 * The buffers named by the pointers must stay valid while the handle may replay the call (n = 0 drops all captures).  Default: off.
 *   tcsfm_graph_replay_counts   captures made / replays launched so far (handle + lanes), for tests and measurement.            */
int tcsfm_set_graph_replay(tcsfm_handle h, int max_graphs);
int tcsfm_graph_replay_counts(tcsfm_handle h, int *captures, int *replays);


/* ---- measurement hooks (bench.py) -------------------------------------------------------------- */

/* While profiling is on, every launch of the three kernel classes is bracketed by a pair of HIP events recorded on the
 * handle's stream.  tcsfm_profile_end() synchronises the stream and returns summed elapsed milliseconds and launch
 * counts per class: index 0 = k_linearize (the hot kernel), 1 = k_solve, 2 = k_pack. */
int tcsfm_profile_begin(tcsfm_handle h);
int tcsfm_profile_end(tcsfm_handle h, double ms_sum[3], int64_t launches[3]);
/* The same session's linearisation launches (k_linearize / k_dense_linearize) as the GPU itself timed them: every workgroup
 * stamps s_memrealtime (100 MHz) at its start and end, duration of a launch = latest end - earliest start.  An event pair
 * around a ~10 us kernel reads 2-4 us high (dispatch latency + the event packets); this figure is the one that agrees with
 * rocprofv3's kernel duration.  Call after tcsfm_profile_end; launches beyond the stamp buffer (4 M workgroups per session)
 * are not counted. */
int tcsfm_profile_kernel_time(tcsfm_handle h, double *ms_sum, int64_t *launches);
/* ... and the time during which AT LEAST ONE of those launches was running (the union of their [start, end] intervals over the handle and
 * its lanes, same counter): with launches of several streams sharing the chip, bytes / this = the chip's rate on the kernel. */
int tcsfm_profile_kernel_busy(tcsfm_handle h, double *ms_busy, int64_t *launches);
/* Parity-test hook.  The reference's masks are discontinuous (valid x [diff < auto_err], min over sources; helpers.py:17-19,
 * optimizer.py:47-69) and LM accepts / rejects on a cost comparison: near a tie the fp32 engine and a float64 checker may
 * decide differently.  While a trace is set, every linearisation `lin` of tcsfm_refine* / tcsfm_refine_dense* over N pairs
 * records the engine's decisions into caller-owned DEVICE buffers:
 *   bits   [lin][N][H*W] uint16  bit 0 = the pixel counts (final mask, incl. the min-over-sources selection), bit 1 = warp valid,
 *                                bits 2 / 3 = parity of the bilinear cell floor(ix) / floor(iy) (grid_sample's backward is
 *                                discontinuous across texel boundaries), bits 4-5 = sign of computed - projected depth,
 *                                bits 6-7 / 8-9 / 10-11 = sign of rec_c - tgt_c per colour channel (the signs in the derivatives
 *                                of |cd - pd| and |rec - tgt|; 2-bit codes: 0 exactly zero, 1 positive, 2 negative)
 *   decide [lin][N]      int32   LM: 1 = trial accepted (lin < n_iters) / last step kept (lin == n_iters); GN: 1
 * so that a checker can replay them and compare the continuous arithmetic at full tolerance (tests/test_gpu_parity.py).
 * tcsfm_linearize and tcsfm_linearize_window record too: their ONE linearisation writes bits [0][N][H*W] (N = 2 S B for a window,
 * stacked order) and leaves `decide` untouched (nothing is decided); the normal equations they return are those of exactly these
 * decisions (tests/test_gpu_linearize_exact.py).  tcsfm_loss_surface records nothing.
 * Capacities in elements; a call that would overflow them returns TCSFM_E_ARG.  Either pointer may be NULL; (NULL, 0, NULL, 0)
 * switches the trace off.  Costs one wave-uniform branch per pixel when off. */
int tcsfm_debug_trace(tcsfm_handle h, uint16_t *bits, int64_t bits_capacity, int32_t *decide, int64_t decide_capacity);
/* Diagnostic builds: 100 MHz wall-clock stamps of the phases of the last k_solve launch of pair 0 (zeros unless the
 * handle was created with TCSFM_DEBUG_STAMPS set in the environment). */
int tcsfm_debug_stamps(tcsfm_handle h, long long out[8]);
/* Test hook: ONE launch of a production pose solve kernel on records and optimiser state the caller gives (tests/test_gpu_solve_exact.py
 * compares it with exact arithmetic).  Every array is HOST memory; the entry copies them into device allocations of its own (not the
 * handle's scratch), launches on the handle's stream, synchronises once and copies every output array back WHOLE -- the caller fills them
 * with a sentinel beforehand and sees what the kernel left alone.  variant: 0 k_solve, 1 k_solve_lean, 2 / 3 the pair role of
 * k_solve_front without / with the pose-consistency code.  np (6 / 7), has_dc, the solver, the chart, the damping schedule, prior_scale
 * and b_dc = w_dc / (H W) come from `opts` and the handle as in a refine call; mode: 0 iteration step, 1 final LM cost check, 2 export of
 * the normal equations.  `state` and `pconst` hold the library's PairState / PairConst structs (sizes: tcsfm_debug_solve_layout).
 * Anything that would index outside the given arrays or reach a branch the variant has compiled out is refused with TCSFM_E_ARG before
 * anything is launched (tcsfm_last_error says what).  With TCSFM_DEBUG_GUARDS=1 the guard bands of the entry's own allocations are read back
 * before they are freed: a launch that wrote outside them makes the call return TCSFM_E_HIP (tcsfm_debug_check_guards sees live
 * allocations only). */
typedef struct tcsfm_debug_solve_args {
    int32_t variant, N, ngrp, mode, it;
    int32_t n_alloc;              /* pairs every per-pair array below holds (>= N): pairs N .. n_alloc - 1 are never touched */
    int32_t rule, grp_fwd, n_pairs;
    int32_t norm_n, norm_Bt, norm_B;                      /* norms [norm_n][2] */
    int32_t pc_np, pc_self0, pc_part0, pose_lin_pairs;    /* pose_lin [2][pose_lin_pairs][12] */
    int32_t c_ncall, c_B, c_S, c_n0;
    int32_t c_len[16];            /* pairs the per-call arrays hold */
    double scale_fwd, scale_inv, w_pc, pc_eps;
    const float *records;         /* [n_alloc][ngrp][nacc] */
    const int32_t *norms;         /* or NULL: the counts are summed from the records */
    void *state;                  /* [n_alloc] PairState, in and out */
    void *pconst;                 /* [n_alloc] PairConst, in and out */
    double *lin_out;              /* [n_alloc][np np + np + 4] or NULL */
    double *delta_out;            /* [n_alloc][8] or NULL */
    int32_t *accept_out, *trace_decide;   /* [n_alloc] or NULL */
    float *pose_out;              /* [n_alloc][6] or NULL (NULL: no launch emits a pose) */
    float *log_scale_out;         /* [n_alloc] or NULL */
    float *c_pose_out[16];        /* c_ncall > 0: [c_len[i]][6] per call */
    float *c_ls_out[16];          /*              [c_len[i]] per call, or NULL */
    float *stats;                 /* [n_alloc][n_iters + 1][TCSFM_NSTAT] or NULL */
    double *pose_lin;             /* in and out, or NULL */
} tcsfm_debug_solve_args;
int tcsfm_debug_solve(tcsfm_handle h, const tcsfm_opts *opts, tcsfm_debug_solve_args *args);
/* sizeof(PairState), sizeof(PairConst) as the library was compiled (host, no GPU needed) */
int tcsfm_debug_solve_layout(int *sizeof_pair_state, int *sizeof_pair_const);
/* Test hook: ONE launch of a production JOINT solve kernel (the 6 NS x 6 NS reduced camera system of a target's NS forward pairs) on records
 * and optimiser state the caller gives (tests/test_gpu_joint_solve_exact.py compares it with exact arithmetic).  As tcsfm_debug_solve: every
 * array is HOST memory, copied into guarded device allocations of the entry's own, one launch on the handle's stream, one synchronisation,
 * every in/out and out array copied back WHOLE, the entry's guard bands read back before they are freed.  variant: 0 k_solve_joint<NS>;
 * 1 / 2 the joint role of k_solve_front<NS> without / with the pose-consistency code (no workgroup takes the pair role); 3 / 4
 * k_solve_joint2<NS> without / with it: group `a` has NS sources per target, group `b` ONE (the free-source mode's inverse groups).
 * Variants 0 to 2 use group `a` only.  The solver, the damping schedule (lambda0, lambda_up, lambda_down, lambda_min) and n_iters come from
 * `opts`; mode: 0 iteration step, 1 final LM cost check; a group whose export_out is given takes the export path (cost, factor, gradient:
 * nothing else written).  Forward pair (s, b) of a group is pair n0 + s B + b of the shared per-pair arrays.  Anything that would index
 * outside a given array or reach a compiled-out branch is refused with TCSFM_E_ARG before anything is launched. */
typedef struct tcsfm_debug_joint_group {
    int32_t B, b_alloc;           /* targets solved; targets every per-target array below holds (>= B): B .. b_alloc - 1 are never touched */
    int32_t nblk, nsplit;         /* records per target; workgroups that share a target's record sum (1 .. 8) */
    int32_t n0;                   /* index of the group's first pair in the shared per-pair arrays */
    int32_t norm_n, norm_B;       /* norms [norm_n][2]; targets per normaliser group (0: one group) */
    int32_t pc_self0, pc_part0;   /* pose_lin slots of the group's pair 0 and of its partner */
    int32_t pad;
    double c_f;
    const float *records;         /* [b_alloc][nblk][NACC] */
    const int32_t *norms;         /* or NULL: 1 / K from the records */
    void *js;                     /* [b_alloc] JointState, in and out */
    double *delta_out;            /* [b_alloc][24] or NULL */
    int32_t *accept_out;          /* [b_alloc] or NULL */
    double *export_out;           /* [b_alloc][26] or NULL; given: the export path */
    double *jpart;                /* [b_alloc][nsplit][NACC], out; required when nsplit > 1 */
    int32_t *jtick;               /* [b_alloc], in and out; required and all zero when nsplit > 1 */
} tcsfm_debug_joint_group;
typedef struct tcsfm_debug_solve_joint_args {
    int32_t variant, NS, it, mode;
    int32_t n_alloc;              /* pairs every shared per-pair array holds */
    int32_t pc_np;                /* pose_lin [2][pc_np][12] */
    int32_t c_ncall, c_B, c_S, pad;
    int32_t c_len[16];            /* pairs the per-call arrays hold */
    double w_pc, pc_eps;
    tcsfm_debug_joint_group a, b;
    void *state;                  /* [n_alloc] PairState, in and out */
    void *pconst;                 /* [n_alloc] PairConst, in and out */
    float *stats;                 /* [n_alloc][n_iters + 1][TCSFM_NSTAT] or NULL */
    float *pose_out;              /* [n_alloc][6] or NULL (NULL: no launch emits a pose) */
    int32_t *trace_decide;        /* [n_alloc] or NULL */
    double *pose_lin;             /* in and out; required by variants 2 and 4 */
    float *c_pose_out[16];        /* c_ncall > 0 (variants 0 to 2): [c_len[i]][6] per call */
} tcsfm_debug_solve_joint_args;
int tcsfm_debug_solve_joint(tcsfm_handle h, const tcsfm_opts *opts, tcsfm_debug_solve_joint_args *args);
/* ... and sizeof(JointState) (host, no GPU needed); any pointer may be NULL */
int tcsfm_debug_solve_joint_layout(int *sizeof_pair_state, int *sizeof_pair_const, int *sizeof_joint_state);

/* ---- SE(3) utilities, host, double (replace liegroups.SE3 at data/kitti_loader_stereo.py:129-147,
 *      validate.py:65-71; liegroups is an absent third-party dependency, version unpinned) ---------- */
void tcsfm_pose_to_matrix(const double pose[6], double T[12]);   /* pose_vec2mat(-pose), 3x4 row-major  */
void tcsfm_matrix_to_pose(const double T[12], double pose[6]);
void tcsfm_se3_exp(const double xi[6], double T[12]);            /* xi = [rho, phi]                     */
void tcsfm_se3_log(const double T[12], double xi[6]);
void tcsfm_se3_mul(const double A[12], const double B[12], double C[12]);
void tcsfm_se3_inv(const double A[12], double B[12]);


/* ---- camera-size frames, host (no GPU needed): the resize's coefficient table and the loaders' intrinsics scaling ------------------
 * tcsfm_resize_coeffs: Pillow's 8-bit Lanczos table of one axis, input length `in` -> output length `out` (both >= 1), in double:
 *     scale = in / out;  fs = max(scale, 1);  support = 3 fs;  *ksize_out = (int)ceil(support) * 2 + 1
 *     output xx:  center = (xx + 0.5) scale;  xmin = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - xmin
 *                 w[x] = lanczos((x + xmin - center + 0.5) / fs), divided by their sum, times 1 << 22, rounded half away from zero
 *   bounds[out][2] = {xmin, n}, kk[out][ksize] (zero beyond n).  With bounds or kk NULL only *ksize_out is written: call twice.
 * tcsfm_scale_intrinsics: K_src, K_out are 9 floats each (row-major 3x3; declared void like tcsfm_frames_from_u8's arrays).  Row 0 is
 *   (float)((double)K * ((double)W / src_w)), row 1 (float)((double)K * ((double)H / src_h)) -- the loaders' K[0] *= zoom_x;
 *   K[1] *= zoom_y -- and row 2 is copied.  K_out may be K_src.
 * Both return TCSFM_OK, or TCSFM_E_ARG for a NULL pointer or a size below 1. */
int tcsfm_resize_coeffs(int in, int out, int *ksize_out, int *bounds, int *kk);
int tcsfm_scale_intrinsics(int src_h, int src_w, int H, int W, const void *K_src, void *K_out);

#ifdef __cplusplus
}
#endif
#endif /* TCSFM_H */
