#!/usr/bin/env python3
"""A miniature of the reference's optimization_experiments/run_sequential_optimization.py on synthetic data: per-window
refinement with the drop-in DepthOptimizer, trajectory composition (validate.compute_trajectory) and odometry errors.

    python examples/run_sequence.py [--frames 40] [--sources 2]          (needs an MI355X)
    python examples/run_sequence.py --frames-only CHECKPOINT              frames in, poses out: see frames_only() below
    python examples/run_sequence.py --frames-only CHECKPOINT --u8-frames  ... from the camera's bytes: interleaved 8-bit RGB [T,H,W,3]
    python examples/run_sequence.py --frames-only CHECKPOINT --camera-size 376x1241   ... from camera-size bytes [T,376,1241,3]: resized on the device

The two "networks" are stand-ins with the reference models' call conventions: the depth net returns the scene's true
disparity for whatever frame it is shown, the pose net returns a noisy version of the true relative pose (PoseNet-quality
initialisation).  Everything between the network calls -- warps, residuals, Gauss-Newton -- runs in libtcsfm_hip.so.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import os as _os; _os.environ.setdefault("TCSFM_SET_ENV_DEFAULTS", "1")      # (a measurement script owns its process: HIP_FORCE_DEV_KERNARG / GPU_MAX_HW_QUEUES when absent)
from tightly_coupled_sfm_amd import synth                                    # noqa: E402
from tightly_coupled_sfm_amd.optimizer import DepthOptimizer                  # noqa: E402
from tightly_coupled_sfm_amd.validate import compute_trajectory               # noqa: E402

H, W = 192, 640


class DepthNet(torch.nn.Module):
    """returns the stored sigmoid disparity of whichever known frame (or its mirror image) each input is"""
    def __init__(self, frames, disps):
        super().__init__(); self.frames, self.disps = frames, disps
    def _one(self, x):
        err = (self.frames - x).abs().flatten(1).amax(1); errf = (torch.flip(self.frames, [3]) - x).abs().flatten(1).amax(1)
        return self.disps[int(err.argmin())] if float(err.min()) <= float(errf.min()) else torch.flip(self.disps[int(errf.argmin())], [2])
    def forward(self, x=None, skips=None, return_disp=True, epoch=0):
        if x is not None and not return_disp:
            return None, [x, x]
        src = x if x is not None else skips[-1]
        return [torch.stack([self._one(src[i:i + 1]) for i in range(src.shape[0])])], [src, src]


class PoseNet(torch.nn.Module):
    def __init__(self):
        super().__init__(); self.next = None
    def forward(self, x):
        out, self.next = self.next, None
        return out if out is not None else torch.zeros(x.shape[0], 6, device=x.device)


def frames_only(args):
    """--frames-only: the library's own depth network and PoseNet from a reference checkpoint (a file with 'depth_state_dict' and
    'pose_state_dict', or a run directory), attached to the engine, and ONE call per sequence that takes the frames alone --
    PoseNetHIP.odometry_sequence(frames, None, K): depth network, coupled PoseNet loop and refinement all run inside it."""
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP, read_pose_state_dict
    S = args.sources
    eng = Engine(H, W, 2 * S * 8, lanes=2)
    depth_net = DepthNetHIP(eng, 8).load_checkpoint(args.frames_only)
    pose_net = PoseNetHIP(eng, 2 * S * 8, read_pose_state_dict(args.frames_only))
    eng.attach_depthnet(depth_net)
    pose = np.array([0.002, -0.001, 0.033, 0.001, -0.003, 0.001])
    first = synth.make_pair(H, W, seed=500, pose_gt=pose)
    frames = torch.as_tensor(np.stack([first["tgt"]] + [synth.make_pair(H, W, seed=500 + i, pose_gt=pose)["src"] for i in range(args.frames - 1)])
                             .astype(np.float32)).pin_memory()
    if args.u8_frames:      # what a camera or a decoder delivers: interleaved 8-bit RGB.  The bytes go up as they are (a quarter of the
        # float frames' PCIe traffic and pinned memory) and the library makes u8 / 255 on the device -- ArrayToTensor's values, bit for bit
        frames = torch.from_numpy(np.ascontiguousarray(np.round(frames.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).pin_memory()
        print(f"frames: uint8 {list(frames.shape)} (HWC), {frames.numel() / 1e6:.1f} MB pinned")
    source_size, K = None, first["K"]
    if args.camera_size:    # what the camera really delivers: frames of ITS size (KITTI: 1241 x 376).  The reference's loaders shrink every frame
        # with Pillow's Lanczos filter on the host and scale K (data/scannet_test_loader.py:157-170); here the camera's bytes go up as they
        # are, the library makes the H x W frames on the device -- Pillow's bytes exactly -- and Engine.scale_intrinsics makes K
        h, w = (int(v) for v in args.camera_size.lower().split("x"))
        big = torch.nn.functional.interpolate(frames.float() if frames.dtype != torch.uint8 else frames.permute(0, 3, 1, 2).float() / 255,
                                              size=(h, w), mode="bilinear", align_corners=False)       # a stand-in camera: the scene enlarged
        frames = (big * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
        source_size = (h, w)
        K_camera = np.asarray(first["K"], dtype=np.float64) * np.array([[w / W], [h / H], [1.0]])       # the camera's own intrinsics
        K = eng.scale_intrinsics(K_camera, source_size)
        print(f"frames: uint8 {list(frames.shape)} at the camera's size, {frames.numel() / 1e6:.1f} MB pinned; K scaled to {W}x{H}:\n{K}")
    opts = default_opts(n_iters=args.gn_iters, min_depth=0.06, max_depth=2.67)
    t0 = time.perf_counter()
    init, refined = pose_net.odometry_sequence(frames, None, K, opts, sources=S, iterations=4, target_pos=-1,
                                               **({} if source_size is None else {"source_size": source_size}),
                                               **({} if args.cam_height is None else {"cam_height": args.cam_height / DEPTH_UNIT}),
                                               **({"disparity": "post"} if args.save_disps or args.gt_depths else {}))
    dt = time.perf_counter() - t0
    print(f"{args.frames} frames -> {refined.shape[0]} windows of {2 * S} directed pairs in {dt * 1e3:.1f} ms (first call: allocations included)")
    with np.printoptions(precision=4, suppress=True):
        print("PoseNet poses of window 0:\n", init[0].numpy())
        print("refined poses of window 0:\n", refined[0].numpy())
        if args.cam_height is not None:     # metres: the DNet ground-plane scale of every window's target frame, computed inside the call from
            # the ring's own depth planes (run_sequential_optimization.py:224-227: 30 * scale_factor * t)
            from tightly_coupled_sfm_amd.streaming import metric_poses
            sc = eng.sequence_scales()
            metric = metric_poses(refined, sc["scale"], S, target_pos=-1, depth_unit=DEPTH_UNIT)
            print(f"per-frame scales (ground pixels {sc['count'].tolist()[:6]} ...):\n", sc["scale"].numpy()[:6], "...")
            print("refined poses of window 0, translations in metres:\n", metric[0].numpy())
    if args.save_disps:     # the structure: every frame's flip-post-processed disparity (helpers.get_disp_for_eigen), kept on the device inside
        # the call and fetched once -- float64 [T,H,W], np.concatenate of the driver's pred_disps: what evaluate_depth_eigen.py loads
        disps = eng.sequence_disparities()
        np.save(args.save_disps, disps)
        print(f"disparities: float64 {list(disps.shape)}, {disps.min():.4f} .. {disps.max():.4f} -> {args.save_disps}")
    if args.gt_depths:      # the paper's depth table: evaluate_depth_eigen.py's loop on the device, over the planes the call kept -- no plane
        # is fetched; the ground truth (one float32 plane per frame, sizes may differ) goes up in groups of one size
        from tightly_coupled_sfm_amd import evaluate_depth_eigen as ev
        gt_depths = ev.load_gt_depths(args.gt_depths)
        n = min(len(gt_depths), args.frames)
        print(ev.format_table(ev.evaluate(None, list(gt_depths[:n]), eng, benchmark="eigen", median_scaling=True)))


DEPTH_UNIT = 30.0       # the reference's depth unit in metres (run_sequential_optimization.py:224)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-only", metavar="CHECKPOINT", default=None,
                    help="load the depth network and the PoseNet from this reference checkpoint and run the sequence from the frames alone "
                         "(Engine.attach_depthnet + PoseNetHIP.odometry_sequence with depths=None)")
    ap.add_argument("--u8-frames", action="store_true",
                    help="with --frames-only: quantise the synthetic frames to interleaved 8-bit RGB [T,H,W,3] and feed the bytes "
                         "(the library converts them on the device: tcsfm_sequence_frame_format)")
    ap.add_argument("--camera-size", metavar="HxW", default="",
                    help="with --frames-only: feed interleaved 8-bit frames of this size (e.g. 376x1241, a KITTI camera) and let the library "
                         "resize them on the device with Pillow's Lanczos bytes (source_size=: tcsfm_sequence_frame_source)")
    ap.add_argument("--cam-height", type=float, default=None, metavar="METRES",
                    help="with --frames-only: the camera's height above the ground (KITTI: 1.65); every frame's DNet scale is computed inside "
                         "the call (cam_height=: tcsfm_sequence_scale) and the translations are printed in metres (streaming.metric_poses)")
    ap.add_argument("--save-disps", metavar="FILE", default="",
                    help="with --frames-only: keep every frame's flip-post-processed disparity inside the call (disparity=\"post\": "
                         "tcsfm_sequence_disparity) and write them as the .npy file paper_plots_and_data/evaluate_depth_eigen.py loads")
    ap.add_argument("--gt-depths", metavar="FILE.npz", default="",
                    help="with --frames-only: the reference's gt_depths.npz (loaded as paper_plots_and_data/evaluate_depth_eigen.py loads it); "
                         "the disparities kept inside the call are evaluated against it on the device (tcsfm_sequence_depth_eval) and the "
                         "script's table is printed")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--sources", type=int, default=1, choices=(1, 2))
    ap.add_argument("--gn-iters", type=int, default=8)
    ap.add_argument("--window-rule", default="reference", choices=("reference", "pair"),
                    help="S = 2: minimise the reference's own compute_optimization_loss (default, as the mirror does) or every directed pair's "
                         "own cost (converges in about half the iterations: DESIGN.md section 2)")
    args = ap.parse_args()
    if args.frames_only:
        return frames_only(args)
    if args.cam_height is not None:
        ap.error("--cam-height goes with --frames-only (the per-window loop below gets its scale from DepthOptimizer)")
    if args.save_disps:
        ap.error("--save-disps goes with --frames-only (the per-window loop below has helpers.get_disp_for_eigen)")
    if args.gt_depths:
        ap.error("--gt-depths goes with --frames-only (it evaluates the disparities a frames-only call keeps)")
    if args.camera_size:
        ap.error("--camera-size goes with --frames-only (for frames held on the device: Engine.resize_u8)")
    if args.u8_frames:
        ap.error("--u8-frames goes with --frames-only (the per-window loop below holds its frames on the device: Engine.frames_from_u8 is for that)")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    rng = np.random.default_rng(0)
    options = {"diff_img_argmin": True, "automasking": True, "mode": "scaled", "l_depth_consist": True, "l_depth_consist_weight": 0.15,
               "l_inverse_reconstruction": True, "num_source_imgs": args.sources, "gn_iters": args.gn_iters, "window_rule": args.window_rule}
    config = {"minibatch": 1, "device": "cuda", "min_depth": 0.06, "max_depth": 2.67, "iterations": 1, "camera_height": 1.65, "flow_type": "none"}
    gt, init, opt, conv, t_total = [], [], [], [], 0.0
    for i in range(args.frames):
        pose = np.array([0.002, -0.001, 0.033, 0.001, -0.003, 0.001]) + rng.normal(scale=[3e-4, 3e-4, 2e-3, 5e-4, 1e-3, 5e-4])
        pairs = [synth.make_pair(H, W, seed=500 + i, pose_gt=pose * (1 if s == 0 else -1)) for s in range(args.sources)]
        frames = t(np.stack([pairs[0]["tgt"]] + [p["src"] for p in pairs]))
        sig = lambda d: synth.depth_to_sigmoid_disp(d.astype(np.float64)).astype(np.float32)
        disps = t(np.stack([sig(pairs[0]["depth_t"])] + [sig(p["depth_s"]) for p in pairs])[:, None])
        fwd = np.stack([synth.perturb_pose(p["pose_gt"], 900 + i * 2 + s) for s, p in enumerate(pairs)])
        pose_net = PoseNet(); pose_net.next = t(np.concatenate([fwd, np.stack([synth.invert_pose(x) for x in fwd])]))
        optimiser = DepthOptimizer(options, config, pose_net, DepthNet(frames, disps), "synthetic")
        gts = [t(p["pose_gt"][None]) for p in pairs]
        data = (frames[0:1], [frames[1 + s:2 + s] for s in range(args.sources)], gts, gts, None, t(pairs[0]["K"][None]), None, None, None, None, None)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = optimiser.optimize_window(i, data)
        torch.cuda.synchronize(); t_total += time.perf_counter() - t0
        gt.append(pairs[0]["pose_gt"].astype(np.float64)); init.append(r["poses_init"][0].numpy().astype(np.float64)); opt.append(r["poses_opt"][0].numpy().astype(np.float64))
        # yardstick: the same window with the same options, started at the true poses and iterated to convergence
        truth = np.stack([p["pose_gt"] for p in pairs])
        pose_net.next = t(np.concatenate([truth, np.stack([synth.invert_pose(x) for x in truth])]))
        conv.append(DepthOptimizer(dict(options, gn_iters=40), config, pose_net, optimiser.depth_model, "synthetic")
                    .optimize_window(i, data)["poses_opt"][0].numpy().astype(np.float64))
    conv_traj = compute_trajectory(np.stack(conv), np.eye(4)[None])[0]
    gt_traj = compute_trajectory(np.stack(gt), np.eye(4)[None])[0]
    for name, poses in (("PoseNet stand-in", init), (f"refined ({args.gn_iters} GN its)", opt)):
        _, _, e_conv, _ = compute_trajectory(np.stack(poses), conv_traj)
        _, _, e_true, _ = compute_trajectory(np.stack(poses), gt_traj)
        print(f"{name:20s} vs converged photometric solution: trans {e_conv[0]:.4f}, rot {e_conv[1]:.4f} deg   |   vs scene truth: trans {e_true[0]:.4f}, rot {e_true[1]:.4f} deg")
    print(f"{args.frames} windows, S={args.sources}: {t_total / args.frames * 1e3:.2f} ms per optimize_window call "
          "(stand-in networks included; the refinement itself is ~0.1 ms)")
    print("note: what the optimiser minimises is the reference's residual; on rendered data its minimiser is offset from the scene truth "
          "(half-pixel sampling convention of the reference's warp, interpolation on the near ground plane), so the first column is "
          "the meaningful one -- in the reference's real pipeline the networks are trained through the same warp")


if __name__ == "__main__":
    main()
