"""Drop-in for train_mono.solve_pose_iteratively (train_mono.py:41-120): the coupled PoseNet / warp iteration and the
residual assembly of every directed pair, forward and inverse, of a window.
  * A pose network with the reference architecture's parameters (models/pose_models.py:88-147) is evaluated by the library's own
    gfx950 PoseNet (csrc/posenet_kernel.h): the whole loop -- network, warp, correction -- runs inside libtcsfm_hip.so
    (tcsfm_solve_pose_iteratively) without a single PyTorch kernel.  Its weights are read once per module (and again when a
    parameter's version counter changes).
  * Any other callable (a different architecture, the constant-pose stand-ins of the tests) is called as given; everything
    between its calls still runs in the library: the (target x valid | reconstruction) input of the next call is written by the
    warp kernel itself (:73-77).
  * the residual maps of all 2 S B directed pairs come from one fused launch (:82-100).
  * Under autograd -- grad enabled, a depth that requires grad, num_iter > 1 and a pose model the library evaluates -- the loop runs
    as the composition of two autograd Functions per iteration, Engine.posenet_input_autograd (the warp, HIP backward
    tcsfm_warp_backward) and PoseNetHIP.__call__ (HIP backward tcsfm_posenet_backward, towards the network's input): the same
    kernels as the fused loop, so stacked_poses, the poses and every map of `outputs` have its bits, and they carry the gradient the
    reference's loss.backward() follows through the poses.  The first call does not depend on the depths and stays plain.  A plain
    nn.Module's PARAMETERS get no gradient (their .grad stays None, whatever their requires_grad says): the library evaluates a
    frozen copy, which is the reference's default tuning mode (optimize_depth_encoder).
  * The reference's optimize_pose_weights_all mode (optimizer.py:187-189) is opt-in through posenet_train.PoseNetModule: its
    parameters live in torch, and when grad is enabled and a depth or one of ITS parameters requires grad, every call of the loop --
    the first included, for any num_iter >= 1 -- runs through the module's autograd Function (HIP backward
    tcsfm_posenet_param_backward: image and parameter gradients from one walk).  Same kernels, same bits as the fused loop.
"""
from __future__ import annotations

import torch

from ._shared import get_engine
from .posenet import PoseNetHIP, is_reference_posenet
from .posenet_train import PoseNetModule

_NETS = {}     # id(module) -> (parameter version stamp, engine, PoseNetHIP)


def _library_posenet(pose_model, eng, n_images):
    if not isinstance(pose_model, torch.nn.Module) or not is_reference_posenet(pose_model):
        return None
    if any(p.device.type != "cuda" for p in pose_model.parameters()):
        return None
    stamp = tuple(int(p._version) for p in pose_model.parameters())
    hit = _NETS.get(id(pose_model))
    if hit is None or hit[1] is not eng or hit[2].max_images < n_images:
        hit = (stamp, eng, PoseNetHIP(eng, max(n_images, eng.max_pairs), pose_model))
    elif hit[0] != stamp:
        hit[2].load(pose_model)
        hit = (stamp, eng, hit[2])
    _NETS[id(pose_model)] = hit
    return hit[2]


def solve_pose_iteratively(num_iter, depths, pose_model, target_img, source_img_list, intrinsics, return_errors=False):
    S, B = len(source_img_list), target_img.shape[0]
    split = S * B
    H, W = target_img.shape[2:]
    eng = get_engine(H, W, 2 * split)
    target_depths = depths[0].float().repeat(S, 1, 1, 1)
    source_depths = torch.cat([d.float() for d in depths[1:]], 0)
    source_imgs = torch.cat([s.float() for s in source_img_list], 0)
    K = intrinsics.float().repeat(2 * S, 1, 1).contiguous()
    target_imgs = target_img.float().repeat(S, 1, 1, 1)
    imgs = torch.cat([torch.cat([target_imgs, source_imgs], 1), torch.cat([source_imgs, target_imgs], 1)], 0)   # :54-62
    d_t = torch.cat([target_depths, source_depths], 0).contiguous()
    d_s = torch.cat([source_depths, target_depths], 0).contiguous()
    tgt, src = imgs[:, 0:3].contiguous(), imgs[:, 3:6].contiguous()
    net = None if isinstance(pose_model, PoseNetModule) else _library_posenet(pose_model, eng, 2 * split)
    if isinstance(pose_model, PoseNetModule):
        # the parameters live in the module: the loop runs under autograd when a depth (num_iter > 1) or a parameter requires grad
        # -- the first call included, whose only differentiable inputs are the parameters -- and inside the library otherwise
        grad_on = torch.is_grad_enabled()
        if grad_on and (any(p.requires_grad for p in pose_model.parameters()) or (num_iter > 1 and any(d.requires_grad for d in depths))):
            full_poses = pose_model(imgs.contiguous())                                                             # :64
            stacked = [full_poses]
            for _ in range(num_iter - 1):                                                                          # :73-80
                new_imgs = eng.posenet_input_autograd(tgt, src, d_t, d_s, full_poses, K)
                full_poses = full_poses + pose_model(new_imgs)
                stacked.append(full_poses)
            stacked_poses = torch.stack(stacked, 1)
        else:
            with torch.no_grad():
                nat = pose_model._native_for(imgs, 2 * split)
            full_poses, stacked_poses = nat.net.solve_pose_iteratively(num_iter, target_img.float(), [s.float() for s in source_img_list],
                                                                       depths[0].float(), [d.float() for d in depths[1:]], intrinsics.float())
    elif net is not None and num_iter > 1 and torch.is_grad_enabled() and any(d.requires_grad for d in depths):
        with torch.no_grad():
            full_poses = net(imgs.contiguous())                                                                    # :64, no depth in it
        stacked = [full_poses]
        for _ in range(num_iter - 1):                                                                              # :73-80
            new_imgs = eng.posenet_input_autograd(tgt, src, d_t, d_s, full_poses, K)
            full_poses = full_poses + net(new_imgs)
            stacked.append(full_poses)
        stacked_poses = torch.stack(stacked, 1)
    elif net is not None:     # network, warps and corrections of all iterations inside the library (:64-80)
        full_poses, stacked_poses = net.solve_pose_iteratively(num_iter, target_img.float(), [s.float() for s in source_img_list],
                                                               depths[0].float(), [d.float() for d in depths[1:]], intrinsics.float())
    else:
        full_poses = pose_model(imgs)                                                                              # :64
        stacked = [full_poses.clone()]
        for _ in range(num_iter - 1):                                                                              # :73-80
            new_imgs = eng.posenet_input(tgt, src, d_t, d_s, full_poses[:, :6].float().contiguous(), K)
            full_poses = full_poses + pose_model(new_imgs)
            stacked.append(full_poses.clone())
        stacked_poses = torch.stack(stacked, 1)
    outputs = {"fwd": {}, "inv": {}}
    if return_errors:                                                                                              # :82-104
        r = eng.compute_photometric_error(tgt, src, d_t, d_s, full_poses[:, :6].float().contiguous(), K)
        for name, sl in (("fwd", slice(0, split)), ("inv", slice(split, None))):
            outputs[name] = {"diff_img": r["diff_img"][sl], "img_rec": r["img_rec"][sl], "valid_mask": r["warp_valid"][sl],
                             "weight_mask": r["weight_mask"][sl], "poses": stacked_poses[sl], "auto_mask_error": r["auto_mask_error"][sl],
                             "auto_mask": r["auto_mask"][sl]}
        outputs["comb"] = {"imgs": torch.cat([tgt * r["warp_valid"], r["img_rec"]], 1), "valid_mask": r["warp_valid"]}
    poses = [stacked_poses[B * i:B * (i + 1), -1] for i in range(S)]                                               # :108-115
    poses_inv = [stacked_poses[split + B * i:split + B * (i + 1), -1] for i in range(S)]
    return (poses, poses_inv, outputs) if return_errors else (poses, poses_inv)
