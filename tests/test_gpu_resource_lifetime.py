"""GPU: every device allocation of an object is gone when the object is closed (csrc/device_owned.h: the owners release themselves; no
list names them).  The guard bands count the library's live allocations exactly (_lib.check_guards), so each test records the count,
creates an object, touches every lazily allocated buffer of it once, closes it and asserts the count is back where it was -- and then
does all of it a second time, on the addresses the first round freed.  The equality is exact: a leaked buffer is +1.

Sizes: 17 x 33 with max_pairs = 4 (odd, no multiple of any tile); the depth network needs multiples of 32 and runs at 32 x 64."""
import gc
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, MAXP = 17, 33, 4


def _live():
    from tightly_coupled_sfm_amd import _lib
    n, bad = _lib.check_guards()
    assert n >= 0, "the GPU tests run with TCSFM_DEBUG_GUARDS=1 (tests/conftest.py)"
    assert bad == 0
    return n


def _twice(body):
    """`body` creates, touches and closes; the count of live allocations returns to its value both times"""
    gc.collect()        # engines that earlier tests dropped without closing go now, not in the middle of the count
    n0 = _live()
    for round_ in (1, 2):
        grown = body()
        assert grown > n0, f"round {round_}: the object allocated nothing?"
        torch.cuda.synchronize()
        assert _live() == n0, f"round {round_}: allocations left behind"


def _rand(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32)


def _K(h, w):
    return np.array([[0.58 * w, 0, 0.5 * w], [0, 1.9 * h, 0.5 * h], [0, 0, 1]], dtype=np.float32)


def _window(h, w, B=1, S=1):
    """a window in the layout of Engine.refine_window, on the GPU"""
    c = lambda t: t.cuda().contiguous()
    tgt, srcs = c(_rand(1, B, 3, h, w)), c(_rand(2, S, B, 3, h, w))
    dt, ds = c(1.0 + 0.2 * _rand(3, B, 1, h, w)), c(1.0 + 0.2 * _rand(4, S, B, 1, h, w))
    K = c(torch.from_numpy(_K(h, w))[None].repeat(B, 1, 1))
    pose = c(0.01 * (_rand(5, 2 * S * B, 6) - 0.5))
    return tgt, srcs, dt, ds, K, pose


def _sequence(h, w, T=3):
    frames, depths = _rand(6, T, 3, h, w).pin_memory(), (1.0 + 0.2 * _rand(7, T, 1, h, w)).pin_memory()
    return frames, depths, _K(h, w), np.zeros((T - 1, 2, 6), dtype=np.float32)


def test_engine_frees_every_lazy_allocation():
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine, default_opts

    def body():
        e = Engine(H, W, MAXP)
        tgt, srcs, dt, ds, K, pose = _window(H, W)
        N, img, d_s = 2, torch.cat([srcs[0], tgt]), torch.cat([ds[0], dt])
        d_t, K2 = torch.cat([dt, ds[0]]), K.repeat(2, 1, 1)
        g3, g1 = _rand(8, N, 3, H, W).cuda(), _rand(9, N, 1, H, W).cuda()
        e.inverse_warp2_backward(img, d_t, d_s, pose, K2, g_rec=g3)                        # warp backward without g_proj_depth ...
        e.inverse_warp2_backward(img, d_t, d_s, pose, K2, g_rec=g3, g_pd=g1, g_cd=g1)      # ... and with it (the fixed-point sums)
        e.compute_photometric_error_backward(torch.cat([tgt, srcs[0]]), img, d_t, d_s, pose, K2, g_diff=g1, g_weight=g1)
        e.scale_recovery(d_t, K2, 1.7)
        e.disp_post_process(g1, g1)
        e.resize_u8((255 * _rand(10, 1, 40, 70, 3)).to(torch.uint8).cuda())
        e.profile_begin()
        e.refine_window(tgt, srcs, dt, ds, K, pose)
        e.profile_end()
        e.set_lanes(2)
        for rule in (_lib.WINDOW_PAIR, _lib.WINDOW_REFERENCE):
            o = default_opts()
            o.window_rule = rule
            e.refine_dense_window(tgt, srcs, dt, ds, K, pose, opts=o)
        e.refine_sequence(*_sequence(H, W), sources=1)
        torch.cuda.synchronize()
        grown = _live()
        e.close()
        return grown

    _twice(body)


def test_posenet_frees_weights_scratch_and_its_lane_clone(monkeypatch):
    import standins
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    monkeypatch.setenv("TCSFM_LANE_PROBE", "0")         # the lanes stay on whatever the probe would find: window 1 runs on lane 1's clone

    def body():
        e = Engine(H, W, MAXP, lanes=2)
        n_engine = _live()
        net = PoseNetHIP(e, 2, standins.posenet_params(0))
        frames, depths, K, _ = _sequence(H, W)
        net.odometry_sequence(frames, depths, K, sources=1, iterations=1, windows_per_call=1)      # window 1 runs on lane 1: the clone
        imgs = _rand(11, 2, 6, H, W).cuda()
        pose, tape = net.forward_train(imgs)
        net.param_backward(imgs, tape, torch.ones_like(pose))
        torch.cuda.synchronize()
        grown = _live()
        net.close()
        assert n_engine < _live() < grown, "closing the network frees its buffers and leaves the engine's (the sequence ring) alone"
        e.close()
        return grown

    _twice(body)


def test_depthnet_frees_weights_training_state_and_its_sequence_clone():
    import depthnet_twin as dtw
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule

    h, w = 32, 64

    def body():
        mod = DepthNetModule(dtw.depthnet_params(0), max_images=2).cuda()
        x = torch.from_numpy(dtw.sample_images(3, 2, h, w)).cuda()
        disp = mod(x)[0][0]                                     # tcsfm_depthnet_load_device + the training forward
        disp.sum().backward()                                   # both backward walks
        nat = mod._native[(x.device.index, h, w)]
        nat.net.disp_for_eigen(x)                               # the instance's post-processing planes
        nat.eng.attach_depthnet(nat.net)                        # the sequence clone
        frames, _, K, p0 = _sequence(h, w)
        nat.eng.refine_sequence(frames, None, K, p0, sources=1, disparity="post")       # ... its activations and planes
        torch.cuda.synchronize()
        grown = _live()
        nat.net.close()
        nat.eng.close()
        return grown

    _twice(body)


def test_optimiser_frees_tables_moments_and_snapshot():
    from tightly_coupled_sfm_amd.engine import Engine
    from tightly_coupled_sfm_amd.optim import LibraryOptimizer

    def body():
        e = Engine(H, W, MAXP)
        n_engine = _live()
        ps = [_rand(12, 37).cuda().requires_grad_(True), _rand(13, 5, 3).cuda().requires_grad_(True)]
        opt = LibraryOptimizer(ps, kind="adam", engine=e)
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        opt.snapshot()
        opt.step()
        opt.restore()
        torch.cuda.synchronize()
        grown = _live()
        e._release(opt)
        assert _live() == n_engine, "the optimiser's five buffers go with it"
        e.close()
        return grown

    _twice(body)
