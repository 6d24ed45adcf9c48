"""opts.host_ptrs = 1 on every entry point that stages its arrays: the library copies host arrays in, runs the same launches and
copies the results back.  Every call runs twice on the same inputs, once on NumPy arrays with host_ptrs = 1 and once on device
tensors, and every output must come back with the same bits."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

H, W = 24, 40


class Out:
    """an output the library stages (a device buffer in the device-pointer run)"""
    def __init__(self, *shape):
        self.shape = shape


class HostOut:
    """a float64 output the library writes on the host in both runs"""
    def __init__(self, *shape):
        self.shape = shape


def _ptr(a):
    return a.data_ptr() if torch.is_tensor(a) else a.ctypes.data


def _both(name, opts, *args, max_pairs=4):
    """lib.<name>(h, &opts, *args) with host_ptrs = 1 on NumPy arrays, then with host_ptrs = 0 on device tensors: same output bits"""
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine
    runs = []
    for host in (True, False):
        e = Engine(H, W, max_pairs)
        o = _lib.Opts()
        C.memmove(C.byref(o), C.byref(opts), C.sizeof(_lib.Opts))
        o.host_ptrs = 1 if host else 0
        keep, outs, cargs = [], [], []
        for a in args:
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a, dtype=np.float32)
                a = a if host else torch.from_numpy(a).cuda()
                keep.append(a); cargs.append(_ptr(a))
            elif isinstance(a, Out):
                buf = np.full(a.shape, -7.0, np.float32) if host else torch.full(a.shape, -7.0, device="cuda")
                outs.append(buf); cargs.append(_ptr(buf))
            elif isinstance(a, HostOut):
                buf = np.zeros(a.shape, np.float64)
                outs.append(buf); cargs.append(_ptr(buf))
            else:
                cargs.append(a)
        e._call(getattr(e.lib, name)(e._h, C.byref(o), *cargs))
        torch.cuda.synchronize()
        runs.append([b.cpu().numpy() if torch.is_tensor(b) else b for b in outs])
        e.close()
    for k, (a, b) in enumerate(zip(*runs)):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, k, np.nanmax(np.abs(a.astype(np.float64) - b)))
        assert np.isfinite(a).any(), (name, k)


def _pairs(N=2):
    from tightly_coupled_sfm_amd import synth
    return synth.make_batch(N, H, W, seed0=5, both_directions=True)


def _window(B=1, S=2, seed=11):
    """B targets of S sources each: tgt [B,3,H,W], srcs [S,B,3,H,W], depth_t [B,1,H,W], depth_s [S,B,1,H,W], K [B,3,3], pose [2SB,6]"""
    from tightly_coupled_sfm_amd import synth
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0 if s == 0 else -1.0)
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base, dtype=np.float32)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"][None] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"][None]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    return dict(tgt=np.stack(tg), srcs=np.stack([np.stack(x) for x in sr]), depth_t=np.stack(dt),
                depth_s=np.stack([np.stack(x) for x in ds]), K=np.stack(K), pose=np.concatenate([fwd, -fwd]).astype(np.float32))


def _opts(**kw):
    from tightly_coupled_sfm_amd.engine import default_opts
    return default_opts(**kw)


def test_disp_to_depth_ssim_and_smooth_loss():
    b = _pairs()
    disp = np.random.default_rng(0).uniform(0.05, 0.95, size=(2, 1, H, W)).astype(np.float32)
    _both("tcsfm_disp_to_depth", _opts(), disp.size, disp, Out(disp.size), Out(disp.size))
    _both("tcsfm_ssim", _opts(), 6, b["tgt"], b["src"], Out(2, 3, H, W))
    _both("tcsfm_smooth_loss", _opts(), 2, disp, b["tgt"], HostOut(1))


def test_warp_posenet_input_and_photometric():
    b = _pairs()
    p = (b["tgt"], b["src"], b["depth_t"], b["depth_s"], b["pose_init"], b["K"])
    _both("tcsfm_warp", _opts(), 2, *p[1:], Out(2, 3, H, W), Out(2, 1, H, W), Out(2, 1, H, W), Out(2, 1, H, W))
    _both("tcsfm_warp_posenet_input", _opts(), 2, *p, Out(2, 6, H, W), Out(2, 1, H, W))
    _both("tcsfm_photometric", _opts(), 2, *p, *(Out(2, 1, H, W) for _ in range(5)), Out(2, 3, H, W))


def test_linearize_linearize_window_and_loss_surface():
    from tightly_coupled_sfm_amd import _lib
    b = _pairs()
    ls = np.array([0.02, -0.03], np.float32)
    o = _opts(refine=_lib.REFINE_POSE_SCALE)
    _both("tcsfm_linearize", o, 2, b["tgt"], b["src"], b["depth_t"], b["depth_s"], b["pose_init"], ls, b["K"],
          HostOut(2, 7, 7), HostOut(2, 7), HostOut(2, 4))
    w = _window()
    ls4 = np.array([0.01, -0.02, 0.03, 0.0], np.float32)
    _both("tcsfm_linearize_window", _opts(refine=_lib.REFINE_POSE_SCALE, argmin=1), 1, 2, w["tgt"], w["srcs"], w["depth_t"], w["depth_s"],
          w["K"], w["pose"], ls4, HostOut(4, 7, 7), HostOut(4, 7), HostOut(4, 4))
    poses = b["pose_init"][0] + np.linspace(-0.01, 0.01, 3)[:, None].astype(np.float32)
    _both("tcsfm_loss_surface", _opts(), b["tgt"][0], b["src"][0], b["depth_t"][0], b["depth_s"][0], b["K"][:1], 3, poses, HostOut(3))


def test_refine_with_log_scale_and_scale_recovery():
    from tightly_coupled_sfm_amd import _lib
    b = _pairs()
    ls = np.array([0.02, -0.03], np.float32)
    _both("tcsfm_refine", _opts(n_iters=3, refine=_lib.REFINE_POSE_SCALE), 2, b["tgt"], b["src"], b["depth_t"], b["depth_s"], b["K"],
          b["pose_init"], ls, Out(2, 6), Out(2), Out(2, 4, _lib.NSTAT))
    _both("tcsfm_scale_recovery", _opts(), 2, b["depth_t"], b["K"], 1.65, 4, Out(1), Out(1), Out(2, H, W), Out(2, H, W))


def test_refine_dense_pair_form():
    from tightly_coupled_sfm_amd import _lib
    b = _pairs()
    for solver in (_lib.SOLVER_GN, _lib.SOLVER_LM):
        _both("tcsfm_refine_dense", _opts(n_iters=2, solver=solver), 2, b["tgt"], b["src"], b["depth_t"], b["depth_s"], b["K"], b["pose_init"],
              Out(2, 6), Out(2, 1, H, W), Out(2, 3, _lib.NSTAT))


@pytest.mark.parametrize("mode", ["pair", "joint", "reference"])
def test_refine_dense_window(mode):
    """the three forms of the dense window: per-pair depth copies, the library's joint mode, the reference's loss"""
    from tightly_coupled_sfm_amd import _lib
    w = _window()
    o = {"pair": _opts(n_iters=2, dense_joint=0, argmin=1),
         "joint": _opts(n_iters=2, dense_joint=1, argmin=1),
         "reference": _opts(n_iters=2, window_rule=_lib.WINDOW_REFERENCE, w_dc=0.15, argmin=1)}[mode]
    _both("tcsfm_refine_dense_window", o, 1, 2, w["tgt"], w["srcs"], w["depth_t"], w["depth_s"], w["K"], w["pose"],
          Out(4, 6), Out(4, 1, H, W), Out(4, 3, _lib.NSTAT))


@pytest.mark.parametrize("with_depth0", [False, True])
def test_linearize_dense_window_sources(with_depth0):
    from tightly_coupled_sfm_amd import _lib
    w = _window()
    d0 = (w["depth_t"] * 0.97).astype(np.float32) if with_depth0 else None
    _both("tcsfm_linearize_dense_window_sources", _opts(window_rule=_lib.WINDOW_REFERENCE, w_dc=0.15, argmin=1), 1, 2, w["tgt"], w["srcs"],
          w["depth_t"], w["depth_s"], w["K"], w["pose"], d0, HostOut(8), HostOut(4, 6), Out(1, 1, H, W), Out(2, 1, 1, H, W))
