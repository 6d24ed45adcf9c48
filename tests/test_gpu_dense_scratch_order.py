"""The dense modes share one handle's scratch (csrc/dense_host.h: DenseScratch), every buffer allocated by whichever mode first needs it.
Four calls -- the reference's loss with the quarter-resolution unknown and free source maps, the reference's loss with the min over the
sources, the library's joint mode under LM, the pair form under LM -- run on ONE handle in two opposite orders; every pose and every
depth map must be, bit for bit, what the same call returns on a fresh handle: neither the order of the first allocations nor what an
earlier mode left in a shared buffer may reach a result."""
import numpy as np
import pytest
import torch

from tightly_coupled_sfm_amd import _lib

pytestmark = pytest.mark.gpu

H, W, MAX_PAIRS, S = 16, 48, 8, 2


def _window(B, seed=3):
    from tightly_coupled_sfm_amd import synth
    tg, dt, K, sr, ds, p0 = [], [], [], [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            base = np.array([0.003, -0.002, 0.033, 0.002, -0.004, 0.0015]) * (1.0, -1.0)[s]
            p = synth.make_pair(H, W, seed=seed + 7 * b, pose_gt=base)
            if s == 0:
                tg.append(p["tgt"]); dt.append(p["depth_t"] * 1.02); K.append(p["K"])
            sr[s].append(p["src"]); ds[s].append(p["depth_s"]); p0[s].append(synth.perturb_pose(p["pose_gt"], seed + s))
    fwd = np.concatenate([np.stack(x) for x in p0])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return (dev(np.stack(tg)), dev(np.stack([np.stack(x) for x in sr])), dev(np.stack(dt)[:, None]), dev(np.stack([np.stack(x) for x in ds])[:, :, None]), dev(np.stack(K)),
            dev(np.concatenate([fwd, -fwd])))


def _modes():
    from tightly_coupled_sfm_amd.engine import default_opts
    base = dict(n_iters=2, min_depth=0.06, max_depth=2.67)
    return [
        ("reference loss, quarter resolution, free source maps",
         default_opts(window_rule=_lib.WINDOW_REFERENCE, depth_param=_lib.DEPTH_QUARTER, free_source_depths=1, argmin=0, **base)),
        ("reference loss, argmin", default_opts(window_rule=_lib.WINDOW_REFERENCE, argmin=1, **base)),
        ("joint mode, LM", default_opts(window_rule=_lib.WINDOW_PAIR, dense_joint=1, solver=_lib.SOLVER_LM, **base)),
        ("pair form, LM", default_opts(window_rule=_lib.WINDOW_PAIR, dense_joint=0, solver=_lib.SOLVER_LM, **base)),
    ]


def _run(eng, w, o):
    pose, depth, _ = eng.refine_dense_window(*w, o)
    torch.cuda.synchronize()
    return pose.clone(), depth.clone()


@pytest.mark.parametrize("B", [1, 2])
def test_dense_results_do_not_depend_on_the_order_of_modes_on_a_handle(B):
    from tightly_coupled_sfm_amd.engine import Engine
    w, modes = _window(B), _modes()
    fresh = []
    for _, o in modes:
        eng = Engine(H, W, MAX_PAIRS)
        fresh.append(_run(eng, w, o))
        eng.close()
    for p, d in fresh:
        assert torch.isfinite(p).all() and torch.isfinite(d).all()
    assert not torch.equal(fresh[0][1], fresh[1][1]) and not torch.equal(fresh[2][1], fresh[3][1])      # (the modes are different computations)
    for order in (range(len(modes)), reversed(range(len(modes)))):
        eng = Engine(H, W, MAX_PAIRS)
        for i in order:
            name, o = modes[i]
            pose, depth = _run(eng, w, o)
            assert torch.equal(pose, fresh[i][0]), f"{name}: poses differ from a fresh handle's"
            assert torch.equal(depth, fresh[i][1]), f"{name}: depth maps differ from a fresh handle's"
        eng.close()
