"""The per-frame scale stage of the sequence calls, without a GPU: the three entries of include/tcsfm.h (tcsfm_scale_recovery_frames,
tcsfm_sequence_scale, tcsfm_sequence_scales) against _lib.EXPORTS, their NULL-handle refusals, streaming.metric_poses against a NumPy
loop, the cam_height keyword's checks, and the ground-pixel counts the GPU tests rely on (both builds of the oracle)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW = ("tcsfm_scale_recovery_frames", "tcsfm_sequence_scale", "tcsfm_sequence_scales")
E_ARG = -1


def _prototype(name):
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "tcsfm.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{}]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/tcsfm.h"
    return [" ".join(d.split()) for d in m.group(1).split(",")]


def test_prototypes_are_in_the_header_and_in_exports():
    from tightly_coupled_sfm_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS, name
        _prototype(name)
    assert _prototype("tcsfm_scale_recovery_frames") == [
        "tcsfm_handle h", "const tcsfm_opts *o", "int N", "const void *depth", "const void *K", "float real_cam_height",
        "void *scale_out", "void *median_out", "int *count_out"]
    assert _prototype("tcsfm_sequence_scale") == ["tcsfm_handle h", "float real_cam_height"]
    assert _prototype("tcsfm_sequence_scales") == ["tcsfm_handle h", "int T", "void *scale_out", "void *median_out", "int *count_out"]
    # the signatures ctypes uses have the header's arity
    for name in NEW:
        assert len(_lib._SIGNATURES[name][1]) == len(_prototype(name)), name


def test_array_parameters_are_void_pointers():
    for name in NEW:
        for decl in _prototype(name):
            assert not re.search(r"\b(float|double)\s*\*", decl), (name, decl)
    # the prototypes of the three sequence calls are what they were
    assert len(_prototype("tcsfm_refine_sequence")) == 13 and len(_prototype("tcsfm_odometry_sequence")) == 15
    assert len(_prototype("tcsfm_refine_dense_sequence")) == 13


def test_null_handle_is_refused():
    from tightly_coupled_sfm_amd import _lib
    lib = _lib.load()
    assert lib.tcsfm_sequence_scale(None, 1.65) == E_ARG
    out = np.zeros(4, np.float32)
    assert lib.tcsfm_sequence_scales(None, 4, out.ctypes.data_as(C.c_void_p), None, None) == E_ARG
    assert not out.any()


def _loop(poses, scale, S, target_pos, unit):
    tp = (S + 1) // 2 if target_pos < 0 else target_pos
    out = np.array(poses, dtype=np.float32, copy=True)
    for w in range(out.shape[0]):
        f = np.float32(unit) * np.float32(scale[w + tp])
        for j in range(2 * S):
            for k in range(3):
                out[w, j, k] = np.float32(out[w, j, k] * f)
    return out


@pytest.mark.parametrize("S,target_pos", [(1, 0), (1, -1), (2, -1), (2, 0)])
def test_metric_poses_agree_with_a_numpy_loop(S, target_pos):
    torch = pytest.importorskip("torch")
    from tightly_coupled_sfm_amd import streaming
    T = 9
    rng = np.random.default_rng(7 + S)
    poses = rng.normal(scale=0.05, size=(T - S, 2 * S, 6)).astype(np.float32)
    scale = rng.uniform(0.02, 0.09, size=T).astype(np.float32)
    scale[3] = np.nan                                            # a frame without ground: its window's translations are NaN, nobody else's
    want = _loop(poses, scale, S, target_pos, 30.0)
    got = streaming.metric_poses(poses, scale, S, target_pos)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == poses.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[:, :, 3:], poses[:, :, 3:])         # rotations untouched
    tp = (S + 1) // 2 if target_pos < 0 else target_pos
    assert np.isnan(got[3 - tp, :, :3]).all() and np.isnan(got[:, :, :3]).sum() == 2 * S * 3
    assert np.array_equal(poses, np.asarray(poses))              # (the input is not modified)
    got_t = streaming.metric_poses(torch.from_numpy(poses), torch.from_numpy(scale), S, target_pos, depth_unit=12.5)
    assert isinstance(got_t, torch.Tensor)
    assert np.array_equal(got_t.numpy().view(np.int32), _loop(poses, scale, S, target_pos, 12.5).view(np.int32))
    with pytest.raises(ValueError):
        streaming.metric_poses(poses, scale[:-1], S, target_pos)
    with pytest.raises(ValueError):
        streaming.metric_poses(poses, scale, S, S + 1)


def test_cam_height_is_checked_before_anything_is_launched():
    """the check is the first statement of every method that takes the keyword: it raises on an object that has no handle at all"""
    from tightly_coupled_sfm_amd.engine import Engine, check_cam_height
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    assert check_cam_height(None) is None and check_cam_height(1.65) == 1.65 and check_cam_height(np.float32(2)) == 2.0
    assert check_cam_height(3) == 3.0
    for bad in ("1.65", [1.65], True, object()):
        with pytest.raises(TypeError):
            check_cam_height(bad)
    for bad in (-1.0, 0.0, float("nan"), float("inf"), -np.float32(0.1)):
        with pytest.raises(ValueError):
            check_cam_height(bad)
    bare = [(Engine.refine_sequence, object.__new__(Engine), (None, None, None, None)),
            (Engine.refine_dense_sequence, object.__new__(Engine), (None, None, None, None)),
            (PoseNetHIP.odometry_sequence, object.__new__(PoseNetHIP), (None, None, None)),
            (SequenceRefiner.run_native, object.__new__(SequenceRefiner), (None, None, None, None))]
    for fn, obj, args in bare:
        assert inspect.signature(fn).parameters["cam_height"].default is None, fn
        with pytest.raises(TypeError, match="cam_height"):
            fn(obj, *args, cam_height="1.65")
        with pytest.raises(ValueError, match="cam_height"):
            fn(obj, *args, cam_height=-1.65)


def test_ground_pixel_counts_of_the_gpu_tests_sequences(oracle32, oracle64):
    """tests/test_gpu_frame_scale.py relies on frames whose ground-pixel counts are all different, odd and even: both builds of the
    oracle agree on them"""
    from tightly_coupled_sfm_amd import synth
    seq = synth.make_sequence(11, 37, 53, seed=4)
    want = [625, 619, 613, 594, 584, 576, 567, 555, 545, 532, 522]
    for orc in (oracle32, oracle64):
        got = [int(orc.ground_height(seq["depths"][t, 0], seq["K"])[1].sum()) for t in range(11)]
        assert got == want, got
    seq = synth.make_sequence(11, 32, 64, seed=4)
    for orc in (oracle32, oracle64):
        got = [int(orc.ground_height(seq["depths"][t, 0], seq["K"])[1].sum()) for t in range(11)]
        assert len(set(got)) == 11 and 526 <= min(got) and max(got) <= 640, got
