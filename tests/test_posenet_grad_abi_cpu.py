"""The PoseNet input gradient's four entry points at the product boundary, without a GPU: include/tcsfm.h declares them, the built
library exports them and the binding's table lists them with the right number of arguments (fails before the feature exists)."""
import os
import re

import pytest

from conftest import REPO

ENTRIES = {"tcsfm_posenet_tape_size": 3,               # instance, N, floats out
           "tcsfm_posenet_forward_train": 5,           # instance, N, images, pose out, tape
           "tcsfm_posenet_backward": 5,                # instance, N, tape, pose cotangent, image gradient out
           "tcsfm_debug_posenet_tape_layer": 8}        # instance, N, tape, layer, four read-outs


@pytest.fixture(scope="module")
def lib():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_point_declared_exported_and_bound(lib, name):
    from tightly_coupled_sfm_amd import _lib
    header = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name
    assert len(m.group(1).split(",")) == ENTRIES[name]
    assert name in _lib.EXPORTS and hasattr(lib, name)
    res, args = _lib._SIGNATURES[name]
    assert len(args) == ENTRIES[name]


def test_python_surface():
    """the wrappers exist; solve_pose_iteratively documents its gradient and what stays out of scope"""
    from tightly_coupled_sfm_amd import engine, posenet, train_mono
    for name in ("forward_train", "backward", "tape_layer", "tape_size"):
        assert callable(getattr(posenet.PoseNetHIP, name))
    assert callable(engine.Engine.posenet_input_autograd)
    assert "optimize_pose_weights_all" in train_mono.__doc__ and "optimize_pose_weights_all" in posenet.PoseNetHIP.__doc__
