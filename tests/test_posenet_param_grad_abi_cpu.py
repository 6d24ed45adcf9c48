"""The PoseNet parameter gradient's two entry points at the product boundary, without a GPU: include/tcsfm.h declares them, the
built library exports them and the binding's table lists them with the right number of arguments; the Python surface exists
(fails before the feature exists)."""
import os
import re

import pytest

from conftest import REPO

ENTRIES = {"tcsfm_posenet_load_device": 7,             # instance, four tables, head weight, head bias
           "tcsfm_posenet_param_backward": 12}         # instance, N, images, tape, pose cotangent, image gradient, four tables, two head outputs


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
    """the wrappers and the module exist; the module carries the reference's thirty parameters under its names"""
    import copy

    import standins
    from tightly_coupled_sfm_amd import posenet, posenet_train, train_mono
    for name in ("load_device", "param_backward"):
        assert callable(getattr(posenet.PoseNetHIP, name))
    mod = posenet_train.PoseNetModule(standins.posenet_params(3))
    twin = standins.PoseNetTwin(standins.posenet_params(3))
    assert [(k, tuple(p.shape)) for k, p in mod.named_parameters()] == [(k, tuple(p.shape)) for k, p in twin.named_parameters()]
    assert all(p.requires_grad for p in mod.parameters())
    clone = copy.deepcopy(mod)
    with __import__("torch").no_grad():
        clone.get_parameter("conv3.0.weight").add_(1.0)
    assert not bool((clone.get_parameter("conv3.0.weight") == mod.get_parameter("conv3.0.weight")).any())
    assert posenet_train.PoseNetModule(twin).get_parameter("pose_pred.weight").shape == (6, 256, 1, 1)
    with pytest.raises(NotImplementedError):
        mod(__import__("torch").zeros(1, 6, 8, 8), return_features=True)
    assert "PoseNetModule" in train_mono.__doc__
