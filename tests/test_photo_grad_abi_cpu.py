"""The photometric backward's two entry points at the product boundary, without a GPU: include/tcsfm.h declares them, the built
library exports them and the binding's table lists them with the right number of arguments (fails before the feature exists)."""
import os
import re

import pytest

from conftest import REPO

ENTRIES = {"tcsfm_photometric_maps_backward": 12,      # handle, opts, N, four inputs, two cotangents, three outputs
           "tcsfm_photometric_backward": 15}           # handle, opts, N, six inputs, three cotangents, three outputs


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
    """the wrappers exist; helpers.compute_photometric_error documents its gradient"""
    from tightly_coupled_sfm_amd import engine, helpers
    assert callable(engine.Engine.photometric_maps_backward) and callable(engine.Engine.compute_photometric_error_backward)
    assert "Differentiable" in helpers.compute_photometric_error.__doc__
