"""The window loss's two entry points at the product boundary, without a GPU: include/tcsfm.h declares them, the built library exports
them and the binding's table lists them with the right number of arguments (fails before the feature exists)."""
import inspect
import os
import re

import pytest

from conftest import REPO

ENTRIES = {"tcsfm_window_loss": 16,                    # handle, opts, B, S, argmin, inverse, eight maps, loss, stats
           "tcsfm_window_loss_backward": 20}           # handle, opts, B, S, argmin, inverse, eight maps, stats, g_loss, four outputs


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


def test_header_cites_the_reference_lines():
    header = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    for name in ENTRIES:
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "optimizer.py:47-86" in comment, name


def test_python_surface():
    """the wrappers and the autograd Function exist; compute_optimization_loss has the `fused` keyword, off by default"""
    from tightly_coupled_sfm_amd import engine, losses
    assert callable(engine.Engine.window_loss) and callable(engine.Engine.window_loss_backward)
    assert issubclass(engine._WindowLoss, __import__("torch").autograd.Function)
    assert inspect.signature(losses.compute_optimization_loss).parameters["fused"].default is False
