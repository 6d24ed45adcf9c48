"""The disparity stage of the sequence calls, without a GPU: the five entries of include/tcsfm.h against _lib.EXPORTS and ctypes'
signatures, the NULL-handle refusals, and the `disparity` keyword's checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

E_ARG = -1
PROTOTYPES = {
    "tcsfm_sequence_disparity": ["tcsfm_handle h", "int mode"],
    "tcsfm_sequence_disparities": ["tcsfm_handle h", "int T", "int first", "int count", "void *out", "int *mode_out"],
    "tcsfm_disp_post_process": ["tcsfm_handle h", "const tcsfm_opts *o", "int N", "const void *l_disp", "const void *r_disp_mirrored", "void *out"],
    "tcsfm_depthnet_disp_for_eigen": ["tcsfm_depthnet *dn", "const tcsfm_opts *o", "int N", "const void *imgs", "void *out"],
    "tcsfm_flip_ramp": ["int W", "void *l_mask_out"],
}


def _header():
    return open(os.path.join(REPO, "include", "tcsfm.h")).read()


def _prototype(name):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{}]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/tcsfm.h"
    return [" ".join(d.split()) for d in m.group(1).split(",")]


def test_prototypes_are_in_the_header_and_exported():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name, want in PROTOTYPES.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert _prototype(name) == want, name
        assert len(_lib._SIGNATURES[name][1]) == len(want), name
    hdr = _header()
    for k, (macro, const) in enumerate((("TCSFM_SEQ_DISP_OFF", _lib.SEQ_DISP_OFF), ("TCSFM_SEQ_DISP_PLAIN", _lib.SEQ_DISP_PLAIN),
                                        ("TCSFM_SEQ_DISP_POST", _lib.SEQ_DISP_POST))):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(k) + r"\b", hdr) and const == k, macro
    # the prototypes of the three sequence calls are what they were
    assert len(_prototype("tcsfm_refine_sequence")) == 13 and len(_prototype("tcsfm_odometry_sequence")) == 15
    assert len(_prototype("tcsfm_refine_dense_sequence")) == 13


def test_null_handle_is_refused():
    from tightly_coupled_sfm_amd import _lib
    lib = _lib.load()
    for mode in (0, 1, 2, 7):
        assert lib.tcsfm_sequence_disparity(None, mode) == E_ARG
    out = np.zeros(4, np.float64)
    mode = C.c_int(-5)
    assert lib.tcsfm_sequence_disparities(None, 4, 0, 1, out.ctypes.data_as(C.c_void_p), C.byref(mode)) == E_ARG
    assert not out.any() and mode.value == -5


def test_disparity_keyword_is_checked_before_anything_is_launched():
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine, check_disparity
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    assert check_disparity(None) == _lib.SEQ_DISP_OFF and check_disparity("plain") == _lib.SEQ_DISP_PLAIN
    assert check_disparity("post") == _lib.SEQ_DISP_POST
    for bad in (1, True, b"post"):
        with pytest.raises(TypeError, match="disparity"):
            check_disparity(bad)
    with pytest.raises(ValueError, match="disparity"):
        check_disparity("eigen")
    frames = np.zeros((3, 3, 8, 8), np.float32)
    for fn, obj, args in ((Engine.refine_sequence, Engine.__new__(Engine), (frames, None, None, None)),
                          (Engine.refine_dense_sequence, Engine.__new__(Engine), (frames, None, None, None)),
                          (PoseNetHIP.odometry_sequence, PoseNetHIP.__new__(PoseNetHIP), (frames, None, None)),
                          (SequenceRefiner.run_native, SequenceRefiner.__new__(SequenceRefiner), (frames, None, None, None))):
        assert inspect.signature(fn).parameters["disparity"].default is None, fn
        with pytest.raises(ValueError, match="disparity"):
            fn(obj, *args, disparity="both")
        with pytest.raises(TypeError, match="disparity"):
            fn(obj, *args, disparity=2)
