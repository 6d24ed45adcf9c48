"""The depth evaluation entries at the product boundary, without a GPU: the header declares them with the agreed parameter lists and
constants, the binding has them, tcsfm_depth_eval_opts has the header's size and layout, tcsfm_depth_eval_default_opts fills it,
tcsfm_depth_eval_crop returns the twin's integers (tests/depth_eval_inputs.py), and a NULL handle is an argument error before
anything touches HIP."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO

import depth_eval_inputs as D

SIZES = [(375, 1242), (370, 1226), (376, 1241), (11, 37), (33, 70), (5, 9), (6, 20), (1, 37), (11, 1), (1, 1)]


@pytest.fixture(scope="module")
def lib():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    return _lib.load()


def _params(code, name, ret="int"):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"include/tcsfm.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_binding_exports_the_entries(lib):
    from tightly_coupled_sfm_amd import _lib
    hdr = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert _params(code, "tcsfm_depth_eval_default_opts", "void") == ["tcsfm_depth_eval_opts *e"]
    assert _params(code, "tcsfm_depth_eval_crop") == ["int protocol", "int gt_h", "int gt_w", "int *crop_out"]
    assert _params(code, "tcsfm_depth_eval") == ["tcsfm_handle h", "const tcsfm_opts *o", "const tcsfm_depth_eval_opts *e", "int N", "int disp_is_f64",
                                                 "const void *disp", "int gt_h", "int gt_w", "const void *gt", "void *metrics_out"]
    assert _params(code, "tcsfm_sequence_depth_eval") == ["tcsfm_handle h", "const tcsfm_depth_eval_opts *e", "int T", "int first", "int count",
                                                          "int gt_h", "int gt_w", "const void *gt", "void *metrics_out"]
    for name, value in (("TCSFM_EVAL_EIGEN", 0), ("TCSFM_EVAL_EIGEN_BENCHMARK", 1), ("TCSFM_NEVAL", 10)):
        assert re.search(r"^#define\s+" + name + r"\s+" + str(value) + r"\s*$", code, flags=re.M), name
    assert (_lib.EVAL_EIGEN, _lib.EVAL_EIGEN_BENCHMARK, _lib.NEVAL) == (0, 1, 10) == (D.EIGEN, D.EIGEN_BENCHMARK, D.NEVAL)
    for name in ("tcsfm_depth_eval_default_opts", "tcsfm_depth_eval_crop", "tcsfm_depth_eval", "tcsfm_sequence_depth_eval"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    fn = lib.tcsfm_depth_eval
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(_lib.Opts), C.POINTER(_lib.DepthEvalOpts), C.c_int, C.c_int,
                                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fn = lib.tcsfm_sequence_depth_eval
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(_lib.DepthEvalOpts)] + [C.c_int] * 5 + [C.c_void_p] * 2


def test_opts_struct_matches_header(lib):
    from tightly_coupled_sfm_amd import _lib
    fields = ("protocol", "median_scaling", "min_depth", "max_depth", "depth_unit", "lds_pairs")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tcsfm.h"\nint main(void){printf("%zu", sizeof(tcsfm_depth_eval_opts));' + \
          "".join(f'printf(" %zu", offsetof(tcsfm_depth_eval_opts, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [C.sizeof(_lib.DepthEvalOpts)] + [getattr(_lib.DepthEvalOpts, f).offset for f in fields]
    assert got == [32, 0, 4, 8, 12, 16, 24]


def test_default_opts(lib):
    from tightly_coupled_sfm_amd import _lib
    e = _lib.DepthEvalOpts()
    C.memset(C.byref(e), 0xFF, C.sizeof(e))
    lib.tcsfm_depth_eval_default_opts(C.byref(e))
    assert (e.protocol, e.median_scaling, e.lds_pairs) == (_lib.EVAL_EIGEN, 1, -1)
    assert e.min_depth == float(np.float32(1e-3)) and e.max_depth == 80.0 and e.depth_unit == 30.0
    assert bytes(e)[28:] == b"\0\0\0\0"                                         # the padding is cleared too
    lib.tcsfm_depth_eval_default_opts(None)                                     # tolerated
    e = _lib.depth_eval_opts("eigen_benchmark", False, 0.5, 20.0, 5.4, 7)
    assert (e.protocol, e.median_scaling, e.min_depth, e.max_depth, e.depth_unit, e.lds_pairs) == (1, 0, 0.5, 20.0, 5.4, 7)
    with pytest.raises(ValueError):
        _lib.depth_eval_opts("scannet")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crop_is_the_twins(lib, size):
    from tightly_coupled_sfm_amd import _lib
    gt_h, gt_w = size
    for protocol in (D.EIGEN, D.EIGEN_BENCHMARK):
        c = (C.c_int * 4)(-1, -1, -1, -1)
        assert lib.tcsfm_depth_eval_crop(protocol, gt_h, gt_w, c) == 0
        assert tuple(c) == D.crop(protocol, gt_h, gt_w) == _lib.depth_eval_crop(protocol, gt_h, gt_w)


def test_crop_refusals(lib):
    from tightly_coupled_sfm_amd import _lib
    c = (C.c_int * 4)(-1, -1, -1, -1)
    for args in ((2, 11, 37), (-1, 11, 37), (0, 0, 37), (0, 11, 0), (1, -3, 4)):
        assert lib.tcsfm_depth_eval_crop(*args, c) == -1
        assert tuple(c) == (-1, -1, -1, -1)
    assert lib.tcsfm_depth_eval_crop(0, 11, 37, None) == -1
    with pytest.raises(ValueError):
        _lib.depth_eval_crop(2, 11, 37)


def test_null_handle_is_an_argument_error(lib):
    from tightly_coupled_sfm_amd import _lib
    o, e = _lib.default_opts(), _lib.depth_eval_opts()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.tcsfm_depth_eval(None, C.byref(o), C.byref(e), 1, 1, p, 2, 2, p, p) == -1
    assert lib.tcsfm_depth_eval(None, None, None, 1, 1, None, 2, 2, None, None) == -1
    assert lib.tcsfm_sequence_depth_eval(None, C.byref(e), 3, 0, 1, 2, 2, p, p) == -1
    assert lib.tcsfm_sequence_depth_eval(None, None, 3, 0, 1, 2, 2, None, None) == -1


def test_host_compute_errors_matches_the_reference():
    from tightly_coupled_sfm_amd import evaluate_depth_eigen as ev
    g = D.golden()
    for k in range(int(g["n_cases"])):
        gt, pred, bench = g[f"gt{k}"], g[f"pred{k}"], int(g[f"bench{k}"])
        m = D.mask_of(gt, bench, 1e-3, 80.0)
        p = np.clip(pred[m] * float(g[f"ratio{k}"]), 0, 80)
        p[p < 1e-3] = 1e-3
        got, want = np.array(ev.compute_errors(gt[m], p)), g[f"errors{k}"]
        # a restatement of the reference's metrics in the inputs' own types; the float32 log and the sums' order may differ between CPUs
        assert np.array_equal(got[4:], want[4:]) and abs(got[3] - want[3]) <= 1e-6
        assert np.allclose(got[:3], want[:3], rtol=D.summed_bound(m.sum()), atol=0)


def test_table_and_ground_truth_loader(tmp_path):
    from tightly_coupled_sfm_amd import evaluate_depth_eigen as ev
    res = dict(med=9.8765, std=0.04321, mean_errors=np.array([0.1234, 1.5, 4.75, 0.2, 0.85, 0.95, 0.985]))
    assert ev.format_table(res) == (" Scaling ratios | med: 9.877 | std: 0.043\n\n"
                                    "   abs_rel |   sq_rel |     rmse | rmse_log |       a1 |       a2 |       a3 | \n"
                                    "& 0.123 & 1.500 & 4.750 & 0.200 & 0.850 & 0.950 & 0.985 ")
    assert ev.format_table(dict(res, med=None, std=None)).startswith("\n   abs_rel |")
    planes = np.empty(2, dtype=object)
    planes[0], planes[1] = np.ones((3, 5), np.float32), np.zeros((4, 6), np.float32)      # sizes differ: an object array, pickled
    np.savez(tmp_path / "gt_depths.npz", data=planes)
    got = ev.load_gt_depths(str(tmp_path / "gt_depths.npz"))
    assert len(got) == 2 and got[0].shape == (3, 5) and got[1].shape == (4, 6) and got[0].dtype == np.float32
