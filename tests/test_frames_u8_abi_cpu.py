"""tcsfm_sequence_frame_format and tcsfm_frames_from_u8 at the product boundary, without a GPU: the header declares them with the
agreed parameter lists, the binding has them, a NULL handle is an argument error before anything touches HIP, and the Python sequence
methods sort their `frames` argument -- float32, uint8 planar, uint8 interleaved, or a TypeError -- before they bind a stream."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def lib():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    return _lib.load()


def _params(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"include/tcsfm.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_binding_exports_the_entries(lib):
    from tightly_coupled_sfm_amd import _lib
    hdr = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert _params(code, "tcsfm_sequence_frame_format") == ["tcsfm_handle h", "int format"]
    # bytes in, floats out, declared `void`: no float * / double * / [ for the overlap table to classify -- the entry enforces its one rule
    assert _params(code, "tcsfm_frames_from_u8") == ["tcsfm_handle h", "const tcsfm_opts *o", "int format", "int N", "const void *src", "void *dst"]
    for name, value in (("TCSFM_FRAMES_F32_CHW", 0), ("TCSFM_FRAMES_U8_CHW", 1), ("TCSFM_FRAMES_U8_HWC", 2)):
        assert re.search(r"^#define\s+" + name + r"\s+" + str(value) + r"\s*$", code, flags=re.M), name
    assert (_lib.FRAMES_F32_CHW, _lib.FRAMES_U8_CHW, _lib.FRAMES_U8_HWC) == (0, 1, 2)
    assert "const uint8_t *" in hdr and '"tcsfm_frames_from_u8: dst overlaps src"' in hdr
    # the honoured pairs are as they were: the new entry is described outside that list
    sec = hdr[hdr.index("The honoured pairs, entry by entry"):hdr.index("(end of the honoured pairs")]
    assert "frames_from_u8" not in sec and hdr.index("tcsfm_frames_from_u8") > hdr.index("(end of the honoured pairs")
    assert "tcsfm_sequence_frame_format" in _lib.EXPORTS and "tcsfm_frames_from_u8" in _lib.EXPORTS
    fn = lib.tcsfm_sequence_frame_format
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    fn = lib.tcsfm_frames_from_u8
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(_lib.Opts), C.c_int, C.c_int, C.c_void_p, C.c_void_p]


def test_null_handle_is_an_argument_error(lib):
    from tightly_coupled_sfm_amd import _lib
    for fmt in (0, 1, 2, 3):
        assert lib.tcsfm_sequence_frame_format(None, fmt) == -1
    o = _lib.default_opts()
    buf = (C.c_ubyte * 64)()
    assert lib.tcsfm_frames_from_u8(None, C.byref(o), 2, 1, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p)) == -1
    assert lib.tcsfm_frames_from_u8(None, None, 2, 1, None, None) == -1


def _bare_engine():
    """an Engine object without a handle: what the argument check sees before _bind()"""
    from tightly_coupled_sfm_amd.engine import Engine

    class Bare(Engine):
        def __init__(self):
            self.H, self.W, self._h = 32, 64, None
            self._seq_depthnet = None

        def _bind(self):
            raise AssertionError("the check runs before the stream is bound")

    return Bare()


def test_frame_format_helper_infers_the_layout():
    torch = pytest.importorskip("torch")
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import frame_format
    H, W = 32, 64
    assert frame_format(torch.zeros((5, 3, H, W)), H, W) == _lib.FRAMES_F32_CHW
    assert frame_format(torch.zeros((5, 3, H, W), dtype=torch.uint8), H, W) == _lib.FRAMES_U8_CHW
    assert frame_format(torch.zeros((5, H, W, 3), dtype=torch.uint8), H, W) == _lib.FRAMES_U8_HWC
    # the smallest frames the library takes: H, W >= 4, so [T,3,H,W] and [T,H,W,3] never coincide
    assert frame_format(torch.zeros((3, 3, 4, 4), dtype=torch.uint8), 4, 4) == _lib.FRAMES_U8_CHW
    assert frame_format(torch.zeros((3, 4, 4, 3), dtype=torch.uint8), 4, 4) == _lib.FRAMES_U8_HWC
    for bad in (torch.zeros((5, 3, H, W), dtype=torch.int16), torch.zeros((5, 3, H, W), dtype=torch.float64),
                torch.zeros((5, 3, W, H), dtype=torch.uint8), torch.zeros((5, H, W, 4), dtype=torch.uint8),
                torch.zeros((3, H, W), dtype=torch.uint8), torch.zeros((5, 3, H, W), dtype=torch.uint8, device="meta")):
        with pytest.raises(TypeError):
            frame_format(bad, H, W)


def test_python_sorts_frames_before_it_binds():
    torch = pytest.importorskip("torch")
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    e = _bare_engine()
    H, W = e.H, e.W
    depths = torch.ones((3, 1, H, W))
    p0 = torch.zeros((2, 2, 6))
    K = [[30.0, 0, 32], [0, 30.0, 16], [0, 0, 1]]
    pn = PoseNetHIP.__new__(PoseNetHIP)
    pn.eng, pn.lib, pn._pn = e, None, None
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, None, 1

    class OnTheGpu(torch.Tensor):
        """what a CUDA tensor shows the check (a machine without a GPU cannot make one)"""
        @property
        def device(self):
            return torch.device("cuda", 0)

        @property
        def is_cuda(self):
            return True

    bad = {"int16": torch.zeros((3, 3, H, W), dtype=torch.int16),
           "uint8, H and W swapped": torch.zeros((3, 3, W, H), dtype=torch.uint8),
           "uint8, four channels": torch.zeros((3, H, W, 4), dtype=torch.uint8),
           "cuda": torch.zeros((3, H, W, 3), dtype=torch.uint8).as_subclass(OnTheGpu)}
    for what, frames in bad.items():
        for call in (lambda f: e.refine_sequence(f, depths, K, p0), lambda f: e.refine_dense_sequence(f, depths, K, p0),
                     lambda f: pn.odometry_sequence(f, depths, K), lambda f: sr.run_native(f, depths, K, p0)):
            with pytest.raises(TypeError):
                call(frames)
    # good frames pass the check and reach _bind() -- with the layout inferred
    for frames, fmt in ((torch.zeros((3, 3, H, W)), _lib.FRAMES_F32_CHW), (torch.zeros((3, 3, H, W), dtype=torch.uint8), _lib.FRAMES_U8_CHW),
                        (torch.zeros((3, H, W, 3), dtype=torch.uint8), _lib.FRAMES_U8_HWC)):
        got, f = e._seq_frames(frames, 3)
        assert f == fmt and got.is_contiguous() and got.dtype == frames.dtype
        with pytest.raises(AssertionError, match="before the stream is bound"):
            e.refine_sequence(frames, depths, K, p0)
        with pytest.raises(AssertionError, match="before the stream is bound"):
            pn.odometry_sequence(frames, depths, K)
