"""tcsfm_sequence_depthnet at the product boundary, without a GPU: the header declares it, the binding has it, a NULL handle is an
argument error before anything touches HIP, and the Python sequence methods refuse depths=None without an attachment before they
bind a stream."""
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


def test_header_declares_and_binding_exports_the_entry(lib):
    from tightly_coupled_sfm_amd import _lib
    hdr = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"\bint\s+tcsfm_sequence_depthnet\s*\(([^)]*)\)\s*;", code)
    assert m, "include/tcsfm.h does not declare tcsfm_sequence_depthnet"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["tcsfm_handle h", "tcsfm_depthnet *dn"]             # no array parameter: nothing for the overlap table
    assert code.index("typedef struct tcsfm_depthnet tcsfm_depthnet") < m.start()
    assert "tcsfm_sequence_depthnet" in _lib.EXPORTS
    fn = lib.tcsfm_sequence_depthnet
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    # the three sequence entries document the NULL depths; the old sentence is gone
    assert "minus the depth network" not in hdr and hdr.count("depths == NULL") >= 3


def test_null_handle_is_an_argument_error(lib):
    assert lib.tcsfm_sequence_depthnet(None, None) == -1
    assert lib.tcsfm_sequence_depthnet(None, C.c_void_p(0)) == -1


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


def test_python_refuses_depths_none_without_an_attachment():
    torch = pytest.importorskip("torch")
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    e = _bare_engine()
    frames = torch.zeros((3, 3, 32, 64))
    p0 = torch.zeros((2, 2, 6))
    K = [[30.0, 0, 32], [0, 30.0, 16], [0, 0, 1]]
    with pytest.raises(ValueError, match="attach_depthnet"):
        e.refine_sequence(frames, None, K, p0)
    with pytest.raises(ValueError, match="attach_depthnet"):
        e.refine_dense_sequence(frames, None, K, p0)
    pn = PoseNetHIP.__new__(PoseNetHIP)
    pn.eng, pn.lib, pn._pn = e, None, None
    with pytest.raises(ValueError, match="attach_depthnet"):
        pn.odometry_sequence(frames, None, K)
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, None, 1
    with pytest.raises(ValueError, match="attach_depthnet"):
        sr.run_native(frames, None, K, p0)
    # a closed network does not count as attached
    class Closed:
        eng, _dn = e, None
    e._seq_depthnet = Closed()
    with pytest.raises(ValueError, match="attach_depthnet"):
        e.refine_sequence(frames, None, K, p0)
    # and attach_depthnet itself refuses what is not a network of this engine, before any library call
    with pytest.raises(ValueError, match="DepthNetHIP"):
        e.attach_depthnet(object())
