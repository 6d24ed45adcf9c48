"""The flip post-processing without a GPU: the NumPy restatement the GPU tests compare against equals the reference's own output
(tests/golden/golden_disp_post.npz, made by make_golden_disp_post.py) bit for bit, and tcsfm_flip_ramp -- the table the device blend
reads -- has NumPy's bits of the reference's ramp, np.linspace included."""
import ctypes as C

import numpy as np
import pytest

import disp_post_inputs as D

E_ARG = -1


@pytest.mark.parametrize("k", range(len(D.GOLDEN_SHAPES)), ids=["x".join(map(str, s)) for s in D.GOLDEN_SHAPES])
def test_restatement_has_the_references_bits(k):
    l, r, post = D.golden()[k]
    assert l.shape == D.GOLDEN_SHAPES[k] and l.dtype == np.float32 and r.dtype == np.float32 and post.dtype == np.float64
    got = D.post_process(l, r)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), post.view(np.int64))
    assert not np.array_equal(post, l.astype(np.float64))          # (the blend did something)


@pytest.fixture(scope="module")
def lib():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("W", [2, 32, 33, 64, 96, 640, 1248])
def test_flip_ramp_has_numpys_bits(lib, W):
    out = np.full(W + 1, -7.0)
    assert lib.tcsfm_flip_ramp(W, out.ctypes.data_as(C.c_void_p)) == 0
    want = 1.0 - np.clip(20 * (np.linspace(0, 1, W) - 0.05), 0, 1)
    assert np.array_equal(out[:W].view(np.int64), want.view(np.int64))
    assert out[W] == -7.0                                           # nothing written past W
    assert out[0] == 1.0 and out[W - 1] == 0.0


def test_flip_ramp_refuses_a_width_below_two(lib):
    out = np.full(4, -7.0)
    for W in (1, 0, -3):
        assert lib.tcsfm_flip_ramp(W, out.ctypes.data_as(C.c_void_p)) == E_ARG
    assert lib.tcsfm_flip_ramp(2, None) == E_ARG
    assert (out == -7.0).all()


def test_engine_flip_ramp_wrapper():
    from tightly_coupled_sfm_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.W = 64
    assert np.array_equal(Engine.flip_ramp(e), D.ramp(64)) and np.array_equal(Engine.flip_ramp(e, 33), D.ramp(33))
    with pytest.raises(ValueError, match="flip_ramp"):
        Engine.flip_ramp(e, 1)
