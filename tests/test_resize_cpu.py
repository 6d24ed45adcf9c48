"""The camera-size resize without a GPU: the NumPy restatement of Pillow's 8-bit Lanczos resize (tests/resize_inputs.py) against the
fixture of Pillow's bytes and against Pillow itself where it is installed; the library's host table (tcsfm_resize_coeffs) against the
restatement's, entry by entry; tcsfm_scale_intrinsics against the double computation; the refusals that need no device.  Every
comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

import resize_inputs as R


@pytest.fixture(scope="module")
def lib():
    from tightly_coupled_sfm_amd import build, _lib
    build.build()
    return _lib.load()


ALL = [c[0] for c in R.CASES] + [s[0] for s in R.SEQUENCES]


def _sizes(name):
    c = R.CASE.get(name) or R.SEQUENCE[name]
    return c[1], c[2]


@pytest.mark.parametrize("name", ALL)
def test_restatement_returns_the_fixtures_bytes(name):
    g = R.golden()
    (h, w), (H, W) = _sizes(name)
    src = g["in_" + name]
    assert src.dtype == np.uint8 and src.shape[1:] == (h, w, 3) and g["out_" + name].shape == (src.shape[0], H, W, 3)
    out, _ = R.resize(src, H, W)
    assert np.array_equal(out, g["out_" + name])


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_fixture_inputs_are_the_generators_and_clip_on_both_sides(name):
    """every pass that runs sees a sum below 0 and one above 255 * 2^22 before its clip: the clamp is exercised on both sides"""
    g = R.golden()
    assert np.array_equal(g["in_" + name], R.make_input(name))
    (h, w), (H, W) = _sizes(name)
    _, stats = R.resize(g["in_" + name], H, W)
    assert (stats["h"] is None) == (w == W) and (stats["v"] is None) == (h == H)
    print(name, stats)
    assert R.clips_both_ways(stats), stats


def test_restatement_is_pillow():
    Image = pytest.importorskip("PIL.Image")
    g = R.golden()

    def pillow(frames, H, W):
        return np.stack([np.asarray(Image.fromarray(f, "RGB").resize((W, H), resample=Image.LANCZOS)) for f in frames])

    for name in ALL:
        (h, w), (H, W) = _sizes(name)
        assert np.array_equal(pillow(g["in_" + name], H, W), g["out_" + name]), name
    rng = np.random.default_rng(17)
    for (h, w), (H, W) in R.REAL:                            # the datasets' camera sizes
        im = rng.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)
        im[0, : h // 2, : w // 2] = (((np.arange(h // 2)[:, None] // 7) % 2) * 255)[:, :, None]
        im[0, h // 2:, w // 2:] = (((np.arange(w - w // 2)[None, :] // 9) % 2) * 255)[:, :, None]
        out, stats = R.resize(im, H, W)
        assert R.clips_both_ways(stats)
        assert np.array_equal(out, pillow(im, H, W)), (h, w)


INS = (157, 370, 375, 376, 968, 1226, 1241, 1242, 1296)
OUTS = (24, 40, 192, 256, 448, 640)
PAIRS = sorted({(o, o) for o in OUTS} | {(i, o) for i in INS for o in OUTS} | {(5, 8), (7, 16), (157, 640)})      # three with in < out named; more arise


def _lib_table(lib, inn, out):
    ks = C.c_int(-1)
    assert lib.tcsfm_resize_coeffs(inn, out, C.byref(ks), None, None) == 0
    bounds = np.full((out, 2), -77, dtype=np.int32)
    kk = np.full((out, ks.value), -77, dtype=np.int32)
    ks2 = C.c_int(-1)
    assert lib.tcsfm_resize_coeffs(inn, out, C.byref(ks2), bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p)) == 0
    assert ks2.value == ks.value
    return ks.value, bounds, kk


def test_library_table_is_the_restatements(lib):
    assert sum(1 for i, o in PAIRS if i < o) >= 3
    for inn, out in PAIRS:
        ks, bounds, kk = _lib_table(lib, inn, out)
        rks, rb, rk = R.coeffs(inn, out)
        assert ks == rks, (inn, out)
        assert np.array_equal(bounds, rb), (inn, out)
        assert np.array_equal(kk, rk), (inn, out)
        # what the kernel relies on: windows inside the input, moving monotonically; ksize bounds every window
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ks).all() and (bounds.sum(1) <= inn).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()


def test_library_table_refusals(lib):
    ks = C.c_int(5)
    assert lib.tcsfm_resize_coeffs(0, 4, C.byref(ks), None, None) == -1
    assert lib.tcsfm_resize_coeffs(4, 0, C.byref(ks), None, None) == -1
    assert lib.tcsfm_resize_coeffs(4, -1, C.byref(ks), None, None) == -1
    assert lib.tcsfm_resize_coeffs(4, 4, None, None, None) == -1
    assert ks.value == 5


def test_scale_intrinsics_is_the_double_computation(lib):
    rng = np.random.default_rng(3)
    for (h, w), (H, W) in R.REAL + [((370, 1226), (192, 640)), ((375, 1242), (192, 640)), ((5, 7), (8, 16))]:
        K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]], dtype=np.float32)
        K[:2] += rng.normal(size=(2, 3)).astype(np.float32)
        want = K.copy()
        want[0] = (K[0].astype(np.float64) * (float(W) / w)).astype(np.float32)
        want[1] = (K[1].astype(np.float64) * (float(H) / h)).astype(np.float32)
        got = np.full((3, 3), np.nan, dtype=np.float32)
        assert lib.tcsfm_scale_intrinsics(h, w, H, W, K.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (h, w)
        inplace = K.copy()                                   # K_out may be K_src
        assert lib.tcsfm_scale_intrinsics(h, w, H, W, inplace.ctypes.data_as(C.c_void_p), inplace.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(inplace.view(np.int32), want.view(np.int32))
    K = np.eye(3, dtype=np.float32)
    P = K.ctypes.data_as(C.c_void_p)
    assert lib.tcsfm_scale_intrinsics(0, 7, 8, 16, P, P) == -1
    assert lib.tcsfm_scale_intrinsics(5, 7, 8, -16, P, P) == -1
    assert lib.tcsfm_scale_intrinsics(5, 7, 8, 16, None, P) == -1 and lib.tcsfm_scale_intrinsics(5, 7, 8, 16, P, None) == -1
    assert np.array_equal(K, np.eye(3, dtype=np.float32))


def test_engine_scale_intrinsics(lib):
    from tightly_coupled_sfm_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.H, e.W, e._h = 192, 640, None
    K = [[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]
    got = e.scale_intrinsics(K, (376, 1241))
    K32 = np.asarray(K, dtype=np.float32).astype(np.float64)
    assert got.dtype == np.float32 and np.array_equal(got[0], (K32[0] * (640.0 / 1241)).astype(np.float32))
    assert np.array_equal(got[1], (K32[1] * (192.0 / 376)).astype(np.float32)) and np.array_equal(got[2], [0, 0, 1])
    with pytest.raises(ValueError):
        e.scale_intrinsics(K, (0, 1241))


def _params(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"include/tcsfm.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_binding_exports_the_entries(lib):
    from tightly_coupled_sfm_amd import _lib
    hdr = open(os.path.join(REPO, "include", "tcsfm.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert _params(code, "tcsfm_sequence_frame_source") == ["tcsfm_handle h", "int src_h", "int src_w"]
    assert _params(code, "tcsfm_resize_u8") == ["tcsfm_handle h", "const tcsfm_opts *o", "int format", "int N", "int src_h", "int src_w",
                                                "const void *src", "int dst_format", "void *dst"]
    assert _params(code, "tcsfm_resize_coeffs") == ["int in", "int out", "int *ksize_out", "int *bounds", "int *kk"]
    assert _params(code, "tcsfm_scale_intrinsics")[:4] == ["int src_h", "int src_w", "int H", "int W"]
    for name in ("tcsfm_sequence_frame_source", "tcsfm_resize_u8", "tcsfm_resize_coeffs", "tcsfm_scale_intrinsics"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert '"tcsfm_resize_u8: dst overlaps src"' in hdr


def test_null_handle_is_an_argument_error(lib):
    from tightly_coupled_sfm_amd import _lib
    for hw in ((0, 0), (47, 79), (-1, 5), (0, 5)):
        assert lib.tcsfm_sequence_frame_source(None, *hw) == -1
    o = _lib.default_opts()
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.tcsfm_resize_u8(None, C.byref(o), 2, 1, 5, 7, p, 2, p) == -1
    assert lib.tcsfm_resize_u8(None, None, 2, 1, 5, 7, None, 0, None) == -1


def _bare_engine(H=24, W=40):
    from tightly_coupled_sfm_amd.engine import Engine

    class Bare(Engine):
        def __init__(self):
            self.H, self.W, self._h = H, W, None
            self._seq_depthnet = None

        def _bind(self):
            raise AssertionError("the check runs before the stream is bound")

    return Bare()


def test_python_checks_source_size_before_it_binds():
    """the setter's arguments, as the Python entry points see them: a bad size or a tensor that is not source-size bytes raises before
    anything touches the GPU; a uint8 tensor of the wrong shape WITHOUT source_size raises what it raised before"""
    torch = pytest.importorskip("torch")
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import source_frame_format
    from tightly_coupled_sfm_amd.posenet import PoseNetHIP
    from tightly_coupled_sfm_amd.streaming import SequenceRefiner
    e = _bare_engine()
    H, W, h, w, T = e.H, e.W, 47, 79, 3
    depths = torch.ones((T, 1, H, W))
    p0 = torch.zeros((T - 1, 2, 6))
    K = [[30.0, 0, 20], [0, 30.0, 12], [0, 0, 1]]
    pn = PoseNetHIP.__new__(PoseNetHIP)
    pn.eng, pn.lib, pn._pn = e, None, None
    sr = SequenceRefiner.__new__(SequenceRefiner)
    sr.eng, sr.opts, sr.S = e, None, 1
    hwc, chw = torch.zeros((T, h, w, 3), dtype=torch.uint8), torch.zeros((T, 3, h, w), dtype=torch.uint8)
    assert source_frame_format(hwc, (h, w)) == _lib.FRAMES_U8_HWC and source_frame_format(chw, (h, w)) == _lib.FRAMES_U8_CHW
    calls = (lambda f, **kw: e.refine_sequence(f, depths, K, p0, **kw), lambda f, **kw: e.refine_dense_sequence(f, depths, K, p0, **kw),
             lambda f, **kw: pn.odometry_sequence(f, depths, K, **kw), lambda f, **kw: sr.run_native(f, depths, K, p0, **kw))
    for call in calls:
        for size in ((-1, w), (h, 0), (0, 0)):
            with pytest.raises(ValueError):
                call(hwc, source_size=size)
        for size in ((h,), "hw", 47):
            with pytest.raises(TypeError):
                call(hwc, source_size=size)
        for bad in (torch.zeros((T, w, h, 3), dtype=torch.uint8), torch.zeros((T, 3, h, w)), torch.zeros((T, h, w, 4), dtype=torch.uint8)):
            with pytest.raises(TypeError):
                call(bad, source_size=(h, w))
        with pytest.raises(TypeError, match=r"uint8 frames must be"):      # camera-size bytes without the keyword: the size is never guessed
            call(hwc)
        for good in (hwc, chw):
            with pytest.raises(AssertionError, match="before the stream is bound"):
                call(good, source_size=(h, w))
