"""cr_render_aov_device / cr_render_aov_host / cr_write_pfm at the boundary, without a GPU: the header declares them, the
ctypes table mirrors their signatures, the built library exports them and refuses a null handle, and the PFM writer
produces the file format byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cr_render_aov_device", "cr_render_aov_host", "cr_write_pfm")


def test_header_declares_the_calls():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())
    for name, out in (("cr_render_aov_device", "d_out"), ("cr_render_aov_host", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, "
                f"int32_t layers, void* {out}, CrStats* stats);") in text
    assert ("CR_API int32_t cr_write_pfm(const char* path, const void* data, int32_t real_type, int32_t width, "
            "int32_t height, int32_t channels /* 1 | 3 */);") in text
    assert "enum { CR_AOV_ALBEDO = 1, CR_AOV_NORMAL = 2, CR_AOV_DEPTH = 4, CR_AOV_COVERAGE = 8 };" in text
    assert "#define CR_ABI_VERSION 4" in text and A.CR_ABI_VERSION == 4
    assert (A.CR_AOV_ALBEDO, A.CR_AOV_NORMAL, A.CR_AOV_DEPTH, A.CR_AOV_COVERAGE) == (1, 2, 4, 8)


def test_python_table_and_docs_name_the_calls():
    want = [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.c_int32, C.c_void_p, C.POINTER(A.CrStats)]
    for name in NAMES[:2]:
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == want, name
    assert A.SYMBOLS["cr_write_pfm"] == (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32])
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    assert "cr_*" in open(os.path.join(ROOT, "crucible_amd", "csrc", "exports.map")).read()


def test_library_exports_the_calls_and_refuses_a_null_handle(hiplib):
    for name in NAMES:
        assert getattr(hiplib, name).restype is C.c_int32
    assert hiplib.cr_render_aov_host(None, None, None, A.CR_AOV_ALL, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_render_aov_device(None, None, None, A.CR_AOV_ALL, None, None) == A.CR_ERR_INVALID_ARG


def read_pfm(path):
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 3)
    return head[0], head[1], head[2], head[3]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("channels", [1, 3])
def test_write_pfm_round_trips(hiplib, tmp_path, dtype, channels):
    from crucible_amd.renderer import write_pfm
    W, H = 5, 3
    rs = np.random.RandomState(4)
    a = rs.uniform(-2.0, 2.0, size=(H, W) if channels == 1 else (H, W, 3)).astype(dtype)
    a.flat[1] = np.inf
    a.flat[7] = -np.inf
    a.flat[9] = 1.0 + 2.0 ** -30   # f64: rounds to f32
    path = str(tmp_path / "x.pfm")
    write_pfm(path, a)
    magic, size, scale, data = read_pfm(path)
    assert (magic, size, scale) == (b"Pf" if channels == 1 else b"PF", b"5 3", b"-1.0")
    assert len(data) == W * H * channels * 4
    got = np.frombuffer(data, dtype="<f4").reshape(a.shape)
    assert got.tobytes() == a.astype(np.float32)[::-1].tobytes()   # rows bottom to top
    assert np.isposinf(got[::-1].flat[1]) and np.isneginf(got[::-1].flat[7])


def test_write_pfm_refusals(hiplib, tmp_path):
    a = np.zeros((3, 5), dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    ok = str(tmp_path / "y.pfm").encode()
    for ch in (0, 2, 4, -1):
        assert hiplib.cr_write_pfm(ok, p, A.CR_REAL_F32, 5, 3, ch) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_write_pfm(ok, p, 7, 5, 3, 1) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_write_pfm(ok, p, A.CR_REAL_F32, 0, 3, 1) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_write_pfm(None, p, A.CR_REAL_F32, 5, 3, 1) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_write_pfm(ok, None, A.CR_REAL_F32, 5, 3, 1) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_write_pfm(b"/nonexistent_dir/x.pfm", p, A.CR_REAL_F32, 5, 3, 1) == A.CR_ERR_IO
    assert not os.path.exists(ok.decode())
