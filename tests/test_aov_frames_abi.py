"""cr_render_aov_frames_device / cr_render_aov_frames_host at the boundary, without a GPU: the header declares them, the
ctypes table mirrors their signatures, the linker script lets them out, the built library exports them and refuses a null
handle, and the ABI version did not move."""
import ctypes as C
import fnmatch
import os
import re

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cr_render_aov_frames_device", "cr_render_aov_frames_host")


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())


def test_header_declares_the_guide_batch_calls():
    text = header()
    for name, out in zip(NAMES, ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers, "
                f"const int32_t* frames, int32_t n_frames, void* {out}, CrStats* stats);") in text


def test_abi_version_is_still_4():
    assert "#define CR_ABI_VERSION 4" in header()
    assert A.CR_ABI_VERSION == 4


def test_python_table_mirrors_the_signatures():
    want = [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
            C.c_void_p, C.POINTER(A.CrStats)]
    for name in NAMES:
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == want, name
    # test_abi.py's equality of the header's names and the table's, restated for the two
    declared = set(re.findall(r"CR_API [^;(]*?\b(cr_\w+)\(", header()))
    assert set(NAMES) <= declared and declared == set(A.SYMBOLS)


def test_exports_map_lets_them_out():
    text = open(os.path.join(ROOT, "crucible_amd", "csrc", "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:([^}]*?)local:", text, re.S).group(1).split(";") if p.strip()]
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name


def test_library_exports_them_and_refuses_a_null_handle(hiplib):
    for name in NAMES:
        fn = getattr(hiplib, name)
        assert fn.argtypes[3] is C.c_int32 and fn.argtypes[4] == C.POINTER(C.c_int32)
    frames = (C.c_int32 * 2)(0, 1)
    # a null handle is refused before anything touches a device
    assert hiplib.cr_render_aov_frames_host(None, None, None, A.CR_AOV_ALL, frames, 2, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_render_aov_frames_device(None, None, None, A.CR_AOV_ALL, frames, 2, None, None) == A.CR_ERR_INVALID_ARG
