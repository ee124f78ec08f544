"""cr_render_adaptive_frames_* at the boundary, without a GPU: the header declares the two calls and their contract, the
version script exports them, the ctypes table mirrors the signatures, the built library has them and refuses a null handle
(a handle needs a device: the other refusals are in tests/test_gpu_adaptive_frames.py), and the ABI version did not move."""
import ctypes as C
import fnmatch
import os
import re

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cr_render_adaptive_frames_device", "cr_render_adaptive_frames_host")


def squeezed(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_header_declares_the_calls_and_the_contract():
    text = squeezed("include", "crucible_hip.h")
    for name, out, counts in zip(CALLS, ("d_out_rgb", "h_out_rgb"), ("d_counts", "h_counts")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, "
                f"const CrAdaptiveParams* adaptive, const int32_t* frames, int32_t n_frames, "
                f"void* {out}, int32_t* {counts}, CrAdaptiveStats* stats);") in text
    raw = open(os.path.join(ROOT, "include", "crucible_hip.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", raw))   # without the comments' line starts
    for phrase in ("params->frame itself is ignored", "a repeated frame has its own accumulators", "frame k at k * image_width*image_height*3 reals",
                   "BIT FOR BIT what cr_render_adaptive_device writes", "one 4-byte read-back", "48 bytes per pixel per frame",
                   "consecutive sub-batches of whole frames", "a null `frames` or n_frames < 1", "would refit or rebuild boxes",
                   "names the first failing frame"):
        assert phrase in text, phrase
    assert "#define CR_ABI_VERSION 4" in text and A.CR_ABI_VERSION == 4


def test_version_script_exports_them():
    text = squeezed("crucible_amd", "csrc", "exports.map")
    glob = re.search(r"global: ([^;]*);", text).group(1).split()
    local = re.search(r"local: ([^;]*);", text).group(1).split()
    assert local == ["*"]
    for name in CALLS:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name


def test_python_table_mirrors_the_signatures():
    want = (C.c_int32, [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.POINTER(A.CrAdaptiveParams),
                        C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(A.CrAdaptiveStats)])
    for name in CALLS:
        assert A.SYMBOLS[name] == want, name


def test_documents_name_the_calls():
    integration = squeezed("INTEGRATION.md")
    for name in CALLS:
        assert f"pub fn {name}(" in integration, name
    assert "6.12" in squeezed("DESIGN.md") and "cr_render_adaptive_frames_host" in squeezed("README.md")


def test_library_exports_them_and_refuses_a_null_handle(hiplib):
    for name in CALLS:
        assert hasattr(hiplib, name), name
    cd, p, ap = A.CrCameraDesc(), A.CrRenderParams(), A.CrAdaptiveParams(4, 2, 4, 0, 0.01)
    out = (C.c_double * 8)()
    counts = (C.c_int32 * 8)()
    frames = (C.c_int32 * 2)(0, 1)
    for cam, params, adaptive in ((cd, p, ap), (None, p, ap), (cd, None, ap), (cd, p, None), (None, None, None)):
        args = [C.byref(x) if x is not None else None for x in (cam, params, adaptive)]
        for name in CALLS:
            assert getattr(hiplib, name)(None, *args, frames, 2, out, counts, None) == A.CR_ERR_INVALID_ARG
            assert getattr(hiplib, name)(None, *args, None, 0, out, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_abi_version() == 4
