"""cr_render_adaptive_region_* at the boundary, without a GPU: the header declares the two calls and their contract, the
version script exports them, the ctypes table mirrors the signatures, the documents name them, the built library has them
and refuses a null handle (a handle needs a device: the other refusals are in tests/test_gpu_adaptive_region.py), and the
ABI version did not move."""
import ctypes as C
import fnmatch
import os
import re

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cr_render_adaptive_region_device", "cr_render_adaptive_region_host")


def squeezed(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_header_declares_the_calls_and_the_contract():
    text = squeezed("include", "crucible_hip.h")
    for name, out, counts in zip(CALLS, ("d_out_rgb", "h_out_rgb"), ("d_counts", "h_counts")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, "
                f"const CrAdaptiveParams* adaptive, const CrRegion* region, "
                f"void* {out}, int32_t* {counts}, CrAdaptiveStats* stats);") in text
    raw = open(os.path.join(ROOT, "include", "crucible_hip.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", raw))   # without the comments' line starts
    for phrase in ("anchored at the region's origin (x0, y0)", "N_b counts the block's pixels inside the region",
                   "(y0 + j) * image_width + (x0 + i)", "BIT FOR BIT the pixel of cr_render_region_device with samples = counts[pixel]",
                   "the region's blocks are the frame's blocks", "A region that is the whole frame gives cr_render_adaptive_device's bytes, counts and stats",
                   "passes does not", "min_samples == params->samples is exactly cr_render_region_*",
                   "more than 2^26 pixels in the region", "up to 2^31 - 1 pixels", "a refused call leaves the handle as it was"):
        assert phrase in text, phrase
    assert "#define CR_ABI_VERSION 4" in text and A.CR_ABI_VERSION == 4
    # the structures the calls share keep their layouts
    assert C.sizeof(A.CrAdaptiveParams) == 24 and C.sizeof(A.CrRegion) == 16
    assert C.sizeof(A.CrAdaptiveStats) == C.sizeof(A.CrStats) + 24


def test_version_script_exports_them():
    text = squeezed("crucible_amd", "csrc", "exports.map")
    glob = re.search(r"global: ([^;]*);", text).group(1).split()
    local = re.search(r"local: ([^;]*);", text).group(1).split()
    assert local == ["*"]
    for name in CALLS:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name


def test_python_table_mirrors_the_signatures():
    want = (C.c_int32, [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.POINTER(A.CrAdaptiveParams),
                        C.POINTER(A.CrRegion), C.c_void_p, C.c_void_p, C.POINTER(A.CrAdaptiveStats)])
    for name in CALLS:
        assert A.SYMBOLS[name] == want, name


def test_documents_name_the_calls():
    integration = squeezed("INTEGRATION.md")
    for name in CALLS:
        assert f"pub fn {name}(" in integration, name
    design = squeezed("DESIGN.md")
    assert "6.13" in design and "cr_render_adaptive_region" in design
    assert "cr_render_adaptive_region_host" in squeezed("README.md")


def test_library_exports_them_and_refuses_a_null_handle(hiplib):
    for name in CALLS:
        assert hasattr(hiplib, name), name
    cd, p, ap, reg = A.CrCameraDesc(), A.CrRenderParams(), A.CrAdaptiveParams(4, 2, 4, 0, 0.01), A.CrRegion(0, 0, 2, 2)
    out = (C.c_double * 12)()
    counts = (C.c_int32 * 4)()
    for cam, params, adaptive, region in ((cd, p, ap, reg), (None, p, ap, reg), (cd, None, ap, reg), (cd, p, None, reg), (cd, p, ap, None),
                                          (None, None, None, None)):
        args = [C.byref(x) if x is not None else None for x in (cam, params, adaptive, region)]
        for name in CALLS:
            assert getattr(hiplib, name)(None, *args, out, counts, None) == A.CR_ERR_INVALID_ARG
            assert getattr(hiplib, name)(None, *args, out, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_abi_version() == 4
