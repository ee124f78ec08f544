"""cr_render_region_* / cr_render_aov_region_* at the boundary, without a GPU: the header declares them, the ctypes table
mirrors their signatures, the built library exports them and refuses a null handle (a handle needs a device: the null
cam, params and region refusals are in tests/test_gpu_region.py and tests/test_gpu_aov_region.py), CrRegion's layout agrees
between the header and ctypes, and the ABI version did not move."""
import ctypes as C
import os
import re
import subprocess

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAUTY = ("cr_render_region_device", "cr_render_region_host")
GUIDE = ("cr_render_aov_region_device", "cr_render_aov_region_host")


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())


def test_header_declares_the_region_calls():
    text = header()
    assert "typedef struct CrRegion { int32_t x0, y0, width, height; } CrRegion;" in text
    for name, out in zip(BEAUTY, ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, const CrRegion* region, "
                f"void* {out}, CrStats* stats);") in text
    for name, out in zip(GUIDE, ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers, "
                f"const CrRegion* region, void* {out}, CrStats* stats);") in text
    assert "#define CR_ABI_VERSION 4" in text and A.CR_ABI_VERSION == 4   # entry points were added without a bump before


def test_python_table_mirrors_the_signatures():
    head = [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams)]
    tail = [C.POINTER(A.CrRegion), C.c_void_p, C.POINTER(A.CrStats)]
    for name in BEAUTY:
        assert A.SYMBOLS[name] == (C.c_int32, head + tail), name
    for name in GUIDE:
        assert A.SYMBOLS[name] == (C.c_int32, head + [C.c_int32] + tail), name


def test_region_layout_matches_the_header(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "crucible_hip.h"\nint main(){\n'
    src += 'printf("CrRegion %zu\\n", sizeof(CrRegion));\n'
    for fname, _ in A.CrRegion._fields_:
        src += f'printf("{fname} %zu\\n", offsetof(CrRegion, {fname}));\n'
    src += "return 0;}\n"
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines() if line)
    assert int(got["CrRegion"]) == C.sizeof(A.CrRegion) == 16
    assert [f for f, _ in A.CrRegion._fields_] == ["x0", "y0", "width", "height"]
    for fname, _ in A.CrRegion._fields_:
        assert int(got[fname]) == getattr(A.CrRegion, fname).offset, fname


def test_library_exports_them_and_refuses_a_null_handle(hiplib):
    for name in BEAUTY + GUIDE:
        assert hasattr(hiplib, name), name
    cd, p, reg = A.CrCameraDesc(), A.CrRenderParams(), A.CrRegion(0, 0, 1, 1)
    out = (C.c_double * 8)()
    # a null handle is refused before anything touches a device, whatever else is null
    for cam, params, region in ((cd, p, reg), (None, p, reg), (cd, None, reg), (cd, p, None), (None, None, None)):
        args = [C.byref(x) if x is not None else None for x in (cam, params)]
        r = C.byref(region) if region is not None else None
        for name in BEAUTY:
            assert getattr(hiplib, name)(None, *args, r, out, None) == A.CR_ERR_INVALID_ARG
        for name in GUIDE:
            assert getattr(hiplib, name)(None, *args, A.CR_AOV_ALL, r, out, None) == A.CR_ERR_INVALID_ARG
