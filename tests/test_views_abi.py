"""cr_render_views_* / cr_render_aov_views_* at the boundary, without a GPU: the header declares the four calls, the ctypes
table mirrors their signatures, the linker script lets them out, the built library exports them and refuses null arguments
before anything touches a device, and the ABI version did not move.  The host half of the feature is checked here too:
tests/views_pack_check.cpp compiles pack.hpp's pack_views / pack_view_keys -- what packs the views' camera records and the
key table they share -- with g++ and prints where every view's keys landed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cr_render_views_device", "cr_render_views_host", "cr_render_aov_views_device", "cr_render_aov_views_host")


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())


def test_header_declares_the_four_calls():
    text = header()
    for name, out in zip(NAMES[:2], ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, "
                f"const CrRenderParams* params, void* {out}, CrStats* stats);") in text
    for name, out in zip(NAMES[2:], ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, "
                f"const CrRenderParams* params, int32_t layers, void* {out}, CrStats* stats);") in text


def test_abi_version_is_still_4(hiplib):
    assert "#define CR_ABI_VERSION 4" in header()
    assert A.CR_ABI_VERSION == 4
    assert hiplib.cr_abi_version() == 4


def test_python_table_mirrors_the_signatures():
    head = [C.c_void_p, C.POINTER(A.CrCameraDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(A.CrRenderParams)]
    tail = [C.c_void_p, C.POINTER(A.CrStats)]
    for name in NAMES:
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == head + ([C.c_int32] if "aov" in name else []) + tail, name
    declared = set(re.findall(r"CR_API [^;(]*?\b(cr_\w+)\(", header()))
    assert set(NAMES) <= declared and declared == set(A.SYMBOLS)


def test_renderer_has_the_four_methods():
    from crucible_amd.renderer import Renderer
    for name in ("render_views", "render_views_device", "render_aov_views", "render_aov_views_device"):
        assert callable(getattr(Renderer, name))


def test_exports_map_lets_them_out():
    text = open(os.path.join(ROOT, "crucible_amd", "csrc", "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:([^}]*?)local:", text, re.S).group(1).split(";") if p.strip()]
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name


def test_library_exports_them_and_refuses_null_arguments(hiplib):
    """Fails on a library without the feature: the symbols are missing.  A null handle is refused before anything touches a
    device, whatever the other arguments are."""
    for name in NAMES:
        fn = getattr(hiplib, name)
        assert fn.argtypes[2] is C.c_int32 and fn.argtypes[3] == C.POINTER(C.c_int32)
    frames = (C.c_int32 * 2)(0, 1)
    cams = (A.CrCameraDesc * 2)()
    p = A.CrRenderParams()
    for cams_arg, n, fr, params in ((None, 2, frames, None), (cams, 2, frames, C.byref(p)), (cams, 0, None, C.byref(p)), (None, -1, None, None)):
        assert hiplib.cr_render_views_host(None, cams_arg, n, fr, params, None, None) == A.CR_ERR_INVALID_ARG
        assert hiplib.cr_render_views_device(None, cams_arg, n, fr, params, None, None) == A.CR_ERR_INVALID_ARG
        assert hiplib.cr_render_aov_views_host(None, cams_arg, n, fr, params, A.CR_AOV_ALL, None, None) == A.CR_ERR_INVALID_ARG
        assert hiplib.cr_render_aov_views_device(None, cams_arg, n, fr, params, A.CR_AOV_ALL, None, None) == A.CR_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views_pack") / "views_pack_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                           "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "views_pack_check.cpp")])
    return exe


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("counts", [[(0, 0)], [(3, 2)], [(2, 1), (0, 0), (0, 4), (5, 0), (1, 1)], [(300, 212), (0, 0), (1, 0)]],
                         ids=["one-unkeyed", "one-keyed", "mixed", "513-keys"])
def test_key_offsets_of_concatenated_views(pack_check, real, counts):
    """View k's look_from keys begin where the keys of the views before it end, its look_at keys right behind them; an
    unkeyed view takes no room and is not animated; the table holds every key once, in call order; and each record is
    otherwise the record of the camera alone (so a view renders what a single call of its camera renders)."""
    args = [str(v) for pair in counts for v in pair]
    lines = subprocess.check_output([pack_check, real, str(len(counts))] + args, text=True).splitlines()
    total = sum(f + a for f, a in counts)
    assert lines[0] == f"total {total}"
    first = 0
    for k, (nf, na) in enumerate(counts):
        assert lines[1 + k].split() == ["view", str(k), str(first), str(nf), str(first + nf), str(na), str(int(nf + na > 0)), "1"], lines[1 + k]
        first += nf + na
    assert lines[1 + len(counts)].split() == ["keys"] + [str(i) for i in range(total)]
