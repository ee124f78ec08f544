"""CR_REFIT_REBUILD at the ABI, without a GPU: the header's constants and the mirrors' agree, the two new entry points
are declared, exported and bound, both mirrors map "rebuild" to 2, and the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from crucible_amd import _abi as A
from crucible_amd.scene import Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crucible_hip.h")


def test_header_constants_equal_the_mirror():
    text = open(HEADER).read()
    m = re.search(r"enum \{ CR_REFIT_OFF = (\d+), CR_REFIT_BOXES = (\d+), CR_REFIT_REBUILD = (\d+) \};", text)
    assert m, "the CR_REFIT_* enum is missing from the header"
    assert tuple(int(x) for x in m.groups()) == (A.CR_REFIT_OFF, A.CR_REFIT_BOXES, A.CR_REFIT_REBUILD) == (0, 1, 2)


def test_symbols_are_declared_exported_and_bound(hiplib):
    text = open(HEADER).read()
    for name in ("cr_export_render_bvh", "cr_frame_build_info"):
        assert re.search(r"CR_API int32_t " + name + r"\(", text), name
        assert name in A.SYMBOLS
        assert getattr(hiplib, name).argtypes == A.SYMBOLS[name][1]
    assert A.SYMBOLS["cr_export_render_bvh"] == A.SYMBOLS["cr_export_bvh"]
    assert A.SYMBOLS["cr_frame_build_info"] == A.SYMBOLS["cr_build_info"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "crucible_amd", "libcrucible_hip.so")], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"cr_export_render_bvh", "cr_frame_build_info"} <= exported
    assert not any("build_frame_scene" in s or "select_tree" in s for s in exported)     # the version script keeps the table to cr_*


def test_python_mirror_maps_rebuild_to_2():
    assert [A.refit_code(v) for v in (False, True, "rebuild", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    with pytest.raises(ValueError):
        A.refit_code("always")
    cam = Scene.new_image(16.0 / 9.0, 16, 24, 180.0, 1).scene_cam
    assert cam.params(1, A.CR_REAL_F32).refit_boxes == 0
    cam.refit_boxes = True
    assert cam.params(1, A.CR_REAL_F32).refit_boxes == 1
    cam.refit_boxes = "rebuild"
    assert cam.params(1, A.CR_REAL_F32).refit_boxes == A.CR_REFIT_REBUILD
    assert C.sizeof(A.CrRenderParams) == 64


CPP = r'''
#include "crucible.hpp"
#include <cstdio>
using namespace crucible;
int main() {
    Scene s = Scene::new_image(16.0 / 9.0, 16, 24, 180.0, 1);
    printf("%d", s.render_params(0).refit_boxes);
    bool on = true;
    s.refit_boxes = on;            printf(" %d", s.render_params(0).refit_boxes);
    s.refit_boxes = "rebuild";     printf(" %d", s.render_params(0).refit_boxes);
    s.refit_boxes = std::string("rebuild"); printf(" %d", s.render_params(0).refit_boxes);
    s.refit_boxes = false;         printf(" %d", s.render_params(0).refit_boxes);
    s.refit_boxes = CR_REFIT_REBUILD; printf(" %d", s.render_params(0).refit_boxes);
    if (s.refit_boxes) printf(" on");
    try { s.refit_boxes = "always"; } catch (const std::invalid_argument&) { printf(" refused"); }
    printf(" %zu\n", sizeof(CrRenderParams));
    return 0;
}
'''


def test_cpp_mirror_maps_rebuild_to_2(hiplib, tmp_path):
    src, exe = str(tmp_path / "refit_mode.cpp"), str(tmp_path / "refit_mode")
    open(src, "w").write(CPP)
    lib_dir = os.path.join(ROOT, "crucible_amd")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-I", os.path.join(ROOT, "crucible_amd", "host"), "-o", exe, src, "-L", lib_dir,
                           "-lcrucible_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    assert subprocess.check_output([exe], text=True).split() == ["0", "1", "2", "2", "0", "2", "on", "refused", "64"]


def test_argument_errors_without_a_device(hiplib):
    info = A.CrBuildInfo()
    n = C.c_int32()
    assert hiplib.cr_frame_build_info(None, A.CR_REAL_F32, C.byref(info)) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_frame_build_info(None, A.CR_REAL_F32, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_export_render_bvh(None, A.CR_REAL_F32, None, None, None, 0, C.byref(n)) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_export_render_bvh(None, A.CR_REAL_F64, None, None, None, 0, None) == A.CR_ERR_INVALID_ARG
