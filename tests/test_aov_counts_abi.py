"""cr_render_aov_counts_* at the boundary, without a GPU: the header declares the six entry points, the ctypes table mirrors
their signatures, the export map lets them through and the built library has them in its dynamic table, the documents name
them, the ABI version is unchanged, a null handle is refused through each, and the CLI's --adaptive-aov asks for
--adaptive."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, PAR, ST = C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.POINTER(A.CrStats)
# name -> the arguments between `params` and `stats`, in the header's words and in ctypes
FORMS = {
    "cr_render_aov_counts_device": ("int32_t layers, const int32_t* d_counts, void* d_out", [C.c_int32, C.c_void_p, C.c_void_p]),
    "cr_render_aov_counts_host": ("int32_t layers, const int32_t* h_counts, void* h_out", [C.c_int32, C.c_void_p, C.c_void_p]),
    "cr_render_aov_counts_frames_device": ("int32_t layers, const int32_t* frames, int32_t n_frames, const int32_t* d_counts, void* d_out",
                                           [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p]),
    "cr_render_aov_counts_frames_host": ("int32_t layers, const int32_t* frames, int32_t n_frames, const int32_t* h_counts, void* h_out",
                                         [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p]),
    "cr_render_aov_counts_region_device": ("int32_t layers, const CrRegion* region, const int32_t* d_counts, void* d_out",
                                           [C.c_int32, C.POINTER(A.CrRegion), C.c_void_p, C.c_void_p]),
    "cr_render_aov_counts_region_host": ("int32_t layers, const CrRegion* region, const int32_t* h_counts, void* h_out",
                                         [C.c_int32, C.POINTER(A.CrRegion), C.c_void_p, C.c_void_p]),
}


def text_of(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_header_declares_the_six_entry_points():
    text = text_of("include", "crucible_hip.h")
    for name, (middle, _) in FORMS.items():
        assert f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, {middle}, CrStats* stats);" in text, name
    assert "#define CR_ABI_VERSION 4" in text
    assert "n_p = min(max(counts[p], 0), params->samples)" in text   # the definition, in full


def test_python_table_mirrors_the_signatures():
    for name, (_, middle) in FORMS.items():
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == [C.c_void_p, CAM, PAR] + middle + [ST], name
    assert A.CR_ABI_VERSION == 4


def test_export_map_and_dynamic_table(hiplib):
    patterns = re.search(r"global:([^}]*?)local:", open(os.path.join(ROOT, "crucible_amd", "csrc", "exports.map")).read(), re.S).group(1)
    patterns = [p.strip() for p in patterns.split(";") if p.strip()]
    table = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "crucible_amd", "libcrucible_hip.so")], capture_output=True, text=True,
                           check=True).stdout
    exported = {line.split()[-1] for line in table.splitlines() if line.split()}
    for name in FORMS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in exported, name
    assert hiplib.cr_abi_version() == 4


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "DESIGN.md"])
def test_documents_name_the_entry_points(doc):
    text = text_of(doc)
    for name in FORMS:
        assert name in text, (doc, name)


def test_a_null_handle_is_refused(hiplib):
    cd, p = A.CrCameraDesc(), A.CrRenderParams()
    plane, out = (C.c_int32 * 4)(), (C.c_double * 64)()
    fr, reg = (C.c_int32 * 1)(0), A.CrRegion(0, 0, 1, 1)
    for name in FORMS:
        middle = [15] + ([fr, 1] if "frames" in name else []) + ([C.byref(reg)] if "region" in name else []) + [C.cast(plane, C.c_void_p), C.cast(out, C.c_void_p)]
        assert getattr(hiplib, name)(None, C.byref(cd), C.byref(p), *middle, None) == A.CR_ERR_INVALID_ARG, name


def test_mirrors_exist():
    from crucible_amd.renderer import Renderer
    from crucible_amd.scene import Scene
    for name in ("render_aov_counts", "render_aov_counts_frames", "render_aov_counts_region"):
        assert callable(getattr(Renderer, name)) and callable(getattr(Renderer, name + "_device")), name
    import inspect
    assert inspect.signature(Scene.set_adaptive).parameters["guide_at_counts"].default is False


def test_cli_adaptive_aov_needs_adaptive(hiplib, tmp_path):
    exe = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    res = subprocess.run([exe, "--file", str(tmp_path / "x"), "--width", "32", "--samples", "8", "--adaptive-aov", "albedo,depth"], capture_output=True,
                         timeout=120)
    assert res.returncode == 2 and b"--adaptive-aov" in res.stderr, res.stderr
    assert not os.listdir(tmp_path)
    # and next to --adaptive an unknown layer is the option's own refusal
    res = subprocess.run([exe, "--file", str(tmp_path / "x"), "--width", "32", "--samples", "8", "--adaptive", "0.1,4,2", "--adaptive-aov", "beauty"],
                         capture_output=True, timeout=120)
    assert res.returncode == 2 and b"--adaptive-aov takes a list" in res.stderr, res.stderr
