"""cr_render_frames_device / cr_render_frames_host at the boundary, without a GPU: the header declares them, the ctypes
table mirrors their signatures, the built library exports them, and the CLI checks its --frames-per-launch value."""
import ctypes as C
import os
import re
import subprocess

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cr_render_frames_device", "cr_render_frames_host")


def test_header_declares_the_batch_calls():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())
    for name, out in zip(NAMES, ("d_out", "h_out")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, "
                f"const int32_t* frames, int32_t n_frames, void* {out}, CrStats* stats);") in text
    assert "#define CR_ABI_VERSION 4" in text


def test_python_table_mirrors_the_signatures():
    want = [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.POINTER(C.c_int32), C.c_int32,
            C.c_void_p, C.POINTER(A.CrStats)]
    for name in NAMES:
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == want, name


def test_library_exports_the_batch_calls(hiplib):
    for name in NAMES:
        fn = getattr(hiplib, name)
        assert fn.argtypes[3] == C.POINTER(C.c_int32)
    # a null handle is refused before anything touches a device
    assert hiplib.cr_render_frames_host(None, None, None, None, 1, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_render_frames_device(None, None, None, None, 1, None, None) == A.CR_ERR_INVALID_ARG


def test_cli_rejects_a_non_positive_frames_per_launch(hiplib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    cli = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")
    r = subprocess.run([cli, "--file", "/nonexistent/x", "--world", "1", "--movie", "--seconds", "1", "--rate", "1",
                        "--frames-per-launch", "0"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--frames-per-launch" in r.stderr
