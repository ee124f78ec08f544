"""cr_render_adaptive_* at the boundary, without a GPU: the header declares the calls, both structs and the rule, the ctypes
table mirrors the signatures, the built library exports them and refuses a null handle (a handle needs a device: the other
refusals are in tests/test_gpu_adaptive.py), the layouts of CrAdaptiveParams and CrAdaptiveStats agree between the header
and ctypes, and the ABI version did not move."""
import ctypes as C
import os
import re
import subprocess

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cr_render_adaptive_device", "cr_render_adaptive_host")


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())


def test_header_declares_the_calls_and_the_rule():
    text = header()
    for name, out, counts in zip(CALLS, ("d_out_rgb", "h_out_rgb"), ("d_counts", "h_counts")):
        assert (f"CR_API int32_t {name}(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, "
                f"const CrAdaptiveParams* adaptive, void* {out}, int32_t* {counts}, CrAdaptiveStats* stats);") in text
    assert "typedef struct CrAdaptiveParams {" in text and "} CrAdaptiveParams;" in text
    assert "typedef struct CrAdaptiveStats {" in text and "} CrAdaptiveStats;" in text
    # the rule, in its exactness
    for phrase in ("d(x, c) = |mag(E[x,c]) - mag(O[x,c])| >> 12", "T_b = (uint64) min(floor(tolerance * (2^(S-12) * qP * 3 N_b)), 2^63)",
                   "the block stops iff D_b <= T_b", "anchored at pixel (0, 0)", "BIT FOR BIT", "min_samples == params->samples is exactly the plain relaxed render"):
        assert phrase in text, phrase
    assert "#define CR_ABI_VERSION 4" in text and A.CR_ABI_VERSION == 4


def test_python_table_mirrors_the_signatures():
    want = (C.c_int32, [C.c_void_p, C.POINTER(A.CrCameraDesc), C.POINTER(A.CrRenderParams), C.POINTER(A.CrAdaptiveParams), C.c_void_p,
                        C.c_void_p, C.POINTER(A.CrAdaptiveStats)])
    for name in CALLS:
        assert A.SYMBOLS[name] == want, name


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"CrAdaptiveParams": A.CrAdaptiveParams, "CrAdaptiveStats": A.CrAdaptiveStats}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "crucible_hip.h"\nint main(){\n'
    for sname, cls in structs.items():
        src += f'printf("{sname} %zu\\n", sizeof({sname}));\n'
        for fname, _ in cls._fields_:
            src += f'printf("{sname}.{fname} %zu\\n", offsetof({sname}, {fname}));\n'
    src += "return 0;}\n"
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines() if line)
    assert int(got["CrAdaptiveParams"]) == C.sizeof(A.CrAdaptiveParams) == 24
    assert int(got["CrAdaptiveStats"]) == C.sizeof(A.CrAdaptiveStats) == C.sizeof(A.CrStats) + 24
    assert [f for f, _ in A.CrAdaptiveParams._fields_] == ["min_samples", "pass_samples", "block_log2", "_reserved", "tolerance"]
    assert [f for f, _ in A.CrAdaptiveStats._fields_] == ["render", "judge_ms", "passes", "blocks", "blocks_stopped", "_pad"]
    for sname, cls in structs.items():
        for fname, _ in cls._fields_:
            assert int(got[f"{sname}.{fname}"]) == getattr(cls, fname).offset, (sname, fname)


def test_library_exports_them_and_refuses_a_null_handle(hiplib):
    for name in CALLS:
        assert hasattr(hiplib, name), name
    cd, p, ap = A.CrCameraDesc(), A.CrRenderParams(), A.CrAdaptiveParams(4, 2, 4, 0, 0.01)
    out = (C.c_double * 8)()
    counts = (C.c_int32 * 8)()
    # a null handle is refused before anything touches a device, whatever else is null
    for cam, params, adaptive in ((cd, p, ap), (None, p, ap), (cd, None, ap), (cd, p, None), (None, None, None)):
        args = [C.byref(x) if x is not None else None for x in (cam, params, adaptive)]
        for name in CALLS:
            assert getattr(hiplib, name)(None, *args, out, counts, None) == A.CR_ERR_INVALID_ARG
            assert getattr(hiplib, name)(None, *args, out, None, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_abi_version() == 4
