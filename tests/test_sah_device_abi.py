"""CR_BVH_BUILD_DEVICE and cr_build_info in the header and in the ctypes mirror."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crucible_hip.h")


def test_header_declares_the_flag_the_struct_and_the_function():
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*CR_BVH_BUILD_DEVICE\s*=\s*(0x[0-9a-fA-F]+|\d+)\s*\}", text)
    assert m and int(m.group(1), 0) == A.CR_BVH_BUILD_DEVICE == 0x100
    assert re.search(r"CR_API\s+int32_t\s+cr_build_info\s*\(\s*CrHandle\s*\*\s*\w*\s*,\s*int32_t\s+real_type\s*,\s*CrBuildInfo\s*\*\s*\w*\s*\)", text)
    assert re.search(r"typedef\s+struct\s+CrBuildInfo\s*\{", text)
    assert A.CR_BVH_BUILD_DEVICE & 0xFF == 0 and A.CR_BVH_LBVH < 0x100      # the low byte keeps the mode
    assert A.CR_ABI_VERSION == 4


def test_mirror_names_the_function():
    res, args = A.SYMBOLS["cr_build_info"]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_int32, C.POINTER(A.CrBuildInfo)]


def test_build_info_layout_matches_header():
    s = "CrBuildInfo"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "crucible_hip.h"\nint main(){\n'
    src += f'printf("{s} %zu\\n", sizeof({s}));\n'
    for fname, _ in A.CrBuildInfo._fields_:
        src += f'printf("{s}.{fname} %zu\\n", offsetof({s}, {fname}));\n'
    src += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    assert int(got[s]) == C.sizeof(A.CrBuildInfo) == 48
    names = [f for f, _ in A.CrBuildInfo._fields_]
    assert names == ["bvh_mode", "built_on_device", "n_wrappers", "device_rounds", "large_nodes", "small_subtrees",
                     "small_threshold", "_pad", "tree_ms", "total_ms"]
    for fname in names:
        assert int(got[f"{s}.{fname}"]) == getattr(A.CrBuildInfo, fname).offset, fname
