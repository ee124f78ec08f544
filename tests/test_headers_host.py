"""The layering of crucible_amd/csrc's headers, checked by compiling, without a device:
- the bottom layer -- hd.hpp, records.hpp, fastdiv.hpp, residency.hpp, launch_plan.hpp -- is free of HIP: each header alone passes
  g++ with warnings as errors and no include path but csrc's own;
- every header behind pathtrace.hpp, pathtrace.hpp itself and handle.hpp are self-contained: each alone passes hipcc for gfx950;
- handle.hpp, which every host unit of the library reads, holds no kernel code of the path tracer: its preprocessed device text
  defines neither walk_round nor pathtrace_body."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crucible_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")

HIP_FREE = ["hd.hpp", "records.hpp", "fastdiv.hpp", "residency.hpp", "launch_plan.hpp"]
LAYERS = ["hd.hpp", "records.hpp", "intersect.hpp", "shade.hpp", "walk.hpp", "megakernel.hpp"]


def one_line_source(tmp_path, header, suffix):
    src = tmp_path / ("only_" + header.replace(".hpp", suffix))
    src.write_text(f'#include "{header}"\n')
    return str(src)


@pytest.mark.parametrize("header", HIP_FREE)
def test_the_bottom_layer_compiles_without_hip(tmp_path, header):
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, one_line_source(tmp_path, header, ".cpp")],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr


@needs_hipcc
@pytest.mark.parametrize("header", LAYERS + ["pathtrace.hpp", "devres.hpp", "handle.hpp"])
def test_each_header_is_self_contained_for_gfx950(tmp_path, header):
    res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, one_line_source(tmp_path, header, ".hip")],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr


@needs_hipcc
def test_handle_hpp_holds_no_kernel_code_of_the_path_tracer(tmp_path):
    def device_text(header):
        res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-E", "--offload-device-only", "-I", CSRC,
                              one_line_source(tmp_path, header, ".hip")], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        return res.stdout
    handle = device_text("handle.hpp")
    assert "struct KernelArgs" in handle                      # the records are there ...
    for definition in ("void walk_round(", "void pathtrace_body("):
        assert definition not in handle, definition           # ... the kernels' code is not
    whole = device_text("pathtrace.hpp")                      # and the search finds the two where they are
    for definition in ("void walk_round(", "void pathtrace_body("):
        assert definition in whole, definition
