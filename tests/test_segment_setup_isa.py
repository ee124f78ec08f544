"""The headline kernel begins a segment without an IEEE f64 division (pathtrace.hpp walk_begin_screened): compiled alone
(tests/screen_isa.hip, as test_gpu_screen_fma.py compiles it), the code from the kernel's entry to the screened box loop holds no
v_div_scale_f64 other than camera_ray's and the launch set-up's.  Which those are is not read off the block layout: the same kernel
is compiled with -DCR_LAZY_INV=0 (walk_begin and its three divisions, everything else the same source), and the stretch must hold
exactly three divisions fewer -- six v_div_scale_f64, three v_div_fmas_f64, three v_div_fixup_f64 -- while the divisions of
1 / direction stand behind the box loop's first step, in the band branch and in front of the compare/select loop.  A layout that
moved camera_ray across the box loop in one build only would fail this test, never pass it.  CPU only: it reads the assembly."""
import re
import subprocess

import pytest

from test_gpu_screen_fma import ISA_FLAGS, ISA_KERNELS, ISA_SRC


def _stretch(tmp_path, tag, extra):
    """(mnemonics from the kernel's entry to its first v_pk_fma_f32, mnemonics after it)."""
    out = tmp_path / f"{tag}.s"
    subprocess.run(ISA_FLAGS + extra + [f"-DSCREEN_ISA_KERNEL={ISA_KERNELS['headline'][0]}", "-o", str(out), ISA_SRC], check=True, timeout=600)
    lines = out.read_text().splitlines()
    entry = next(i for i, l in enumerate(lines) if re.match(r"^_ZN2cr16pathtrace_kernel\w*:", l))
    end = next(i for i in range(entry, len(lines)) if "s_endpgm" in lines[i])
    first_fma = next(i for i in range(entry, end) if "v_pk_fma_f32" in lines[i])
    ops = lambda a, b: [l.split()[0] for l in lines[a:b] if re.match(r"^\s+[sv]_", l)]   # noqa: E731
    return ops(entry, first_fma), ops(first_fma, end)


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("segment_setup_isa")
    return _stretch(d, "lazy", []), _stretch(d, "divides", ["-DCR_LAZY_INV=0"])


def test_three_divisions_fewer_between_entry_and_box_loop(builds):
    (lazy, lazy_after), (div, _) = builds
    assert len(lazy) > 500 and len(div) > 500, (len(lazy), len(div))   # the stretch holds regeneration and the segment's set-up
    for op, per_division in (("v_div_scale_f64", 2), ("v_div_fmas_f64", 1), ("v_div_fixup_f64", 1)):
        assert div.count(op) - lazy.count(op) == 3 * per_division, (op, div.count(op), lazy.count(op))
    # the reciprocals are still made: three bare v_rcp_f64 for the three inside the divisions
    assert lazy.count("v_rcp_f64_e32") == div.count("v_rcp_f64_e32"), (lazy.count("v_rcp_f64_e32"), div.count("v_rcp_f64_e32"))
    # ... and 1.0 / rd is divided where Aabb::hit's f64 form runs: behind the box loop's first step, twice three divisions
    assert lazy_after.count("v_div_scale_f64") >= 12, lazy_after.count("v_div_scale_f64")


def test_the_switch_changes_nothing_but_the_set_up(builds):
    """The two builds differ in the set-up alone: the box loop of either is the pinned one (test_gpu_screen_fma.py pins the default)."""
    (_, lazy_after), (_, div_after) = builds
    assert lazy_after.count("v_pk_fma_f32") == div_after.count("v_pk_fma_f32") == 3
