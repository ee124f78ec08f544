"""The compiled form of the headline kernel without work counters (pathtrace.hpp pathtrace_kernel_quiet<RES_LDS>, what a
render that asks for no stats runs) beside the counted one (pathtrace_kernel<double, RES_LDS, false, false, false, true,
true>), from a device-only compile of tests/quiet_isa.hip -- no GPU needed:
  - the quiet kernel's screened box step has 20 vector instructions, one fewer than the counted kernel's 21: the v_mov that
    copied the step count into the per-lane node count is gone, and the step count itself stays in a scalar register
    (s_add_i32 / s_cmp / s_cselect) -- no vector instruction of the step writes an integer count;
  - the compiler's remark for the quiet kernel shows no spilled register, no scratch and 4 waves per SIMD."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_screen_fma import ISA_FLAGS, _screened_loop  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "quiet_isa.hip")
# vector instructions that could keep a per-lane count: integer adds and subtracts, and a move (of the scalar count)
COUNT_OPS = re.compile(r"^v_(mov_b32|add_u32|add_co_u32|addc_co_u32|add_nc_u32|sub_u32|sub_co_u32|subrev_u32|subrev_co_u32|sub_nc_u32|add3_u32|lshl_add_u32|mad_u32_u24)")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{kernel: (the screened loop's instructions, the resource remarks)} of the quiet and the counted headline kernel."""
    d = tmp_path_factory.mktemp("quiet_isa")
    procs = {}
    for name, flags in (("quiet", ["-DQUIET_ISA"]), ("counted", [])):
        out = d / f"{name}.s"
        procs[name] = (out, subprocess.Popen(ISA_FLAGS + flags + ["-Rpass-analysis=kernel-resource-usage", "-o", str(out), SRC],
                                             stderr=subprocess.PIPE, text=True))
    got = {}
    for name, (out, p) in procs.items():
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err
        got[name] = (_screened_loop(out.read_text()), err)
    return got


def _valu(loop):
    return [l.split()[0] for l in loop if l.startswith("v_")]


def test_quiet_step_is_20_vector_instructions_and_keeps_no_lane_count(compiled):
    loop, _ = compiled["quiet"]
    valu = _valu(loop)
    assert valu.count("v_pk_fma_f32") == 3, loop
    assert len(valu) == 20, (len(valu), loop)
    assert not [op for op in valu if COUNT_OPS.match(op)], loop
    # the step count: a scalar add, compared with the round's budget and turned into the limit by a scalar select
    ops = [l.split()[0] for l in loop]
    assert ops.count("s_add_i32") == 1 and "s_cselect_b32" in ops and any(op.startswith("s_cmp_") for op in ops), loop


def test_quiet_kernel_has_no_spill_no_scratch_and_four_waves(compiled):
    _, remarks = compiled["quiet"]
    assert "pathtrace_kernel_quiet" in remarks, remarks

    def field(name):
        m = re.findall(r"remark:\s+" + re.escape(name) + r":\s+(\d+)", remarks)
        assert len(m) == 1, (name, remarks)   # one kernel in the unit
        return int(m[0])
    assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("Occupancy [waves/SIMD]") == 4
    assert field("VGPRs") <= 128


def test_counted_step_still_has_21(compiled):
    loop, remarks = compiled["counted"]
    valu = _valu(loop)
    assert "pathtrace_kernel_quiet" not in remarks
    assert valu.count("v_pk_fma_f32") == 3, loop
    assert len(valu) == 21, (len(valu), loop)
