"""The compiled form of the headline kernel without work counters (pathtrace_kernel_quiet<RES_LDS>) around its screened box
step, from a device-only compile of tests/quiet_isa.hip -- no GPU needed:
  - no more VGPRs than the figure profiles/r03_kernel_resources.json holds for the kernel, no spill, no scratch, 4 waves;
  - the position is carried across rounds as an LDS address (walk.hpp WalkOffset): the rounds loop -- the loop around the
    screened box loop -- turns no index into an address or back (v_lshl_add_u32 .., 5, .. / v_lshrrev_b32 .., 5, ..) outside
    the two places that read an index, the band branch's f64 fetch and the compare/select loop, which both load f64 records
    from global memory: exactly three conversions, each at its place;
  - the rounds run at a wave priority of their own: one s_setprio 1 and one s_setprio 0, both outside the rounds loop (in
    front of it and behind it, under the scalar branch on the ballot of walking lanes).
The walk's knobs are still read through the kernarg pointer inside the rounds loop: pinning them in scalar registers
measured slower, so nothing is asserted about s_load_dword."""
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_screen_fma import ISA_FLAGS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "quiet_isa.hip")
KERNEL = "cr::pathtrace_kernel_quiet<1>"
BLOCK = re.compile(r"^(?:\.L(BB\w+):|; %bb\.(\d+):)")
TO_ADDRESS = re.compile(r"v_lshl_add_u32 .*, 5, ")
TO_INDEX = re.compile(r"v_lshrrev_b32\S* \S+ 5, ")


def rounds_loop(asm):
    """The basic blocks of the rounds loop, in layout order: the loop that is the parent of the screened box loop (the
    innermost loop with a v_pk_fma_f32), its child loops' blocks included.  [(name, header of the block's loop, instructions)];
    also the names of the screened loop and of the other child loops."""
    blocks, cur = [], None
    for line in asm.splitlines():
        m = BLOCK.match(line)
        if m:
            cur = {"name": m.group(1) or "bb." + m.group(2), "loop": None, "parents": [], "ins": []}
            blocks.append(cur)
        if cur is None:
            continue
        comment = line.split(";", 1)[1] if ";" in line else ""
        mm = re.search(r"in Loop: Header=(BB\w+)", comment)
        if mm:
            cur["loop"] = mm.group(1)
        if re.search(r"This (Inner )?Loop Header", comment):
            cur["loop"] = cur["name"]
        mm = re.search(r"Parent Loop (BB\w+)", comment)
        if mm:
            cur["parents"].append(mm.group(1))
        text = line.split(";")[0].strip()
        if text and not text.startswith((".", "#")) and not m:
            cur["ins"].append(text)
    parents = {b["name"]: b["parents"] for b in blocks if b["loop"] == b["name"]}
    inner = next(b["loop"] for b in blocks if any(i.startswith("v_pk_fma_f32") for i in b["ins"]))
    rounds = parents[inner][-1]
    body = [b for b in blocks if b["loop"] is not None and (b["loop"] == rounds or rounds in parents.get(b["loop"], []))]
    others = sorted({b["loop"] for b in body if b["loop"] not in (rounds, inner)})
    return [(b["name"], b["loop"], b["ins"]) for b in body], inner, others, [i for b in blocks for i in b["ins"]]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = tmp_path_factory.mktemp("walk_offset_isa") / "quiet.s"
    p = subprocess.run(ISA_FLAGS + ["-DQUIET_ISA", "-Rpass-analysis=kernel-resource-usage", "-o", str(out), SRC], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return out.read_text(), p.stderr


def test_resources_are_no_worse_than_the_committed_figures(compiled):
    _, remarks = compiled
    assert "pathtrace_kernel_quiet" in remarks, remarks

    def field(name):
        m = re.findall(r"remark:\s+" + re.escape(name) + r":\s+(\d+)", remarks)
        assert len(m) == 1, (name, remarks)
        return int(m[0])
    base = json.load(open(os.path.join(ROOT, "profiles", "r03_kernel_resources.json")))["kernels"][KERNEL]
    print(f"\n[walk offset isa] VGPRs {field('VGPRs')} (committed {base['vgprs']}), SGPRs {field('TotalSGPRs')}")
    assert field("VGPRs") <= base["vgprs"] <= 128
    assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("Occupancy [waves/SIMD]") == 4


def test_rounds_loop_converts_the_position_only_where_an_index_is_read(compiled):
    """Exactly three conversions are left in the rounds loop (profiles/experiments/round_overhead_ab.txt):
      - one address -> index inside the box loop, in the band branch's block, the one that loads the f64 record;
      - one address -> index between the box loop's last block and the compare/select loop's first, and one index -> address
        behind that loop's last block: the pair around the loop that walks by index.
    None stands in front of the box loop or at its tail, where the parent turned the index into an address and back."""
    body, inner, others, _ = rounds_loop(compiled[0])
    assert len(body) > 20, len(body)   # the rounds loop: box loop, compare/select loop, leaf phase
    loads = lambda ins: any(i.startswith("global_load") for i in ins)  # noqa: E731
    select = [loop for loop in others if any(loads(ins) for _, l, ins in body if l == loop)]
    assert len(select) == 1, (others, select)   # the compare/select loop: the other child loop that reads f64 records
    box = [k for k, (_, l, _) in enumerate(body) if l == inner]
    sel = [k for k, (_, l, _) in enumerate(body) if l == select[0]]
    assert max(box) < min(sel)
    found = [(k, "index" if TO_INDEX.match(i) else "address", loads(ins)) for k, (_, _, ins) in enumerate(body) for i in ins
             if TO_ADDRESS.match(i) or TO_INDEX.match(i)]
    assert len(found) == 3, found
    (k0, what0, band), (k1, what1, _), (k2, what2, _) = found
    assert what0 == "index" and k0 in box and band, found
    assert what1 == "index" and max(box) < k1 < min(sel) and body[k1][1] not in (inner, select[0]), found
    assert what2 == "address" and k2 > max(sel) and body[k2][1] not in (inner, select[0]), found


def test_priority_is_raised_in_front_of_the_rounds_loop_and_dropped_behind_it(compiled):
    body, _, _, every = rounds_loop(compiled[0])
    prio = [i for i in every if i.startswith("s_setprio")]
    assert sorted(prio) == ["s_setprio 0", "s_setprio 1"], prio
    assert not [i for _, _, ins in body for i in ins if i.startswith("s_setprio")]
