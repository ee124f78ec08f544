"""Every resource a handle holds is owned by a type, and the types give it back: checked by running them.

The device buffers, events, pinned blocks and the stream of CrHandle, DevScene, SahDeviceWork and CrGroup are DevBuf, DevEvent,
PinnedBuf, DevStream and CamSlot members (crucible_amd/csrc/devres.hpp), whose destructors release them.  This compiles
tests/handle_lifetime_check.cpp with g++ and the address and undefined-behaviour sanitizers against tests/hip_stub, a stand-in
for the HIP runtime that counts what is live and logs every call, and runs it: each type's ensure / create / release / move /
borrow, CamSlot::acquire with each of its three allocations failing, and a whole CrHandle whose every owning member -- found
here by its declared type in handle.hpp, not by a list -- is filled and which is then deleted.  What no program can show, that
no resource sits in a member no type owns, the declarations and a search of the sources show."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crucible_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

# raw pointer members that own nothing, and why
BORROWED = {"wf_ring_dev": "the device address of wf_ring_host's block (hipHostGetDevicePointer): freed with it"}

OWNING = r"DevBuf|DevEvent|PinnedBuf|DevStream|CamSlot"
TOUCH = {"DevBuf": "ensure_buf", "DevEvent": "create_event", "PinnedBuf": "ensure_pinned", "DevStream": "create_stream", "CamSlot": "acquire_slot"}


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def braces(text, start):
    """The text between the brace at or after `start` and its partner."""
    k = text.index("{", start)
    depth, i = 0, k
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[k + 1:i]
        i += 1


def struct_body(text, name):
    m = re.search(r"\bstruct\s+" + name + r"\s*\{", text)
    assert m, name
    return braces(text, m.start())


def without_functions(body):
    """A struct's body without the bodies of its member functions (their locals are not members)."""
    out, depth = [], 0
    for ch in body:
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            out.append(ch)
    return "".join(out)


def members(body, type_pattern):
    """Names declared with a type matching `type_pattern` at the top level of a struct body: `T a, b[2], c = nullptr;`."""
    names = []
    for stmt in without_functions(body).split(";"):
        m = re.match(r"\s*(?:static\s+|constexpr\s+)*(" + type_pattern + r")\s+(.*)$", stmt.strip(), flags=re.S)
        if not m or "(" in m.group(2).split("=")[0]:
            continue
        for decl in re.split(r",(?![^\[]*\])", m.group(2)):
            name = re.match(r"\s*\**\s*([A-Za-z_]\w*)", decl.split("=")[0])
            if name:
                names.append(name.group(1))
    return names


def pointer_members(body):
    names = []
    for stmt in without_functions(body).split(";"):
        m = re.match(r"\s*(?:const\s+)?(void|char|u?int\d+_t|float|double)\s*\*\s*(.*)$", stmt.strip(), flags=re.S)
        if not m or "(" in m.group(2).split("=")[0]:
            continue
        for decl in m.group(2).split(","):
            name = re.match(r"\s*\**\s*([A-Za-z_]\w*)", decl.split("=")[0])
            if name:
                names.append(name.group(1))
    return names


HANDLE = strip_comments(read("handle.hpp"))
GROUP = strip_comments(read("group.hpp"))
STRUCTS = {"CrHandle": struct_body(HANDLE, "CrHandle"), "DevScene": struct_body(HANDLE, "DevScene"),
           "SahDeviceWork": struct_body(HANDLE, "SahDeviceWork"), "CrGroup": struct_body(GROUP, "CrGroup")}


def touches(body, prefix):
    """One C++ statement per owning member of `body`, by its declared type."""
    return [f"    each({prefix}{name}, {TOUCH[kind]});" for kind in TOUCH for name in members(body, kind)]


def touch_source():
    """touch_handle: every owning member of CrHandle, those of its four scenes and of its SAH working set included."""
    lines = ["static void touch_handle(CrHandle& h) {"] + touches(STRUCTS["CrHandle"], "h.")
    scenes = members(STRUCTS["CrHandle"], r"DevScene<\w+>")
    for scene in scenes:
        lines += touches(STRUCTS["DevScene"], f"h.{scene}.")
    for work in members(STRUCTS["CrHandle"], "SahDeviceWork"):
        lines += touches(STRUCTS["SahDeviceWork"], f"h.{work}.")
    lines += ["}", "static void touch_sah_work(SahDeviceWork& w) {"] + touches(STRUCTS["SahDeviceWork"], "w.") + ["}"]
    return "\n".join(lines) + "\n", scenes


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    """handle_lifetime_check.cpp over the generated handle_touch.inc: compiled once, run once as a child process."""
    tmp = tmp_path_factory.mktemp("handle_lifetime")
    source, _ = touch_source()
    (tmp / "handle_touch.inc").write_text(source)
    exe = str(tmp / "handle_lifetime_check")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(TESTS, "hip_stub"),
                          "-I", CSRC, "-I", str(tmp), os.path.join(TESTS, "handle_lifetime_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_the_parser_sees_the_members():
    h = members(STRUCTS["CrHandle"], r"DevBuf")
    for name in ("fx_acc", "aov_acc", "aov_flags", "aov_counts", "ad_acc", "ad_lists", "ad_block_n", "ad_ctrl", "ad_counts", "out_buf", "sample_buf", "sg_acc",
                 "att_stack", "times_dev", "update_stage", "images", "texels", "work_counter", "counters", "wf_job", "wf_acc"):
        assert name in h, name
    assert len(h) >= 29
    assert set(members(STRUCTS["CrHandle"], r"DevEvent")) == {"ev0", "ev1", "ad_ev0", "ad_ev1", "times_ev", "wf_ev"}
    assert set(members(STRUCTS["CrHandle"], r"PinnedBuf")) == {"times_host", "wf_ring_host"}
    assert members(STRUCTS["CrHandle"], r"DevStream") == ["stream"] and members(STRUCTS["CrHandle"], r"CamSlot") == ["cam"]
    assert set(pointer_members(STRUCTS["CrHandle"])) == {"wf_ring_dev"}
    assert set(members(STRUCTS["CrHandle"], r"DevScene<\w+>")) == {"s32", "s64", "f32", "f64"} and members(STRUCTS["CrHandle"], r"SahDeviceWork") == ["sah_work"]
    d = members(STRUCTS["DevScene"], r"DevBuf")
    for name in ("entries", "prims", "mats", "texs", "keys", "leaf_runs", "entries_refit", "screen", "screen_refit", "screen_overflow", "desc_pos", "frame_map"):
        assert name in d, name
    assert set(members(STRUCTS["SahDeviceWork"], r"DevBuf")) == {"box", "order", "seg", "pbins", "flags", "scan", "tmp", "slots", "nodes", "small", "ctr"}
    assert set(members(STRUCTS["CrGroup"], r"std::vector<DevBuf>")) == {"partial", "flags", "status"} and set(members(STRUCTS["CrGroup"], r"DevEvent")) == {"ev0", "ev1"}
    # and the generated program touches each of them: a line per member, the scenes' members once per scene
    source, scenes = touch_source()
    assert len(scenes) == 4
    for line in ("each(h.stream, create_stream);", "each(h.cam, acquire_slot);", "each(h.wf_ev, create_event);", "each(h.times_host, ensure_pinned);",
                 "each(h.aov_flags, ensure_buf);", "each(h.f64.frame_map, ensure_buf);", "each(h.s32.mats, ensure_buf);", "each(h.sah_work.slots, ensure_buf);"):
        assert source.count(line) == 1, line
    assert source.count("each(h.") == len(h) + 6 + 2 + 1 + 1 + 4 * len(d) + 11


def test_the_stream_is_declared_before_every_other_resource():
    """Members are destroyed in reverse order of declaration: the stream goes last, as the program's log shows."""
    body = without_functions(STRUCTS["CrHandle"])
    first = min(m.start() for m in re.finditer(r"\b(?:" + OWNING + r"|DevScene<\w+>|SahDeviceWork)\s+\w", body))
    assert re.match(r"DevStream\s+stream\b", body[first:])


def test_the_check_program_is_clean(check_run):
    """Under -fsanitize=address,undefined: no finding, no leak, every CHECK held."""
    assert check_run.returncode == 0, check_run.stdout + check_run.stderr
    assert "runtime error" not in check_run.stderr and "Sanitizer" not in check_run.stderr, check_run.stderr


@pytest.mark.parametrize("section", ["DevBuf", "DevEvent PinnedBuf DevStream", "CamSlot", "CrHandle"])
def test_the_check_program_ran(check_run, section):
    """DevBuf etc.: each owning type; CamSlot: acquire with its 1st, 2nd, 3rd allocation failing; CrHandle: the whole handle."""
    assert ("ok " + section) in check_run.stdout.splitlines(), check_run.stdout + check_run.stderr


@pytest.mark.parametrize("struct", sorted(STRUCTS))
def test_no_member_is_a_raw_resource(struct):
    body = STRUCTS[struct]
    assert members(body, r"hipEvent_t|hipStream_t") == []
    assert [name for name in pointer_members(body) if name not in BORROWED] == []


def test_only_devres_frees_and_allocates():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hpp", ".hip", ".h", ".cpp")):
            continue
        text = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', strip_comments(read(name)))   # calls, not the error texts that name one
        for call in (r"\bhipFree\b", r"\bhipHostFree\b", r"\bhipEventDestroy\b", r"\bhipStreamDestroy\b", r"\bhipMalloc\(", r"\bhipHostMalloc\(", r"\bhipEventCreate"):
            if re.search(call, text):
                found.setdefault(name, []).append(call)
    assert sorted(found) == ["devres.hpp"], found
    assert len(found["devres.hpp"]) == 7
