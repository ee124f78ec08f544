"""Every resource a handle declares is given back by name.

DevBuf has no destructor: cr_destroy, DevScene::release, SahDeviceWork::release and group_free are lists a person keeps.
This reads the declarations in crucible_amd/csrc/handle.hpp and group.hpp -- every DevBuf, every hipEvent_t and every pinned
host pointer of CrHandle, DevScene, SahDeviceWork and CrGroup -- and asserts that each name is released in the body that
owns it.  A member added without its release fails here, on the CPU; tests/test_gpu_handle_memory.py can only see a leak of
an allocation granule or more per handle."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crucible_amd", "csrc")

# raw pointer members that own nothing, and why
BORROWED = {"wf_ring_dev": "the device address of wf_ring_host (hipHostGetDevicePointer)",
            "p": "DevBuf's own", "raw": "DevBuf's own"}


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


def function_body(text, signature):
    m = re.search(signature, text)
    assert m, signature
    return braces(text, m.end() - 1)


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


def released(body, name, how):
    """`name` handed to `how` in `body`: name.release(), &name (a list of buffers that is released in a loop),
    hipEventDestroy(.. name ..), hipHostFree(.. name ..)."""
    n = re.escape(name)
    if how == "release":
        return bool(re.search(r"(?:->|\b)" + n + r"(?:\[\w+\])?\s*\.\s*release\s*\(", body) or re.search(r"&\s*" + n + r"\b", body))
    return bool(re.search(how + r"\s*\(\s*(?:\(void\*\)\s*)?(?:\w+->)?" + n + r"\b", body))


HANDLE = strip_comments(read("handle.hpp"))
API = strip_comments(read("api.hip"))
GROUP = strip_comments(read("group.hpp")) + strip_comments(read("group.hip"))


def owners():
    """(struct, its body, the body that releases its members)"""
    return [("CrHandle", struct_body(HANDLE, "CrHandle"), function_body(API, r"void\s+cr_destroy\s*\([^)]*\)\s*\{")),
            ("DevScene", struct_body(HANDLE, "DevScene"), function_body(struct_body(HANDLE, "DevScene"), r"void\s+release\s*\(\s*\)\s*\{")),
            ("SahDeviceWork", struct_body(HANDLE, "SahDeviceWork"), function_body(struct_body(HANDLE, "SahDeviceWork"), r"void\s+release\s*\(\s*\)\s*\{")),
            ("CrGroup", struct_body(GROUP, "CrGroup"), function_body(GROUP, r"void\s+group_free\s*\([^)]*\)\s*\{"))]


def missing():
    out = []
    for struct, body, free in owners():
        for name in members(body, r"DevBuf|std::vector<DevBuf>|DevScene<\w+>|SahDeviceWork"):
            if not released(free, name, "release"):
                out.append(f"{struct}::{name}: no release()")
        for name in members(body, r"hipEvent_t"):
            if not released(free, name, "hipEventDestroy"):
                out.append(f"{struct}::{name}: no hipEventDestroy")
        for name in pointer_members(body):
            if name in BORROWED:
                continue
            if not released(free, name, "hipHostFree"):
                out.append(f"{struct}::{name}: no hipHostFree (or say in BORROWED why it owns nothing)")
        if struct == "CrHandle":
            if not re.search(r"hipStreamDestroy\s*\(\s*h->stream", free):
                out.append("CrHandle::stream: no hipStreamDestroy")
        if struct == "CrGroup":
            if not re.search(r"CommDestroy\s*\(\s*g->comms", free) or not re.search(r"cr_destroy\s*\(\s*g->members", free):
                out.append("CrGroup: comms or members not destroyed")
    return out


def test_the_parser_sees_the_members():
    by = {s: b for s, b, _ in owners()}
    h = members(by["CrHandle"], r"DevBuf")
    for name in ("fx_acc", "aov_acc", "aov_flags", "aov_counts", "ad_acc", "ad_lists", "ad_block_n", "ad_ctrl", "ad_counts", "out_buf", "sample_buf", "sg_acc",
                 "att_stack", "times_dev", "update_stage", "cam_dev", "images", "texels", "work_counter", "counters", "wf_job", "wf_acc"):
        assert name in h, name
    assert len(h) >= 30
    assert set(members(by["CrHandle"], r"hipEvent_t")) == {"ev0", "ev1", "cam_ev", "ad_ev0", "ad_ev1", "times_ev", "wf_ev"}
    assert set(pointer_members(by["CrHandle"])) == {"cam_host", "times_host", "wf_ring_host", "wf_ring_dev"}
    assert set(members(by["CrHandle"], r"DevScene<\w+>")) == {"s32", "s64", "f32", "f64"} and members(by["CrHandle"], r"SahDeviceWork") == ["sah_work"]
    d = members(by["DevScene"], r"DevBuf")
    for name in ("entries", "prims", "mats", "texs", "keys", "leaf_runs", "entries_refit", "screen", "screen_refit", "screen_overflow", "desc_pos", "frame_map"):
        assert name in d, name
    assert set(members(by["SahDeviceWork"], r"DevBuf")) == {"box", "order", "seg", "pbins", "flags", "scan", "tmp", "slots", "nodes", "small", "ctr"}
    assert set(members(by["CrGroup"], r"std::vector<DevBuf>")) == {"partial", "flags", "status"} and set(members(by["CrGroup"], r"hipEvent_t")) == {"ev0", "ev1"}


def test_every_member_is_released():
    assert missing() == []


def test_a_dropped_release_is_noticed():
    """What the check is worth: take one entry out of each list and it fails, naming the member."""
    global API, HANDLE, GROUP
    keep = API, HANDLE, GROUP
    try:
        for text, which, entry, name in ((API, "API", "h->ad_lists.release();", "CrHandle::ad_lists"),
                                         (API, "API", "h->cam_dev[i].release();", "CrHandle::cam_dev"),
                                         (API, "API", "if (h->times_ev) (void)hipEventDestroy(h->times_ev);", "CrHandle::times_ev"),
                                         (API, "API", "if (h->times_host) (void)hipHostFree(h->times_host);", "CrHandle::times_host"),
                                         (API, "API", "h->f64.release();", "CrHandle::f64"),
                                         (HANDLE, "HANDLE", "screen_overflow.release();", "DevScene::screen_overflow"),
                                         (HANDLE, "HANDLE", "&slots[1], ", None), (HANDLE, "HANDLE", "&scan, ", "SahDeviceWork::scan"),
                                         (GROUP, "GROUP", "if (i < g->flags.size()) g->flags[i].release();", "CrGroup::flags")):
            assert text.count(entry) == 1, entry
            globals()[which] = text.replace(entry, "")
            found = missing()
            API, HANDLE, GROUP = keep
            if name is None:        # slots[0] is still in the list: an array is one name
                assert found == [], found
            else:
                assert len(found) == 1 and found[0].startswith(name + ":"), (entry, found)
    finally:
        API, HANDLE, GROUP = keep
