"""The host tree code of crucible_amd/csrc/tree.hpp, checked without a device: tests/tree_check.cpp compiles it with g++ and
runs the stage functions build_dev_scene calls, in its order.  What comes out is held to the independent models and to the
oracle: the binned-SAH trees to tests/sah_model.py, the reference-mode tree to the oracle's own, the LBVH numbering to
tests/lbvh_model.py, the splice of BVHWrapper elements and the per-octant links of CR_BVH_SAH_ORDERED to their
definitions.  Every comparison is exact.  The program is built twice, plain and with -fsanitize=address,undefined; every case
runs in both and must print the same bytes with nothing on stderr -- among them node graphs no device may be made to
produce (lbvh_number's "malformed topology" returns)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import lbvh_model as L
import sah_model as M
import scenes
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.scene import HitList, Lambertian, Scene, Sphere
from scenes import SAH_HAND as HAND
from test_gpu_sah_build import SCENES
from test_lbvh_model_host import box_corpus
from test_sah_device_host import NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [(A.CR_REAL_F64, np.float64), (A.CR_REAL_F32, np.float32)]
REAL_IDS = ["f64", "f32"]
LEAF_RUN, LEAF_PSEUDO, LEAF_RUN_INDEX = 0x40000000, 0x20000000, 0x1FFFFFFF   # pathtrace.hpp kLeafRun, kLeafPseudo, kLeafRunIndex


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """(plain, sanitized)"""
    out = tmp_path_factory.mktemp("tree_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"tree_check_{tag}")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "tree_check.cpp")])
        built.append(exe)
    return built


def run_both(exes, what, path):
    """The program's output; the same bytes from both builds, nothing on stderr."""
    outs = []
    for exe in exes:
        res = subprocess.run([exe, what, str(path)], capture_output=True, timeout=300)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout)
    assert outs[0] == outs[1]
    return outs[0].decode().splitlines()


def write_scene(path, flat, rt, mode, tag_materials=False, hide=None):
    recs = L.prim_records(flat).copy()
    if hide is not None:
        recs["flags"][hide] |= L.HIDDEN
    if tag_materials:   # the tree code carries a record's material index and never reads it: here it names the descriptor
        recs["material"] = np.arange(len(recs))
    assert recs.dtype.itemsize == C.sizeof(A.CrPrimitive)
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", 1 if rt == A.CR_REAL_F64 else 0, mode, len(recs)))
        f.write(recs.tobytes())
    return recs


def parse_export(lines, with_boxes=True):
    """-> spliced, boxes (n, 6), children (n, 2), split_axis (n), the lines after the wrappers"""
    assert lines[0].split()[0] == "spliced" and lines[1].split()[0] == "wrappers"
    n = int(lines[1].split()[1])
    rows = [l.split() for l in lines[2:2 + n]]
    boxes = np.array([[float.fromhex(x) for x in r[:6]] for r in rows]).reshape(n, 6) if with_boxes else None
    ints = np.array([[int(x) for x in r[-3:]] for r in rows], dtype=np.int32).reshape(n, 3)
    return int(lines[0].split()[1]), boxes, ints[:, :2], ints[:, 2], lines[2 + n:]


# ------------------------------------------------------------------ sah
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED], ids=["sah", "ordered"])
@pytest.mark.parametrize("name", NAMES)
def test_sah_tree_equals_the_model(exes, tmp_path, name, mode, rt, real):
    flat = SCENES[name]().flatten()
    write_scene(tmp_path / "in.bin", flat, rt, mode)
    spliced, boxes, kids, axis, rest = parse_export(run_both(exes, "tree", tmp_path / "in.bin"))
    want = M.build(flat, real, mode)
    assert spliced == 0 and not rest and len(kids) == len(want.children) > 0
    assert np.array_equal(kids, want.children)
    assert np.array_equal(axis, want.split_axis)
    assert np.array_equal(boxes, want.boxes)
    if name.startswith("hand_"):
        _, children, hand_axis, _ = HAND[name[5:]]
        assert kids.tolist() == children and axis.tolist() == (hand_axis if mode == A.CR_BVH_SAH_ORDERED else [-1] * len(hand_axis))


# ------------------------------------------------------------------ reference
def listed_spheres(how):
    """The static scene of test_gpu_lists.py::test_a_list_is_its_objects_when_nothing_clips: a list grown by add(), or from
    HitList::new (its box stays empty)."""
    sc = Scene.new_image(16.0 / 9.0, 96, 1, 360.0, 1)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)), "ground")
    rs = np.random.RandomState(4)
    objs = [Sphere.new((rs.uniform(-4, 4), 0.3, rs.uniform(-3, 3)), 0.3, Lambertian.new_from_color(tuple(rs.uniform(0.1, 0.9, 3)), 1.0)) for _ in range(24)]
    if how == "add":
        l = HitList.default()
        for o in objs:
            l.add(o)
        sc.add_element(l, "l")
    else:
        sc.add_element(HitList.new(objs), "l")
    return sc


REFERENCE_SCENES = {
    "book1": lambda: book1_end_scene(1, scene_seed=2, image_width=32, samples=1), "mixed": lambda: scenes.mixed_scene(32, 1),
    "one": lambda: scenes.few_spheres(1), "two": lambda: scenes.few_spheres(2), "five": lambda: scenes.few_spheres(5),
    "lists_mixed": lambda: scenes.list_scene(32, 1, variant="mixed"), "only_lists": lambda: scenes.list_scene(32, 1, variant="only_lists"),
    "one_list": lambda: scenes.list_scene(32, 1, variant="one_list"), "list_add": lambda: listed_spheres("add"), "list_new": lambda: listed_spheres("new"),
}


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", list(REFERENCE_SCENES))
def test_reference_tree_is_the_oracle_tree(exes, oracles, tmp_path, name, rt, real):
    flat = REFERENCE_SCENES[name]().flatten()
    write_scene(tmp_path / "in.bin", flat, rt, A.CR_BVH_REFERENCE)
    spliced, boxes, kids, axis, rest = parse_export(run_both(exes, "tree", tmp_path / "in.bin"))
    assert spliced == 0 and not rest and (axis == -1).all()
    o = oracles[rt]
    h = o.scene_create(flat)
    try:
        cap = len(kids) + 8
        oboxes = np.zeros((cap, 6), dtype=o.np_real)
        okids = np.zeros((cap, 2), dtype=np.int32)
        n = o.lib.oracle_bvh_dump(h, oboxes.ctypes.data, okids.ctypes.data, cap)
    finally:
        o.scene_destroy(h)
    assert n == len(kids) > 0
    assert np.array_equal(boxes, oboxes[:n].astype(np.float64))
    # the oracle's dump marks wrapper children -1 and names primitives by list index
    assert np.array_equal(np.where(kids >= 0, -1, ~kids), okids[:n])
    if "list" in name:
        named = {~c for c in kids.ravel() if c < 0}
        assert any(flat.prims[i].kind == A.CR_PRIM_LIST for i in named) and not any(flat.prims[i].flags & A.CR_PRIM_MEMBER for i in named)


# ------------------------------------------------------------------ splice
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("variant", ["mixed", "only", "only_hidden", "pair", "small"])
def test_spliced_records_name_every_primitive_once(exes, tmp_path, variant, rt, real):
    """"only": a span-1 root (the element alone in its leaf wrapper); "only_hidden": the same with one of its members
    hidden in the description itself (the scene classes drop a wrapper's hidden objects before it gets there); "small": an
    element of one object, and one without a visible object."""
    flat = scenes.wrapped_scene(32, 1, variant=variant.split("_")[0]).flatten()
    hide = None
    if variant == "only_hidden":
        hide = int(np.nonzero(L.prim_records(flat)["flags"] & L.MEMBER)[0][4])
    recs = write_scene(tmp_path / "in.bin", flat, rt, A.CR_BVH_REFERENCE, tag_materials=True, hide=hide)
    lines = run_both(exes, "tree", tmp_path / "in.bin")
    assert lines[0] == "spliced 1"
    n = int(lines[1].split()[1])
    rec = np.array([[int(x) for x in l.split()] for l in lines[2:2 + n]], dtype=np.int64).reshape(n, 2)
    at = 2 + n
    n_runs = int(lines[at].split()[1])
    runs = np.array([[int(x) for x in l.split()] for l in lines[at + 1:at + 1 + n_runs]], dtype=np.int64).reshape(n_runs, 2)
    at += 1 + n_runs
    n_prims = int(lines[at].split()[1])
    prim_desc = [int(l) for l in lines[at + 1:at + 1 + n_prims]]
    assert at + 1 + n_prims == len(lines) and n > 0
    # following the links from record 0 visits every record exactly once and ends at the count
    seen, k = [], 0
    while k != n:
        assert 0 <= k < n and len(seen) < n
        seen.append(k)
        k = -rec[k, 0] if rec[k, 0] < 0 else rec[k, 1]
    assert sorted(seen) == list(range(n))
    # the runs of the leaves
    spans, n_pseudo, empty_pseudo = [], 0, 0
    used_runs = []
    for leaf in rec[rec[:, 0] >= 0, 0]:
        if leaf & LEAF_RUN:
            idx = int(leaf & LEAF_RUN_INDEX)
            assert idx < n_runs
            used_runs.append(idx)
            first, count = runs[idx]
            pseudo = bool(leaf & LEAF_PSEUDO)
            n_pseudo += pseudo
            empty_pseudo += pseudo and count == 0
            assert pseudo or count not in (1, 2)
        else:
            assert not leaf & LEAF_PSEUDO
            first, count = leaf >> 1, (leaf & 1) + 1
        assert 0 <= first and count >= 0 and first + count <= n_prims      # inside leaf_prims
        spans.append((int(first), int(count)))
    assert sorted(used_runs) == list(range(n_runs))
    covered = np.zeros(n_prims, dtype=np.int32)
    for first, count in spans:
        covered[first:first + count] += 1
    assert (covered == 1).all()                                             # no overlap, nothing left out
    # together: the scene's visible primitives, each inner element's once
    vis = L.visible_prims(recs)
    assert sorted(prim_desc) == sorted(vis.tolist()) and len(set(prim_desc)) == len(prim_desc)
    assert ((recs["flags"][vis] & L.MEMBER) != 0).sum() >= 1
    if variant.startswith("only"):
        assert empty_pseudo == 1 and rec[0, 0] < 0                          # the element twice: an empty record is the second child
        members = np.nonzero(recs["flags"] & L.MEMBER)[0]
        n_hidden = int(((recs["flags"][members] & L.HIDDEN) != 0).sum())
        assert n_hidden == (variant == "only_hidden") and len(prim_desc) == len(members) - n_hidden
    if variant == "mixed":
        assert n_pseudo > empty_pseudo                                      # a primitive or list beside an element


# ------------------------------------------------------------------ lbvh
def lbvh_scenes():
    corpus = box_corpus()
    sph, tri = corpus[6], corpus[171]
    assert sph[0] == L.SPHERE and tri[0] == L.TRIANGLE
    pick = {"n1": [corpus[0]], "n2": [corpus[1], tri], "n3": [sph, tri, corpus[3]],
            "duplicates": [sph, tri, sph, corpus[0], sph, tri, corpus[165], corpus[172]]}
    return {k: scenes.ArrayScene([kind for kind, _ in v], np.array([row for _, row in v])) for k, v in pick.items()}


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", ["n1", "n2", "n3", "duplicates"])
def test_lbvh_numbering_equals_the_model(exes, tmp_path, name, rt, real):
    flat = lbvh_scenes()[name].flatten()
    write_scene(tmp_path / "in.bin", flat, rt, A.CR_BVH_LBVH)
    spliced, _, kids, axis, rest = parse_export(run_both(exes, "lbvh", tmp_path / "in.bin"), with_boxes=False)
    want = L.build(flat, real)
    assert spliced == 0 and (axis == -1).all()
    assert np.array_equal(kids, want.children)
    assert rest[0] == f"order {len(want.order)}" and [int(x) for x in rest[1:]] == want.order.tolist()
    if name == "duplicates":
        assert len(np.unique(want.keys)) < len(want.keys) - 2


BAD_GRAPHS = {   # n = 4 primitives: internal nodes 0..2, two children each; ~p names sorted primitive p
    "child_out_of_range": [3, ~0, ~1, ~2, ~3, ~0], "child_far_out_of_range": [2 ** 31 - 1, ~0, ~1, ~2, ~3, ~0],
    "leaf_out_of_range": [1, 2, ~0, ~4, ~2, ~3], "leaf_far_out_of_range": [1, 2, ~0, -2 ** 31, ~2, ~3],
    "node_twice": [1, 1, ~0, ~1, ~2, ~3], "cycle": [1, ~0, 0, ~1, ~2, ~3], "self_cycle": [0, ~0, ~1, ~2, ~3, ~0],
    "too_few_children": [1, 2, ~0, ~1],
}


@pytest.mark.parametrize("name", list(BAD_GRAPHS))
def test_numbering_refuses_a_malformed_graph(exes, tmp_path, name):
    """What build_lbvh answers with "malformed topology from the device": no GPU test may reach it."""
    g = BAD_GRAPHS[name]
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(struct.pack(f"<2i{len(g)}i", 4, len(g), *g))
    assert run_both(exes, "number", tmp_path / "g.bin") == ["ok 0"]


def test_numbering_takes_a_proper_graph(exes, tmp_path):
    g = [1, 2, ~0, ~1, ~2, ~3]
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(struct.pack(f"<2i{len(g)}i", 4, len(g), *g))
    assert run_both(exes, "number", tmp_path / "g.bin") == ["ok 1 7"]


# ------------------------------------------------------------------ links
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", ["r300"] + ["hand_" + n for n in HAND])
def test_ordered_links_walk_every_record_once(exes, tmp_path, name, rt, real):
    flat = SCENES[name]().flatten()
    write_scene(tmp_path / "in.bin", flat, rt, A.CR_BVH_SAH_ORDERED)
    rows = np.array([[int(x) for x in l.split()] for l in run_both(exes, "links", tmp_path / "in.bin")], dtype=np.int64)
    n = len(rows)
    assert n == len(M.build(flat, real, M.ORDERED).children) and rows.shape == (n, 18)
    left, axis, near, skip = rows[:, 0], rows[:, 1], rows[:, 2:10], rows[:, 10:18]
    inner = left >= 0
    assert inner.sum() == (n - 1) // 2 and ((axis >= 0) == inner).all() and (axis <= 2).all()
    for o in range(8):
        seen, k = [], 0
        while k != n:
            assert 0 <= k < n and len(seen) < n
            seen.append(k)
            k = near[k, o] if inner[k] else skip[k, o]
        assert sorted(seen) == list(range(n)), o
        bit = (o >> axis[inner]) & 1
        assert np.array_equal(near[inner, o], left[inner] + bit)           # the left child exactly when bit `axis` of o is 0
