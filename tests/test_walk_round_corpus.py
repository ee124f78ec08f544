"""The corpus of tests/walk_round_corpus.py reaches what it claims -- checked on the CPU, from the oracle and the exported trees
(tests/tree_check.cpp's, the host tree code without a device) alone: every ray group is there and sits on its edge, the counted
probe agrees with the plain probe and with a walker of the exported tree in plain Python on every ray, and the lane
assignments hold every ray once with partial waves."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import walk_round_corpus as W
from crucible_amd import _abi as A
from test_tree_host import parse_export, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"ref": A.CR_BVH_REFERENCE, "ord": A.CR_BVH_SAH_ORDERED}
KINDS = {"main": ("ref", "ord"), "list": ("ref",), "two": ("ref", "ord")}   # scene -> the tree modes it is walked under
COMMON = ["camera", "miss_root", "inside_out", "axis_two_zeros", "axis_one_zero", "tiny_direction", "far_origin"]


def build_tree_check(exe):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                           "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "tree_check.cpp")])


def host_tree(exe, tmp, flat, rt, mode):
    """(boxes, children, split_axis) of cr_export_bvh's shape from the host tree code, and the scene file's bytes."""
    path = tmp / f"scene_{rt}_{mode}.bin"
    write_scene(path, flat, rt, mode)
    res = subprocess.run([str(exe), "tree", str(path)], capture_output=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, res.stderr.decode()
    spliced, boxes, kids, axis, rest = parse_export(res.stdout.decode().splitlines())
    assert spliced == 0 and not rest and len(kids) > 0
    return (boxes, kids, axis), path.read_bytes()


def build_corpus(tmp, o64):
    """Per scene kind: the scene, its description, the f64 exported trees of its modes, the rays and their group names."""
    exe = tmp / "tree_check"
    build_tree_check(exe)
    out = {"exe": exe, "tmp": tmp}
    for kind, modes in KINDS.items():
        sc = W.scene(kind)
        flat = sc.flatten()
        trees = {m: host_tree(exe, tmp, flat, A.CR_REAL_F64, MODES[m])[0] for m in modes}
        rows, names = W.rays(kind, o64, sc, trees)
        out[kind] = {"scene": sc, "flat": flat, "trees": trees, "rows": rows, "names": names}
    return out


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, o64):
    return build_corpus(tmp_path_factory.mktemp("walk_round_corpus"), o64)


def probe_all(o, flat, rows, tree=None):
    """The counted probe of every ray: (hit, mat, t bits, node tests, primitive tests) arrays, and the plain probe's (hit, mat, record)."""
    h = o.scene_create(flat)
    n = len(rows)
    hit, mat, nodes, prims = np.zeros(n, bool), np.full(n, -1, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    t = np.zeros(n, dtype=o.np_real)
    plain = []
    try:
        if tree is not None:
            o.set_tree(h, *tree)
        rec = np.zeros(10, dtype=o.np_real)
        for k, ray in enumerate(rows):
            with np.errstate(over="ignore"):
                orig, d = o.arr(ray[0:3]), o.arr(ray[3:6])
            m = C.c_int32(-1)
            ph = o.lib.oracle_world_hit(h, o._p(orig), o._p(d), o.real(ray[6]), o.real(0.001), o.real(np.inf), o._p(rec), C.byref(m))
            plain.append((bool(ph), m.value, rec.tobytes() if ph else b""))
            hit[k], crec, cm, nodes[k], prims[k] = o.world_hit_counted(h, orig, d, ray[6])
            if hit[k]:
                mat[k], t[k] = cm, crec[0]
                assert (True, cm, crec.tobytes()) == plain[-1], ("the counted probe differs from the plain probe", k, ray)
            else:
                assert not ph, ("the counted probe differs from the plain probe", k, ray)
    finally:
        o.scene_destroy(h)
    bits = t.view(np.uint64 if o.np_real == np.float64 else np.uint32).astype(np.uint64)
    return {"hit": hit, "mat": mat, "t": t, "bits": bits, "nodes": nodes, "prims": prims}


def test_every_group_is_there(corpus):
    for kind, modes in KINDS.items():
        names = corpus[kind]["names"]
        want = COMMON + ["band_" + m for m in modes]
        if kind == "main":
            want += [g + m for m in modes for g in ("second_primitive_", "later_leaf_nearer_")]
        counts = {g: int((names == g).sum()) for g in want}
        print(f"\n[walk_round corpus] {kind}: {len(names)} rays, {counts}")
        assert set(names) == set(want)
        floor = 1 if kind == "two" else 8
        assert all(c >= floor for c in counts.values()), counts
    assert len(corpus["main"]["rows"]) + len(corpus["list"]["rows"]) + len(corpus["two"]["rows"]) < 2000   # tiny launches


@pytest.mark.parametrize("kind", list(KINDS))
def test_counted_probe_is_the_plain_probe_on_the_corpus(corpus, oracles, kind):
    """The hit, the record and the material of oracle_world_hit_counted are oracle_world_hit's (probe_all asserts it ray by ray),
    in both precisions, on the oracle's own tree and on the exported ordered tree with its split axes."""
    c = corpus[kind]
    for rt, o in oracles.items():
        for m in KINDS[kind]:
            tree = None if m == "ref" else host_tree(corpus["exe"], corpus["tmp"], c["flat"], rt, MODES[m])[0]
            got = probe_all(o, c["flat"], c["rows"], tree)
            assert got["hit"].any() and not got["hit"].all() and (got["nodes"] >= 1).all()


def test_groups_sit_on_their_edges(corpus, oracles, o64):
    for kind in KINDS:
        c = corpus[kind]
        rows, names = c["rows"], c["names"]
        root = c["trees"]["ref"][0][0].reshape(3, 2)
        with np.errstate(divide="ignore", over="ignore"):
            inv = 1.0 / rows[:, 3:6]
            inv32 = (1.0 / rows[:, 3:6].astype(np.float32))
        assert (np.isinf(inv[names == "axis_two_zeros"]).sum(axis=1) == 2).all()
        assert (np.isinf(inv[names == "axis_one_zero"]).sum(axis=1) == 1).all()
        others = ~np.isin(names, W.EXACT_GROUPS)
        assert np.isfinite(inv[others]).all() and np.isfinite(inv32[others]).all()   # the budgeted loops, in both precisions
        for g in W.UNSCREENED_GROUPS:   # finite 1/direction, but outside the range the f64 screen accepts
            assert all(W.screen_margin(root.ravel(), r) == np.inf for r in rows[names == g]), g
        assert (np.abs(rows[names == "far_origin", 0:3].astype(np.float32)).max(axis=1) > 2.0 ** 100).all()
        screened = ~np.isin(names, W.EXACT_GROUPS + W.UNSCREENED_GROUPS)
        assert all(np.isfinite(W.screen_margin(root.ravel(), r)) for r in rows[screened])
        inside = rows[names == "inside_out", 0:3]
        assert ((inside >= root[:, 0]) & (inside <= root[:, 1])).all()
        for o in oracles.values():   # a ray that misses the root box: one node test, no primitive test
            got = probe_all(o, c["flat"], rows[names == "miss_root"])
            assert not got["hit"].any() and (got["nodes"] == 1).all() and (got["prims"] == 0).all()


@pytest.mark.parametrize("mode", ["ref", "ord"])
def test_searched_groups_against_the_walker_and_the_counted_probe(corpus, o64, mode):
    """On the main scene the walker of the exported tree and the counted probe agree on every ray (closest primitive, t,
    node tests, primitive tests); by the walker's trace the band rays meet a box too close to call and go on
    stepping, the second-primitive rays end on the second child of a two-primitive leaf, and the later-leaf rays are hit in
    two leaves, the later one nearer."""
    c = corpus["main"]
    rows, names, tree = c["rows"], c["names"], c["trees"][mode]
    prims = W.prim_table(c["flat"])
    kids = tree[1]
    got = probe_all(o64, c["flat"], rows, None if mode == "ref" else tree)
    band_then_steps = 0
    for k, ray in enumerate(rows):
        best, t, nodes, nprims, events, visited = W.walk(o64, prims, tree, ray)
        assert (best >= 0) == bool(got["hit"][k]) and nodes == got["nodes"][k] and nprims == got["prims"][k], (names[k], k)
        if best >= 0:
            assert prims[best][2] == got["mat"][k] and np.float64(t).tobytes() == got["t"][k].tobytes(), (names[k], k)
        if names[k] == "band_" + mode:
            assert W.in_band(tree, ray), k
            band_then_steps += W.band_then_steps(o64, prims, tree, ray)
        if names[k] == "second_primitive_" + mode:
            w = events[-1][0]
            assert kids[w, 0] != kids[w, 1] and best == ~int(kids[w, 1]), k
        if names[k] == "later_leaf_nearer_" + mode:
            leaves = [w for w, _, _ in events]
            assert len(set(leaves)) >= 2 and all(a[2] > b[2] for a, b in zip(events, events[1:])), k
    print(f"\n[walk_round corpus] {mode}: {band_then_steps} band rays meet the band at an inner wrapper and step on")
    assert band_then_steps >= 8


def test_assignments_hold_every_ray_once_in_partial_waves():
    for n in (1, 63, 300, 471):
        t = W.assignments(n)
        assert t.shape[0] == len(W.PERM_SEEDS) and t.shape[2:] == (64, W.K) and t.dtype == np.int32
        for p in range(t.shape[0]):
            assert sorted(t[p][t[p] >= 0].tolist()) == list(range(n))
            held = (t[p] >= 0).sum(axis=-1)
            assert ((t[p] >= 0) == (np.arange(W.K) < held[..., None])).all()   # a queue has no holes
        if n >= 300:
            held = (t >= 0).sum(axis=-1)
            assert all((held == c).any() for c in (0, 1, 2, W.K)) and t.shape[1] >= 2   # partial waves, more than one block
            assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2])
    assert len(W.SCHEDULES) == 90 and len(set(W.SCHEDULES)) == 90
