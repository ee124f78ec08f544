"""tests/lds_capacity.py, the CPU restatement that tests/test_gpu_lds_capacity.py predicts residencies with, held to the
library's own headers without a device: the record sizes and slot bytes to what g++ prints for records.hpp and
launch_plan.hpp (tests/record_sizes_check.cpp), the layout to residency.hpp through tests/residency_check.cpp's layout
cases, the wrapper count to tree.hpp through tests/tree_check.cpp; then the scenes the search finds: how near each comes to
its threshold, and that a render of one really reads the records at the ends of its tables."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import lbvh_model as L
import lds_capacity as K
import scenes
from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crucible_amd", "csrc")
SAN = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def compile_check(out, name, flags=(), extra=()):
    exe = str(out / (name + ("_san" if extra else "")))
    subprocess.check_call(["g++", "-O1", "-std=c++17", *flags, *extra, "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("lds_capacity")
    return {"sizes": [compile_check(out, "record_sizes_check", ("-Wall", "-Werror")), compile_check(out, "record_sizes_check", ("-Wall", "-Werror"), SAN)],
            "layout": [compile_check(out, "residency_check", ("-Wall", "-Werror")), compile_check(out, "residency_check", ("-Wall", "-Werror"), SAN)],
            "tree": [compile_check(out, "tree_check", ("-ffp-contract=off", "-pthread"))]}


def run(exes, *args):
    """The program's lines; the same from every build of it, nothing on stderr."""
    outs = []
    for exe in exes:
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert len(set(outs)) == 1
    return outs[0].splitlines()


# ---------------------------------------------------------------------------------------------------- sizes and thresholds
def test_record_sizes_and_slot_bytes_are_the_headers(programs):
    got = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in run(programs["sizes"])}
    for field in ("entry", "entry_o", "screen", "screen_o", "prim", "mat", "tex"):
        assert got[field] == (K.SIZES[K.F64][field], K.SIZES[K.F32][field]), field
    assert got["max_block"] == (K.MAX_BLOCK, K.MAX_BLOCK)
    for tile in (4, 5, 6):
        assert got[f"fx_lds_{tile}"] == (K.fx_lds_bytes(K.MAX_BLOCK, tile),) * 2
    assert got["aov_lds"] == (K.aov_lds_bytes(K.MAX_BLOCK),) * 2
    # what the issue's table says, written out: a threshold off by one slot size shows here before it shows on a device
    assert got["fx_lds_4"][0] == 12288 and got["aov_lds"][0] == 16384
    assert K.THRESHOLDS == {"reference": 163840, "relaxed": 151552, "guide": 147456, "tile8x8": 114688, "tile8x4": 139264}
    assert K.T_TILE_8X4 == K.LDS - K.fx_lds_bytes(K.MAX_BLOCK, 5) and K.T_TILE_8X8 == K.LDS - got["fx_lds_6"][0]
    # queue.hpp:33: 1024 slots of 112 (f64) / 68 (f32) bytes, 8192 bytes of rings, 64 of control words
    assert (K.queue_state_bytes(K.F64), K.queue_state_bytes(K.F32)) == (122944, 77888)
    assert (K.queue_threshold(K.F64), K.queue_threshold(K.F32)) == (40880, 85936)
    # a default window with full side tables and the guide slots fills the LDS exactly (f32: 4096 records of 32 bytes)
    assert K.WINDOW + K.SIDE_LIMIT + K.aov_lds_bytes(K.MAX_BLOCK) == K.LDS == 4096 * K.SIZES[K.F32]["entry"] + 32768


def layout_cases():
    cases = []
    for name, row in K.ROWS.items():
        s = K.SIZES[row.rt]
        for n, w, m, t in [(3, 3, 3, 3), (1151, 1277, 2, 2), (1316, 1607, 2, 1), (4097, 4097, 256, 256), (33, 33, 67, 67), (5, 7, 0, 0), (2, 1, 1, 0)]:
            for with_prims, with_side in ((1, 1), (1, 0), (0, 1), (0, 0)):
                cases.append((s, s[row.record], n, w, m, t, with_prims, with_side))
    return cases


def test_layout_is_residency_hpp(programs, tmp_path):
    cases = layout_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"L {w} {rec} {n} {s['prim']} {m} {s['mat']} {t} {s['tex']} {wp} {ws}\n" for s, rec, n, w, m, t, wp, ws in cases))
    lines = run(programs["layout"], path)
    assert len(lines) == len(cases)
    for (s, rec, n, w, m, t, wp, ws), line in zip(cases, lines):
        want = K.scene_layout(w * rec, n * s["prim"], m * s["mat"], t * s["tex"], bool(wp), bool(ws))
        assert tuple(int(x) for x in line.split()) == tuple(want), (rec, n, w, m, t, wp, ws)
    # the issue's two examples
    assert K.layout_of("f64", 1151, 1277, 2, 2) == 151552 and K.layout_of("f32", 1316, 1607, 2, 1) == 114688
    assert K.side_table_bytes(K.F32, 256, 256) == 16384 and K.side_table_bytes(K.F32, 256, 257) == 16416


def write_prims(path, flat, rt, mode):
    recs = L.prim_records(flat)
    assert recs.dtype.itemsize == C.sizeof(A.CrPrimitive)
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", 1 if rt == A.CR_REAL_F64 else 0, mode, len(recs)))
        f.write(recs.tobytes())


def host_tree(programs, path):
    """tree.hpp's reference tree of the description at `path`: (wrappers, the primitives its leaves name in walk order)"""
    lines = run(programs["tree"], "tree", path)
    assert lines[0] == "spliced 0"
    n = int(lines[1].split()[1])
    kids = np.array([[int(x) for x in l.split()[-3:-1]] for l in lines[2:2 + n]], dtype=np.int64).reshape(n, 2)
    return n, [~c for c in kids.ravel() if c < 0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 32, 33, 100, 1000, 4096, 4097])
def test_tree_size_is_tree_hpp(programs, tmp_path, n):
    k = np.arange(n)
    sc = scenes.sah_spheres(np.stack([(k % 64) * 1.0, ((k // 64) % 8) * 1.0, (k // 512) * 1.0], axis=1), np.full(n, 0.25))
    write_prims(tmp_path / "in.bin", sc.flatten(), A.CR_REAL_F64, A.CR_BVH_REFERENCE)
    wrappers, _ = host_tree(programs, tmp_path / "in.bin")
    assert wrappers == K.tree_size(n) and wrappers % 2 == 1


# ---------------------------------------------------------------------------------------------------- the search
# (row, threshold) pairs that must land on the byte: gap 0 below, 16 above
EXACT = {("f64", "reference"), ("f64", "relaxed"), ("f64", "guide"), ("f32", "relaxed"), ("f32", "guide"), ("f32", "tile8x8")}


@pytest.mark.parametrize("name", list(K.THRESHOLDS))
@pytest.mark.parametrize("row", K.UNORDERED)
def test_gap_and_excess(row, name):
    threshold = K.THRESHOLDS[name]
    at, over = K.find(row, threshold)
    gap, excess = threshold - at.bytes, over.bytes - threshold
    print(f"{row} {name} {threshold}: at {tuple(at)} gap {gap}, over {tuple(over)} excess {excess}")
    for f in (at, over):
        assert f.wrappers == K.tree_size(f.n) and f.bytes == K.layout_of(row, f.n, f.wrappers, f.mats, f.texs)
        wide = 2 if (row, name) == ("f64-wrappers", "guide") else 1   # (lds_capacity.find: the one place the narrow search cannot reach)
        assert K.MIN_MATS <= f.mats <= K.MIN_MATS + wide * K.MAX_FILL and K.MIN_TEXS <= f.texs <= K.MIN_TEXS + wide * K.MAX_FILL
    assert 0 <= gap <= 32 and 0 < excess <= 32
    assert K.predict(at.bytes, threshold) == 1 and K.predict(over.bytes, threshold) == 2
    if (row, name) in EXACT:
        assert (gap, excess) == (0, 16)


def test_pipeline_thresholds_are_reachable():
    """The queue pipeline counts the wrappers' layout (ds.lds_bytes); the wavefront pipeline stages wrappers | primitives
    alone, so only the sphere count moves its layout: 96 + 64 or 48 + 32 bytes a step, two steps where the wrapper count does."""
    for row, rt in (("f64-wrappers", K.F64), ("f32", K.F32)):
        at, over = K.find(row, K.queue_threshold(rt))
        print(f"{row} queue {K.queue_threshold(rt)}: at {tuple(at)}, over {tuple(over)}")
        assert 0 <= K.queue_threshold(rt) - at.bytes <= 32 and 0 < over.bytes - K.queue_threshold(rt) <= 32
        at, over = K.find(row, K.LDS, False)
        print(f"{row} wavefront {K.LDS}: at {tuple(at)}, over {tuple(over)}")
        step = 2 * (K.SIZES[rt]["prim"] + K.SIZES[rt]["entry"])
        assert 0 <= K.LDS - at.bytes < step and 0 < over.bytes - K.LDS <= step and over.n == at.n + 1


# ---------------------------------------------------------------------------------------------------- the scene proves something
def probe(oracle, sc):
    """The wrapper count and leaf order of the oracle's tree, the material of the closest hit of every camera ray of the render
    (-1: the sky), and the colours the ground's hits read from the last texture"""
    cam, flat = sc.scene_cam, sc.flatten()
    lib, R = oracle.lib, oracle.np_real
    cd, p = cam.desc(), cam.params(1, oracle.real_type, 0, None, 0, A.CR_SUM_DEFAULT)
    n_mats, n_texs = flat.desc.n_materials, flat.desc.n_textures
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    h = oracle.scene_create(flat)
    mats, colours = [], []
    try:
        oracle.render(h, cam, seed=1, pix_begin=0, pix_end=1, n_threads=1)   # primes the scene's boxes (tests/test_gpu_aov.py model)
        cap = K.tree_size(flat.desc.n_prims) + 8
        boxes, kids = np.zeros((cap, 6), dtype=R), np.zeros((cap, 2), dtype=np.int32)
        n = lib.oracle_bvh_dump(h, boxes.ctypes.data, kids.ctypes.data, cap)
        leaves = [int(c) for c in kids[:n].ravel() if c >= 0]
        ray, rec, col = np.zeros(8, dtype=R), np.zeros(10, dtype=R), np.zeros(3, dtype=R)
        mat = C.c_int32()
        # the render's own probes: the camera ray of every sample of every pixel
        for j in range(cam.image_height):
            for i in range(cam.image_width):
                for s in range(cam.samples):
                    lib.oracle_camera_ray(C.byref(cd), C.byref(p), i, j, s, ptr(ray))
                    o, d = np.ascontiguousarray(ray[0:3]), np.ascontiguousarray(ray[3:6])
                    if lib.oracle_world_hit(h, ptr(o), ptr(d), oracle.real(ray[6]), oracle.real(0.001), oracle.real(np.inf), ptr(rec), C.byref(mat)):
                        mats.append(mat.value)
                        if mat.value == n_mats - 1:
                            assert flat.materials[mat.value].texture == n_texs - 1
                            loc = np.ascontiguousarray(rec[1:4])
                            lib.oracle_texture_value(h, n_texs - 1, oracle.real(rec[7]), oracle.real(rec[8]), ptr(loc), ptr(col))
                            colours.append(tuple(float(c) for c in col))
                    else:
                        mats.append(-1)
    finally:
        oracle.scene_destroy(h)
    return n, leaves, mats, colours


@pytest.mark.parametrize("row", K.UNORDERED)
def test_the_at_scene_reads_the_ends_of_its_tables(oracles, programs, tmp_path, row):
    """The sphere at leaf position 0 (the ground: the last material, whose checker is the last texture) and the sphere at the
    last leaf position (the marker: material 0, its alone) are each some camera ray's closest hit; the ground's hits read
    the last texture and get colours of several of the solid textures under it; every material is some sphere's.  A scene
    that fails this would let stage_scene drop the end of a table unnoticed."""
    rt = K.ROWS[row].rt
    at, _ = K.find(row, K.T_RELAXED)
    sc = K.scene_of(at)
    flat = sc.flatten()
    n = flat.desc.n_prims
    assert (n, flat.desc.n_materials, flat.desc.n_textures) == (at.n, at.mats, at.texs)
    wrappers, leaves, mats, colours = probe(oracles[rt], sc)
    assert wrappers == K.tree_size(n) == at.wrappers
    assert leaves[0] == 0 and leaves[-1] == n - 1                       # ground first, marker last, in the oracle's tree
    write_prims(tmp_path / "in.bin", flat, rt, A.CR_BVH_REFERENCE)
    host_wrappers, host_leaves = host_tree(programs, tmp_path / "in.bin")
    assert host_wrappers == wrappers and host_leaves == leaves          # ... and in tree.hpp's
    assert flat.prims[0].material == at.mats - 1 and flat.prims[n - 1].material == 0
    assert sum(1 for k in range(n) if flat.prims[k].material in (0, at.mats - 1)) == 2
    assert {flat.prims[k].material for k in range(n)} == set(range(at.mats))
    assert {flat.materials[k].kind for k in range(at.mats)} == {A.CR_MAT_LAMBERTIAN, A.CR_MAT_METAL, A.CR_MAT_DIELECTRIC}
    assert mats.count(0) >= 4 and mats.count(at.mats - 1) >= 100 and mats.count(-1) >= 20, (mats.count(0), mats.count(at.mats - 1), mats.count(-1))
    assert len(set(mats) - {-1, 0, at.mats - 1}) >= min(2, at.mats - 2)   # and the grid's spheres
    solid = {tuple(flat.textures[k].color) for k in range(at.texs) if flat.textures[k].kind == A.CR_TEX_SOLID}
    R = oracles[rt].np_real
    assert len(set(colours)) >= 3 and set(colours) <= {tuple(float(R(c)) for c in s) for s in solid}
    # every texture hangs under the last one
    live = {at.texs - 1}
    for k in range(at.texs - 1, -1, -1):
        if k in live and flat.textures[k].kind == A.CR_TEX_CHECKER:
            live |= {flat.textures[k].even, flat.textures[k].odd}
    assert live == set(range(at.texs)) and {flat.textures[at.texs - 1].even, flat.textures[at.texs - 1].odd} == {at.texs - 2, at.texs - 3}
