"""crucible_amd/csrc/residency.hpp, the rule that settles how much of a scene a launch stages in LDS (shared by the render's
walk_ladder and the guide pass's aov_ladder_ord), checked without a device (launch()'s chunk and tile rules, once here, are
part of the launch plan: tests/test_launch_plan_host.py):
tests/residency_check.cpp compiles the header with g++ (plain, and with -fsanitize=address,undefined) and prints the
decision of each case.  The expected decisions below are written out by hand from the rule, not computed
by a second copy of it: (res, screen, latency, lds_entries, lds_side, lds_bytes, clear_screen).  So are the offsets of the layout
that the rule, every launch's byte count and the kernels' stage_scene share (scene_layout): (prims, mats, texs, bytes, end)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL, LDS, TOP = 0, 1, 2

# bytes of a wrapper record and of a screening record, per tree (an ordered f32 tree has no screening records and no SCREEN
# kernels: can_screen is false there, and the ladder still hands the ordered screening record's size over)
F64 = dict(entry_rec=64, screen_rec=32, ordered=0, can_screen=1, f32=0)
F64_ORD = dict(entry_rec=96, screen_rec=64, ordered=1, can_screen=1, f32=0)
F32 = dict(entry_rec=32, screen_rec=32, ordered=0, can_screen=1, f32=1)
F32_ORD = dict(entry_rec=64, screen_rec=64, ordered=1, can_screen=0, f32=1)

FIELDS = ("n_entries entry_rec screen_rec ordered can_screen screen screen_lds plain_lds lds_bytes lds_all_screen side_bytes "
          "lds_top_bytes lds_side_limit f32 whole_frame adaptive latency_entries latency_top_bytes latency_slot_bytes").split()
# a handle's defaults: a 128 KB window, side tables up to 16 KB, the 6-waves-per-SIMD entry point never (its window 48 KB,
# its slots fx_lds_bytes(512, 4) = 6144); a whole frame outside an adaptive run; a tree too large for LDS, walked on its
# screening records
DEFAULTS = dict(screen=1, screen_lds=0, plain_lds=0, lds_bytes=9000, lds_all_screen=5800, side_bytes=0, lds_top_bytes=128 * 1024,
                lds_side_limit=16 * 1024, whole_frame=1, adaptive=0, latency_entries=0, latency_top_bytes=48 * 1024, latency_slot_bytes=6144)


def R(tree, n_entries, **kw):
    q = dict(DEFAULTS, **tree)
    q.update(kw, n_entries=n_entries)
    assert sorted(q) == sorted(FIELDS)
    return "R " + " ".join(str(int(q[k])) for k in FIELDS)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("residency_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"residency_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "residency_check.cpp")])
        built.append(exe)
    return built


def check(exes, tmp_path, cases):
    """cases: (name, the case's line, the expected numbers); both builds print them."""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in cases))
    outs = []
    for exe in exes:
        res = subprocess.run([exe, path], capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    got = [tuple(int(x) for x in line.split()) for line in outs[0].splitlines()]
    assert len(got) == len(cases)
    for (name, _, want), g in zip(cases, got):
        assert g == tuple(want), (name, g, want)


def test_lds_row(exes, tmp_path):
    check(exes, tmp_path, [
        ("both fit: the screen wins", R(F64, 100, screen_lds=1, plain_lds=1), (LDS, 1, 0, 100, 0, 5800, 0)),
        ("screen_lds off: the plain kernel, and the screening pointer goes", R(F64, 100, plain_lds=1), (LDS, 0, 0, 100, 0, 9000, 1)),
        ("only the screen fits", R(F64, 100, screen_lds=1), (LDS, 1, 0, 100, 0, 5800, 0)),
        ("ordered f64", R(F64_ORD, 100, screen_lds=1, plain_lds=1), (LDS, 1, 0, 100, 0, 5800, 0)),
        ("no SCREEN kernels: plain even if screen_lds were set", R(F32_ORD, 100, screen_lds=1, plain_lds=1), (LDS, 0, 0, 100, 0, 9000, 1)),
        ("the side tables are part of lds_bytes: lds_side stays 0", R(F32, 100, plain_lds=1, screen=0, side_bytes=64), (LDS, 0, 0, 100, 0, 9000, 1)),
        ("the 6-waves-per-SIMD entry point is not asked", R(F32, 100, plain_lds=1, screen=0, latency_entries=1), (LDS, 0, 0, 100, 0, 9000, 1)),
        ("no entries, everything fits: GLOBAL", R(F64, 0, screen=0, screen_lds=1, plain_lds=1), (GLOBAL, 0, 0, 0, 0, 0, 0)),
        ("no entries, a window: GLOBAL", R(F64, 0, screen=0), (GLOBAL, 0, 0, 0, 0, 0, 0)),
    ])


def test_window_size(exes, tmp_path):
    KB = dict(lds_top_bytes=1024)
    check(exes, tmp_path, [
        ("128 KB of 32-byte screening records", R(F64, 10000), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("128 KB of 64-byte wrappers", R(F64, 10000, screen=0), (TOP, 0, 0, 2048, 1, 131072, 0)),
        ("1 KB, f64 screen", R(F64, 10000, **KB), (TOP, 1, 0, 32, 1, 1024, 0)),
        ("1 KB, f64 wrappers", R(F64, 10000, screen=0, **KB), (TOP, 0, 0, 16, 1, 1024, 0)),
        ("1 KB, ordered f64 screen", R(F64_ORD, 10000, **KB), (TOP, 1, 0, 16, 0, 1024, 0)),
        ("1 KB, ordered f64 wrappers: 10 of 96 bytes", R(F64_ORD, 10000, screen=0, **KB), (TOP, 0, 0, 10, 0, 960, 0)),
        ("1 KB, f32", R(F32, 10000, **KB), (TOP, 1, 0, 32, 1, 1024, 0)),
        ("1 KB, ordered f32: wrappers, no SCREEN kernel", R(F32_ORD, 10000, screen=0, **KB), (TOP, 0, 0, 16, 0, 1024, 0)),
        ("a window below one record", R(F64, 10000, lds_top_bytes=31), (GLOBAL, 1, 0, 0, 0, 0, 0)),
        ("exactly one record", R(F64, 10000, lds_top_bytes=32), (TOP, 1, 0, 1, 1, 32, 0)),
        ("a tree below the window", R(F64, 5), (TOP, 1, 0, 5, 1, 160, 0)),
    ])


def test_side_tables(exes, tmp_path):
    check(exes, tmp_path, [
        ("at the limit: they join", R(F64, 10000, side_bytes=16384), (TOP, 1, 0, 4096, 1, 147456, 0)),
        ("16 bytes over: they stay out", R(F64, 10000, side_bytes=16400), (TOP, 1, 0, 4096, 0, 131072, 0)),
        ("limit 0", R(F64, 10000, side_bytes=16, lds_side_limit=0), (TOP, 1, 0, 4096, 0, 131072, 0)),
        ("limit 0, no tables: 0 <= 0 joins", R(F64, 10000, side_bytes=0, lds_side_limit=0), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("an ordered tree never takes them", R(F64_ORD, 10000, side_bytes=64), (TOP, 1, 0, 2048, 0, 131072, 0)),
        ("an ordered tree, no tables", R(F64_ORD, 10000, side_bytes=0), (TOP, 1, 0, 2048, 0, 131072, 0)),
        # (every record size of the library is a multiple of 16; 40 bytes shows the rounding: 25 records, 1000 -> 1008 bytes)
        ("the window is rounded up to 16 before they follow", R(dict(F64, entry_rec=40), 10000, screen=0, lds_top_bytes=1024, side_bytes=32),
         (TOP, 0, 0, 25, 1, 1040, 0)),
        ("no rounding without them", R(dict(F64, entry_rec=40), 10000, screen=0, lds_top_bytes=1024, side_bytes=32, lds_side_limit=16),
         (TOP, 0, 0, 25, 0, 1000, 0)),
    ])


def test_latency(exes, tmp_path):
    small = dict(latency_entries=1, latency_top_bytes=1024)     # two 32-byte records: used = 64 + 6144, cap = 54597 - 6208 = 48389
    large = dict(latency_entries=1000)                          # 48 KB: 1536 records, used = 49152 + 6144 = 55296 > 54597, cap 0
    mid = dict(latency_entries=1000, latency_top_bytes=40960)   # 1280 records, used = 47104, cap = 7493
    check(exes, tmp_path, [
        ("on: two records", R(F32, 2, **small), (TOP, 0, 1, 2, 1, 64, 0)),
        ("the handle's limit binds", R(F32, 2, side_bytes=16384, **small), (TOP, 0, 1, 2, 1, 16448, 0)),
        ("over the handle's limit", R(F32, 2, side_bytes=16400, **small), (TOP, 0, 1, 2, 0, 64, 0)),
        ("never a SCREEN kernel, with or without w.screen", R(F32, 2, screen=0, **small), (TOP, 0, 1, 2, 1, 64, 0)),
        ("ordered: no side tables", R(F32_ORD, 2, screen=0, **small), (TOP, 0, 1, 2, 0, 128, 0)),
        ("48 KB: 1536 records, cap 0, no tables join", R(F32, 100000, **large), (TOP, 0, 1, 1536, 1, 49152, 0)),
        ("48 KB: cap 0, any table stays out", R(F32, 100000, side_bytes=16, **large), (TOP, 0, 1, 1536, 0, 49152, 0)),
        ("40 KB: the share of 160 KB binds, 7488 <= 7493", R(F32, 100000, side_bytes=7488, **mid), (TOP, 0, 1, 1280, 1, 48448, 0)),
        ("40 KB: 7504 > 7493", R(F32, 100000, side_bytes=7504, **mid), (TOP, 0, 1, 1280, 0, 40960, 0)),
        ("its window holds no record: GLOBAL on the regular kernel", R(F32, 100000, latency_entries=1000, latency_top_bytes=31), (GLOBAL, 1, 0, 0, 0, 0, 0)),
        # off: the handle's own window (128 KB) and the regular kernels
        ("off: n == latency_entries", R(F32, 2, latency_entries=2, latency_top_bytes=1024), (TOP, 1, 0, 2, 1, 64, 0)),
        ("off: a region", R(F32, 100000, whole_frame=0, **large), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("off: an adaptive run", R(F32, 100000, adaptive=1, **large), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("off: f64", R(F64, 100000, **large), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("off: latency_entries = 0", R(F32, 100000, latency_entries=0), (TOP, 1, 0, 4096, 1, 131072, 0)),
        ("off: the guide pass (no whole frame, not adaptive)", R(F32, 2, whole_frame=0, **small), (TOP, 1, 0, 2, 1, 64, 0)),
    ])


def test_global_row(exes, tmp_path):
    none = dict(lds_top_bytes=0)
    check(exes, tmp_path, [
        ("screen", R(F64, 10000, **none), (GLOBAL, 1, 0, 0, 0, 0, 0)),
        ("no screen", R(F64, 10000, screen=0, **none), (GLOBAL, 0, 0, 0, 0, 0, 0)),
        ("ordered f64", R(F64_ORD, 10000, **none), (GLOBAL, 1, 0, 0, 0, 0, 0)),
        ("f32", R(F32, 10000, **none), (GLOBAL, 1, 0, 0, 0, 0, 0)),
        ("no SCREEN kernels, whatever w.screen says", R(F32_ORD, 10000, screen=1, **none), (GLOBAL, 0, 0, 0, 0, 0, 0)),
        ("the side tables do not matter", R(F64, 10000, side_bytes=64, **none), (GLOBAL, 1, 0, 0, 0, 0, 0)),
    ])


# bytes of a primitive, material and texture record (pathtrace.hpp Prim, Mat, Tex), per precision
REC64 = dict(prim_rec=96, mat_rec=48, tex_rec=48)
REC32 = dict(prim_rec=48, mat_rec=32, tex_rec=32)


def L(n_records, record_rec, n_prims, n_mats, n_texs, with_prims, with_side, prim_rec, mat_rec, tex_rec):
    return f"L {n_records} {record_rec} {n_prims} {prim_rec} {n_mats} {mat_rec} {n_texs} {tex_rec} {with_prims} {with_side}"


def test_layout(exes, tmp_path):
    """records | primitives | materials | textures, every table at a multiple of 16; `bytes` ends the last table staged."""
    ODD = dict(prim_rec=20, mat_rec=24, tex_rec=20)   # no record of the library: sizes that 16 does not divide
    check(exes, tmp_path, [
        # the whole scene (RES_LDS), 2 primitives, 2 materials, 1 texture behind the four trees' records
        ("f64 wrappers: 192 | 192 | 96 | 48", L(3, 64, 2, 2, 1, 1, 1, **REC64), (192, 384, 480, 528, 528)),
        ("f64 screening records: 96 | 192 | 96 | 48", L(3, 32, 2, 2, 1, 1, 1, **REC64), (96, 288, 384, 432, 432)),
        ("ordered f64 wrappers, one of each: 96 | 96 | 48 | 48", L(1, 96, 1, 1, 1, 1, 1, **REC64), (96, 192, 240, 288, 288)),
        ("ordered f64 screening records, one of each: 64 | 96 | 48 | 48", L(1, 64, 1, 1, 1, 1, 1, **REC64), (64, 160, 208, 256, 256)),
        ("f32: 96 | 96 | 64 | 32", L(3, 32, 2, 2, 1, 1, 1, **REC32), (96, 192, 256, 288, 288)),
        ("ordered f32: 192 | 96 | 64 | 32", L(3, 64, 2, 2, 1, 1, 1, **REC32), (192, 288, 352, 384, 384)),
        ("no records: the primitives at 0", L(0, 64, 2, 2, 1, 1, 1, **REC64), (0, 192, 288, 336, 336)),
        ("no tables behind one record", L(1, 64, 0, 0, 0, 1, 1, **REC64), (64, 64, 64, 64, 64)),
        # 3 x 40 = 120 -> 128; 3 x 20 = 60 -> 64; 24 -> 32; the last table ends at 224 + 20, unrounded, and end() rounds it
        ("every size rounded up to 16, the end only in end()", L(3, 40, 3, 1, 1, 1, 1, **ODD), (128, 192, 224, 244, 256)),
        # a window (RES_TOP): no primitives, whatever the scene has
        ("window of 25 screening records with 5 materials, 1 texture", L(25, 32, 100, 5, 1, 0, 1, **REC64), (800, 800, 1040, 1088, 1088)),
        ("window of 1000 bytes: rounded before the side tables follow", L(25, 40, 100, 1, 0, 0, 1, **REC32), (1008, 1008, 1040, 1040, 1040)),
        ("window alone: 1000 bytes, what follows it begins at 1008", L(25, 40, 100, 5, 1, 0, 0, **REC64), (1008, 1008, 1008, 1000, 1008)),
        ("window of no records, side tables at 0", L(0, 32, 100, 1, 1, 0, 1, **REC64), (0, 0, 48, 96, 96)),
        # geometry only (the wavefront extend kernel): materials and textures take no room
        ("geometry only", L(3, 64, 2, 5, 1, 1, 0, **REC64), (192, 384, 384, 384, 384)),
        ("geometry only, 60 bytes of primitives", L(3, 64, 3, 5, 1, 1, 0, **ODD), (192, 256, 256, 252, 256)),
    ])


def test_layout_keeps_a_scene_s_bytes(exes, tmp_path):
    """The two byte counts a handle derives from an uploaded scene, as they were computed before the layout existed -- the sum
    of every table rounded up to 16 --, for the counts of test_motion_boxes_host.py's keyed scene: 11 primitives (a binary tree
    over them has 21 wrappers), 5 materials, 1 texture.  DevScene::lds_bytes is end() over the wrappers, WalkChoice::
    lds_all_screen end() over the screening records.  The counts are multiplied here by the record sizes above and handed to
    scene_layout directly: handle.hpp's whole_scene_layout and scene_lds_bytes, which do that multiplication in the library,
    need the HIP runtime and are not compiled here -- a wrong record size or flag there shows in the GPU tests alone
    (test_gpu_variants.py, test_gpu_handle_memory.py)."""
    check(exes, tmp_path, [
        # f64: 21 x 64 = 1344, 11 x 96 = 1056, 5 x 48 = 240, 48: 2688; with 21 x 32 = 672 in the wrappers' place 2016
        ("f64 lds_bytes", L(21, 64, 11, 5, 1, 1, 1, **REC64), (1344, 2400, 2640, 2688, 2688)),
        ("f64 lds_all_screen", L(21, 32, 11, 5, 1, 1, 1, **REC64), (672, 1728, 1968, 2016, 2016)),
        # f32: 21 x 32 = 672, 11 x 48 = 528, 5 x 32 = 160, 32: 1392, and the same with its 32-byte screening records
        ("f32 lds_bytes and lds_all_screen", L(21, 32, 11, 5, 1, 1, 1, **REC32), (672, 1200, 1360, 1392, 1392)),
        # ordered trees: 21 x 96 = 2016 -> 3360, 21 x 64 = 1344 -> 2688 (f64); 21 x 64 = 1344 -> 2064 (f32)
        ("ordered f64 lds_bytes", L(21, 96, 11, 5, 1, 1, 1, **REC64), (2016, 3072, 3312, 3360, 3360)),
        ("ordered f64 lds_all_screen", L(21, 64, 11, 5, 1, 1, 1, **REC64), (1344, 2400, 2640, 2688, 2688)),
        ("ordered f32 lds_bytes", L(21, 64, 11, 5, 1, 1, 1, **REC32), (1344, 1872, 2032, 2064, 2064)),
    ])
