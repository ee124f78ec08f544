"""oracle_world_hit_counted: the closest-hit probe that also returns the ray's own node tests and primitive tests.

Held to the probe it stands beside (the same hit, the same record, bit for bit) and to the oracle's render: over the primary
rays of a depth-1 frame the per-ray counts add up to the frame's node_tests and prim_tests -- on the oracle's own tree and
on an exported CR_BVH_SAH_ORDERED tree (tests/tree_check.cpp's, built on the CPU) with its split axes, in f64 and f32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from crucible_amd import _abi as A
from test_gpu_variants import matrix_scene
from test_tree_host import parse_export, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]


@pytest.fixture(scope="module")
def tree_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_counted") / "tree_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "tree_check.cpp")])
    return exe


def exported_tree(exe, tmp_path, flat, rt, mode):
    """(boxes, children, split_axis) as cr_export_bvh returns them, from the host tree code alone."""
    write_scene(tmp_path / "in.bin", flat, rt, mode)
    res = subprocess.run([exe, "tree", str(tmp_path / "in.bin")], capture_output=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, res.stderr.decode()
    spliced, boxes, kids, axis, rest = parse_export(res.stdout.decode().splitlines())
    assert spliced == 0 and not rest and len(kids) > 0
    return boxes, kids, axis


def primary_rays(o, cam, seed):
    """oracle_camera_ray of every (pixel, sample) of the frame: rows of origin(3), direction(3), time."""
    cd = cam.desc()
    p = cam.params(seed, o.real_type, 0, None, 0, A.CR_SUM_DEFAULT)
    rays = np.zeros((cam.image_height, cam.image_width, cam.samples, 8), dtype=o.np_real)
    for j in range(cam.image_height):
        for i in range(cam.image_width):
            for s in range(cam.samples):
                o.lib.oracle_camera_ray(C.byref(cd), C.byref(p), i, j, s, o._p(rays[j, i, s]))
    return rays.reshape(-1, 8)[:, :7]


def extra_rays(rs, n=200):
    """Rays a camera does not make: from inside the scene outwards, past the scene, and along one or two axes."""
    rows = []
    for _ in range(n):
        o = np.array([rs.uniform(-5, 5), rs.uniform(0.05, 1.0), rs.uniform(-5, 4)])
        d = rs.normal(size=3)
        rows.append(np.concatenate([o, d, [0.0]]))
        rows.append(np.concatenate([[0.0, 500.0, 0.0], [rs.normal(), abs(rs.normal()) + 0.1, rs.normal()], [0.0]]))   # misses the root
        axis = rs.randint(3)
        d1 = np.zeros(3)
        d1[axis] = rs.choice([-1.0, 1.0])
        rows.append(np.concatenate([o, d1, [0.0]]))                         # two zero components
        d2 = rs.normal(size=3)
        d2[axis] = 0.0
        rows.append(np.concatenate([o, d2, [0.0]]))                         # one zero component
    return np.array(rows)


def probe_both(o, h, ray):
    """(plain probe's result, counted probe's result) for one ray on (0.001, inf)."""
    orig, dirn = o.arr(ray[0:3]), o.arr(ray[3:6])
    rec = np.zeros(10, dtype=o.np_real)
    mat = C.c_int32(-1)
    hit = o.lib.oracle_world_hit(h, o._p(orig), o._p(dirn), o.real(ray[6]), o.real(0.001), o.real(np.inf), o._p(rec), C.byref(mat))
    return (bool(hit), rec, mat.value), o.world_hit_counted(h, orig, dirn, ray[6])


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("ordered", [False, True], ids=["reference-tree", "exported-ordered-tree"])
@pytest.mark.parametrize("kind", ["static", "list"])
def test_counts_add_up_to_the_render_and_the_hit_is_the_plain_probe(oracles, tree_exe, tmp_path, kind, ordered, rt, tag):
    o = oracles[rt]
    sc = matrix_scene(kind)
    cam = sc.scene_cam
    cam.set_max_depth(1)
    if ordered:
        sc.bvh_mode = A.CR_BVH_SAH_ORDERED
    flat = sc.flatten()
    h = o.scene_create(flat)
    try:
        if ordered:
            boxes, kids, axis = exported_tree(tree_exe, tmp_path, flat, rt, A.CR_BVH_SAH_ORDERED)
            assert (axis >= 0).sum() == (len(kids) - 1) // 2   # every inner wrapper has its split axis
            o.set_tree(h, boxes, kids, axis)
        _, st = o.render(h, cam, seed=SEED)   # (also leaves the frame's boxes in the scene for the probes)
        rays = primary_rays(o, cam, SEED)
        assert st["segments"] == len(rays) == 24 * 16 * 3
        nodes = prims = hits = 0
        for ray in rays:
            (hit, rec, mat), (chit, crec, cmat, cn, cp) = probe_both(o, h, ray)
            assert chit == hit and (not hit or (cmat == mat and crec.tobytes() == rec.tobytes())), ray
            assert cn >= 1 and (cp > 0 or not hit)
            nodes, prims, hits = nodes + cn, prims + cp, hits + hit
        assert (nodes, prims) == (st["node_tests"], st["prim_tests"]), (nodes, prims, st["node_tests"], st["prim_tests"])
        assert 0 < hits < len(rays)
        # rays no camera makes: the same answer as the plain probe, and a ray that misses the root box costs one node test
        missed_root = 0
        for ray in extra_rays(np.random.RandomState(3)).astype(o.np_real):
            (hit, rec, mat), (chit, crec, cmat, cn, cp) = probe_both(o, h, ray)
            assert chit == hit and (not hit or (cmat == mat and crec.tobytes() == rec.tobytes())), ray
            missed_root += (cn, cp) == (1, 0)
        assert missed_root >= 200
    finally:
        o.scene_destroy(h)


def test_counted_probe_on_a_two_primitive_scene(o64):
    """The root is the only wrapper and a leaf: one node test; two primitive tests when its box is hit, none when it is missed."""
    from crucible_amd.scene import Lambertian, Scene, Sphere
    sc = Scene.new_image(1.0, 4, 1, 360.0, 1)
    sc.add_element(Sphere.new((-1.0, 0.0, 0.0), 0.5, Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)), "a")
    sc.add_element(Sphere.new((1.0, 0.0, 0.0), 0.5, Lambertian.new_from_color((0.2, 0.5, 0.5), 1.0)), "b")
    h = o64.scene_create(sc.flatten())
    try:
        hit, rec, mat, n, p = o64.world_hit_counted(h, (-1.0, 0.0, 5.0), (0.0, 0.0, -1.0))
        assert hit and mat == 0 and rec[0] == 4.5 and (n, p) == (1, 2)
        hit, _, _, n, p = o64.world_hit_counted(h, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
        assert not hit and (n, p) == (1, 2)
        hit, _, _, n, p = o64.world_hit_counted(h, (0.0, 3.0, 5.0), (0.0, 0.0, -1.0))
        assert not hit and (n, p) == (1, 0)
    finally:
        o64.scene_destroy(h)
