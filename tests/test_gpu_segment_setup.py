"""The f64 render kernels' segment set-up through the ABI (pathtrace.hpp walk_begin_screened, walk_round's LAZY_INV and
SPHERE_LOOP, shade's reuse of WalkState::dd): small frames of scenes that take each of the paths -- spheres alone (the
spheres-only primitive loop), spheres and triangles (the general loop), triangles alone, and a camera that looks exactly down
-z at a polished metal wall -- at 32 x 18, 8 spp, depth 50, f64.  In CR_SUM_REFERENCE_ORDER the frame is the oracle's bit for
bit with equal counters; in the library's default order (CR_SUM_RELAXED) it is within 1e-12 of it with equal counters."""
import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.scene import CheckerTexture, Dielectric, Lambertian, Metal, Scene, Sphere, Triangle

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")


def _frame(look_from, look_at, vfov=35.0, defocus=0.0):
    sc = Scene.new_image(16.0 / 9.0, 32, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(8)
    cam.set_max_depth(50)
    cam.look_from(look_from)
    cam.look_at(look_at)
    cam.set_vfov(vfov)
    if defocus:
        cam.set_defocus_angle(defocus)
        cam.set_focus_dist(10.0)
    return sc


def book48():
    """48 spheres in the book's manner: a checker ground, three large spheres, small ones of all three materials."""
    rs = np.random.RandomState(48)
    sc = _frame((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, defocus=0.6)
    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.32, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    sc.add_element(Sphere.new((0.0, -1000.0, 0.0), 1000.0, ground), "ground")
    sc.add_element(Sphere.new((0.0, 1.0, 0.0), 1.0, Dielectric.new(1.5)), "glass")
    sc.add_element(Sphere.new((-4.0, 1.0, 0.0), 1.0, Lambertian.new_from_color((0.4, 0.2, 0.1), 1.0)), "matte")
    sc.add_element(Sphere.new((4.0, 1.0, 0.0), 1.0, Metal.new((0.7, 0.6, 0.5), 0.0)), "mirror")
    for k in range(44):
        c = (rs.uniform(-6, 6), 0.2, rs.uniform(-4, 4))
        pick = k % 3
        mat = (Lambertian.new_from_color(tuple(rs.uniform(0, 1, 3) * rs.uniform(0, 1, 3)), 1.0) if pick == 0 else
               Metal.new(tuple(rs.uniform(0.5, 1, 3)), float(rs.uniform(0, 0.5))) if pick == 1 else Dielectric.new(1.5))
        sc.add_element(Sphere.new(c, 0.2, mat), f"s{k}")
    return sc


def _tetrahedra(sc, n, seed, mats):
    rs = np.random.RandomState(seed)
    for k in range(n):
        o = np.array([rs.uniform(-3, 3), rs.uniform(0.0, 1.5), rs.uniform(-3, 3)])
        p = [tuple(o + rs.uniform(-0.6, 0.6, 3)) for _ in range(4)]
        for j, (a, b, c) in enumerate([(0, 1, 3), (1, 2, 3), (2, 0, 3), (0, 2, 1)]):
            sc.add_element(Triangle.new(p[a], p[b], p[c], mats[(k + j) % len(mats)]), f"t{k}_{j}")


def _mats():
    return [Lambertian.new_from_color((0.8, 0.3, 0.3), 1.0), Metal.new((0.8, 0.8, 0.8), 0.1), Dielectric.new(1.5),
            Lambertian.new_from_texture(CheckerTexture.new_from_color(0.5, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9)), 1.0)]


def spheres_and_triangles():
    sc = _frame((6.0, 2.5, 5.0), (0.0, 0.6, 0.0))
    mats = _mats()
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, mats[3]), "ground")
    for k in range(6):
        sc.add_element(Sphere.new((k - 2.5, 0.5, 0.3 * k), 0.45, mats[k % 3]), f"s{k}")
    _tetrahedra(sc, 5, 7, mats)
    return sc


def triangles_only():
    sc = _frame((6.0, 2.5, 5.0), (0.0, 0.6, 0.0))
    mats = _mats()
    sc.add_element(Triangle.new((-8.0, 0.0, -8.0), (8.0, 0.0, 8.0), (8.0, -0.5, -8.0), mats[3]), "floor_a")
    sc.add_element(Triangle.new((-8.0, 0.0, -8.0), (-8.0, -0.5, 8.0), (8.0, 0.0, 8.0), mats[3]), "floor_b")
    _tetrahedra(sc, 8, 9, mats)
    return sc


def metal_wall():
    """The camera looks exactly down -z, defocus off, at a wall of polished metal (fuzz 0) in the plane z = -4: the wall's
    normal is (0, 0, 1) exactly and a reflected ray keeps its x and y.  Every sample is jittered inside its pixel, so no ray of
    this frame has an exactly zero component -- a frame through the ABI cannot ask for one; tests/test_gpu_walk_lazy.py walks
    600 rays with one and two exact zeros (and subnormal and 2^+-105 components) through the same code ray by ray.  This frame
    is the axis-aligned case nearest to it that a camera makes.  A matte sphere behind the camera is what the reflections see."""
    sc = _frame((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), 60.0)
    wall = Metal.new((0.9, 0.9, 0.9), 0.0)
    sc.add_element(Triangle.new((-6.0, -4.0, -4.0), (6.0, -4.0, -4.0), (6.0, 4.0, -4.0), wall), "wall_a")
    sc.add_element(Triangle.new((-6.0, -4.0, -4.0), (6.0, 4.0, -4.0), (-6.0, 4.0, -4.0), wall), "wall_b")
    sc.add_element(Sphere.new((0.0, 0.0, -6.0), 1.0, Lambertian.new_from_color((0.2, 0.2, 0.8), 1.0)), "behind_wall")   # gives the wall's leaves depth
    sc.add_element(Sphere.new((1.0, 0.5, 6.0), 2.0, Lambertian.new_from_color((0.8, 0.4, 0.2), 1.0)), "behind_camera")
    sc.add_element(Sphere.new((-2.0, -1.0, 0.0), 0.7, Dielectric.new(1.5)), "glass")
    return sc


SCENES = {"book48": book48, "spheres-and-triangles": spheres_and_triangles, "triangles-only": triangles_only, "metal-wall": metal_wall}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_segment_setup_frames_are_the_oracles(renderer, o64, name):
    sc = SCENES[name]()
    cam = sc.scene_cam
    assert (cam.image_width, cam.image_height) == (32, 18)
    renderer.upload_scene(sc.flatten())
    ref, rst = o64.render_image(sc, seed=SEED)
    img, st = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_REFERENCE_ORDER)
    assert np.array_equal(img, ref, equal_nan=True), f"differing px = {(img != ref).any(axis=-1).sum()}, max {np.abs(img - ref).max()}"
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert rst["prim_tests"] > 0 and rst["segments"] > 32 * 18 * 8   # paths that hit and scatter
    fast, fst = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)
    d = np.abs(fast - ref).max()
    print(f"\n[segment setup] {name}: {rst['segments']} segments, {rst['node_tests']} box tests, {rst['prim_tests']} primitive tests; "
          f"default order within {d:.3g}")
    assert d <= 1e-12, d
    for k in COUNTERS:
        assert fst[k] == rst[k], (k, fst[k], rst[k])
