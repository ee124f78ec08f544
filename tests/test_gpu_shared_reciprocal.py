"""Renders through the kernels that share Sphere::hit's reciprocal (sphere_quot / quot_form of crucible_amd/csrc/pathtrace.hpp), f64,
48 x 27 at 8 samples, depth 50: in the parity mode bit-equal to the oracle with its counters, with the library's relaxed sums the
same counters and a frame within 1e-12 of the parity frame -- under every residency of the scene (tree in LDS, its top in LDS, all
in global memory; the first two run the kernels with the shared reciprocal, the last and every keyed scene the ones that divide).
Scenes: a small book1-style scene with glass spheres (the second root: rays that leave a sphere from inside); the same spheres
seen by a camera at the origin whose focus distance is 2^-210, so that every primary ray has |d|^2 near 2^-419 -- below the range
the short quotient is proven for -- while the spheres stay where the f32 screening records can hold them (the kernel with the
shared reciprocal runs, and its guard must send those segments to the division); the whole scene scaled by 2^210 (|d|^2 near
2^427; box planes beyond f32, so the kernel without the screen renders it); and keyed spheres (the ANIM kernels).  The oracle's
first-hit model confirms on the CPU that the primary rays of the scaled cameras hit spheres.  The guide layers of the first scene
run too."""
import math

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import CheckerTexture, Dielectric, Lambertian, Metal, Scene, Sphere
from test_gpu_aov import model as aov_model
from test_gpu_aov import parity as aov_parity

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
F64 = A.CR_REAL_F64
REF, RELAX = A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_RELAXED
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
W, SPP, DEPTH = 48, 8, 50
RESIDENCIES = [({}, 1), ({"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "1"}, 2), ({"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "0"}, 0)]
RES_IDS = ["scene-in-lds", "tree-top-in-lds", "scene-in-global-memory"]


def book_scene(scale=1.0, focus=None):
    """The shape of book1's end scene, small: a checkered ground, a grid of small spheres of every material (a third of them
    glass), the three large ones -- the glass one with a bubble inside.  The camera stands at the origin (a focus distance far
    below 1 would be absorbed by any other position) and the spheres are placed around it; `scale` multiplies every length."""
    sc = Scene.new_image(16.0 / 9.0, W, 24, 180.0, 1)
    cam = sc.scene_cam
    assert (cam.image_width, cam.image_height) == (48, 27)
    cam.set_samples(SPP)
    cam.set_max_depth(DEPTH)
    cam.look_from((0.0, 0.0, 0.0))
    cam.look_at((-13.0 * scale, -2.0 * scale, -3.0 * scale))
    cam.set_vfov(20.0)
    cam.set_focus_dist(10.0 * scale if focus is None else focus)
    o = (-13.0, -2.0, -3.0)   # the world's origin as the camera sees it

    def at(x, y, z):
        return ((x + o[0]) * scale, (y + o[1]) * scale, (z + o[2]) * scale)

    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.32, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    sc.add_element(Sphere.new(at(0.0, -1000.0, 0.0), 1000.0 * scale, ground), "ground")
    rs = np.random.RandomState(4)
    k = 0
    for a in range(-3, 6):
        for b in range(-3, 4):
            c = (a + 0.9 * rs.rand(), 0.2, b + 0.9 * rs.rand())
            if math.dist(c, (4.0, 0.2, 0.0)) <= 0.9:
                continue
            mat = (Dielectric.new(1.5) if k % 3 == 0 else
                   Metal.new(tuple(0.5 + 0.5 * rs.rand(3)), 0.5 * rs.rand()) if k % 3 == 1 else Lambertian.new_from_color(tuple(rs.rand(3) * rs.rand(3)), 1.0))
            sc.add_element(Sphere.new(at(*c), 0.2 * scale, mat), f"small{k}")
            k += 1
    sc.add_element(Sphere.new(at(0.0, 1.0, 0.0), 1.0 * scale, Dielectric.new(1.5)), "large_dielectric")
    sc.add_element(Sphere.new(at(0.0, 1.0, 0.0), 0.7 * scale, Dielectric.new(1.0 / 1.5)), "bubble")
    sc.add_element(Sphere.new(at(-4.0, 1.0, 0.0), 1.0 * scale, Lambertian.new_from_color((0.4, 0.2, 0.1), 1.0)), "large_lambertian")
    sc.add_element(Sphere.new(at(4.0, 1.0, 0.0), 1.0 * scale, Metal.new((0.7, 0.6, 0.5), 0.0)), "large_metal")
    return sc


SCENES = {
    "book": lambda: book_scene(),
    "tiny-directions": lambda: book_scene(focus=2.0 ** -210),
    "huge-scene": lambda: book_scene(scale=2.0 ** 210),
    "keyed-spheres": lambda: scenes.moving_scene(width=W, samples=SPP, frame=0, depth=DEPTH),
}
_WANT = {}


def want(oracles, name):
    """The oracle's parity frame and counters, computed once per scene and shared by the residencies."""
    if name not in _WANT:
        img, st = oracles[F64].render_image(SCENES[name](), seed=SEED, sum_order=REF)
        img.setflags(write=False)
        _WANT[name] = (img, st)
    return _WANT[name]


@pytest.mark.parametrize("name,least", [("tiny-directions", 0.5), ("huge-scene", 0.5), ("book", 0.5)])
def test_the_primary_rays_of_the_scaled_cameras_hit_spheres(oracles, name, least):
    """On the CPU: the oracle's first-hit model, one sample per pixel.  The ground alone fills more than half of the frame."""
    sc = SCENES[name]()
    sc.scene_cam.set_samples(1)
    layers, _ = aov_model(oracles[F64], sc, SEED)
    cover = float(layers["coverage"].mean())
    print(f"\n[shared reciprocal] {name}: {cover:.3f} of the primary rays hit a sphere")
    assert cover >= least


@pytest.mark.parametrize("env,res", RESIDENCIES, ids=RES_IDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_parity_and_library_defaults(monkeypatch, oracles, name, env, res):
    sc = SCENES[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref, rst = want(oracles, name)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        img, st = r.render(sc.scene_cam, seed=SEED, real_type=F64, sum_order=REF)
        assert st["scene_in_lds"] == res
        assert np.array_equal(img, ref), f"parity mode: {(img != ref).any(axis=-1).sum()} pixels differ from the oracle"
        fast, fst = r.render(sc.scene_cam, seed=SEED, real_type=F64, sum_order=RELAX)
        assert fst["scene_in_lds"] == res
        worst = float(np.abs(fast - ref).max())
        print(f"\n[shared reciprocal] {name}, residency {res}: relaxed sums within {worst:.3g} of the parity frame")
        assert worst <= 1e-12
        for s in (st, fst):
            assert s["samples"] == 48 * 27 * SPP and s["nan_pixels"] == 0
            for k in COUNTERS:
                assert s[k] == rst[k], (k, s[k], rst[k])
        assert st["prim_tests"] > st["segments"] > st["samples"]
    finally:
        r.close()


def test_guide_layers_of_the_book_scene(renderer, oracles):
    got, st = aov_parity(renderer, oracles, SCENES["book"](), F64)
    assert 0.5 <= got["coverage"].mean() <= 1.0
