"""A render whose caller asks for no stats runs, where one exists, the kernel that keeps no work counters
(pathtrace.hpp pathtrace_kernel_quiet: the static f64 relaxed SCREEN kernel on an unordered tree with the scene in LDS;
render.hpp: launch_variant names it as that kernel's twin in the MegaKernel descriptor, launch() picks it).  The paths are the same paths, so the frame must be the counted render's bit for bit: every
case below renders f64 with relaxed sums twice, without and with a CrStats, and compares with np.array_equal -- through
the host entry point unless a case says otherwise.  The counted twin's scene_in_lds shows the residency the pair ran at."""
import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.renderer import Renderer
from crucible_amd.scene import Dielectric, Lambertian, Metal, Scene, Sphere, Triangle

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
F64, RELAX = A.CR_REAL_F64, A.CR_SUM_RELAXED
WINDOW = {"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "1"}   # a 1 KB window of the tree's top: RES_TOP (tests/test_gpu_variants.py)


def book1():
    return book1_end_scene(1, scene_seed=1, image_width=96, samples=8)


def pair(r, cam, **kw):
    """(frame, stats) of the counted render, after asserting that the render without stats wrote the same frame."""
    quiet, none = r.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=False, **kw)
    assert not any(none[k] for k in COUNTERS)   # a null CrStats: nothing was filled in
    counted, st = r.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=True, **kw)
    assert quiet.dtype == counted.dtype and quiet.shape == counted.shape
    assert np.array_equal(quiet, counted), f"differing px = {(quiet != counted).any(axis=-1).sum()}"
    assert st["segments"] > 0 and st["node_tests"] > 0 and st["prim_tests"] > 0
    return counted, st


@pytest.fixture(scope="module")
def book1_frame(renderer):
    """The counted frame and stats of book1 96 x 54 @ 8 spp on the session's renderer (default knobs: RES_LDS)."""
    sc = book1()
    assert (sc.scene_cam.image_width, sc.scene_cam.image_height) == (96, 54)
    renderer.upload_scene(sc.flatten())
    img, st = pair(renderer, sc.scene_cam)
    assert st["scene_in_lds"] == 1
    return img, st


def test_book1_in_lds(book1_frame, o64):
    """The headline's kernel at a small size: spheres alone (the spheres-only primitive loop), the whole scene in LDS."""
    img, st = book1_frame
    ref, rst = o64.render_image(book1(), seed=SEED, sum_order=RELAX)
    assert np.array_equal(img, ref)
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])


def test_spheres_and_triangles_with_two_primitive_leaves(renderer):
    """uniform_kind < 0: the general primitive loop, image textures and a spherical sky (texel fetches), leaves of two."""
    sc = scenes.mixed_scene(96, 8)
    renderer.upload_scene(sc.flatten())
    _, kids, _ = renderer.export_bvh(F64)
    leaves = (kids[:, 0] < 0) & (kids[:, 1] < 0)
    assert (kids[leaves, 0] != kids[leaves, 1]).any()   # (a leaf of one primitive names it twice)
    img, st = pair(renderer, sc.scene_cam)
    assert st["scene_in_lds"] == 1 and st["texel_fetches"] > 0


@pytest.mark.parametrize("build", [book1, lambda: scenes.mixed_scene(96, 8)], ids=["book1", "mixed"])
def test_tree_top_in_a_window(renderer, book1_frame, monkeypatch, build):
    """RES_TOP: a window of the tree's top in LDS, the rest and the primitives through L2.  The quiet twin of this kernel
    measured slower than the counted one on 1M spheres and is not built: its descriptor names no twin, so
    launch() must keep such a render on the counted kernel, stats or none, and the frame is the same."""
    for k, v in WINDOW.items():
        monkeypatch.setenv(k, v)
    sc = build()
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        img, st = pair(r, sc.scene_cam)
        assert st["scene_in_lds"] == 2
        if build is book1:
            assert np.array_equal(img, book1_frame[0]) and all(st[k] == book1_frame[1][k] for k in COUNTERS)
    finally:
        r.close()


@pytest.mark.parametrize("exit_lanes", ["1", "64"])
@pytest.mark.parametrize("steps", ["1", "3", "10"])
def test_walk_schedules(book1_frame, monkeypatch, steps, exit_lanes):
    """The round's budget is what the pinned scalar step count is compared with: short, odd and long rounds, leaving the
    walk with the first finished lane or the last.  A schedule changes neither frame nor counters."""
    monkeypatch.setenv("CRUCIBLE_WALK_ROUND", steps)
    monkeypatch.setenv("CRUCIBLE_WALK_EXIT", exit_lanes)
    sc = book1()
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        img, st = pair(r, sc.scene_cam)
        assert np.array_equal(img, book1_frame[0]) and all(st[k] == book1_frame[1][k] for k in COUNTERS)
    finally:
        r.close()


def test_shards_and_fixed_point_words(renderer, book1_frame):
    """output_sum shards of the samples and CR_OUTPUT_FIXED_SUM words: quiet equals counted shard by shard, and the words of
    the shards add up to the whole frame's."""
    sc = book1()
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    shards = ((0, 3), (3, 0), (3, 4), (7, 1))
    for s0, n in shards:
        part, st = (pair(renderer, cam, sample_begin=s0, sample_count=n, output_sum=True) if n else
                    renderer.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=False, sample_begin=s0, sample_count=n, output_sum=True))
        assert part.dtype == np.float64 and (n > 0 or not part.any())
    words = np.zeros((cam.image_height, cam.image_width, 3), dtype=np.uint64)
    for s0, n in shards:
        if n:
            w, _ = pair(renderer, cam, sample_begin=s0, sample_count=n, output_sum=A.CR_OUTPUT_FIXED_SUM)
            assert w.dtype == np.uint64
            words += w
    whole, _ = pair(renderer, cam, output_sum=A.CR_OUTPUT_FIXED_SUM)
    assert np.array_equal(words, whole)
    total, _ = pair(renderer, cam, output_sum=True)
    assert np.array_equal(total / 8.0, book1_frame[0])


def far_axis_scene():
    """A camera that looks exactly down -z (a polished metal wall with the normal (0, 0, 1) keeps a reflected ray's x and y:
    the axis-parallel frame a camera can make, tests/test_gpu_segment_setup.py metal_wall) in a scene scaled by 2^101:
    every origin has a component beyond the screen's range of 2^100, so every segment is outside screen_in_range and walks
    with Aabb::hit's compare/select form on the f64 records -- the unscreened path of the SCREEN kernels."""
    s = 2.0 ** 101
    sc = Scene.new_image(16.0 / 9.0, 32, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(8)
    cam.set_max_depth(50)
    cam.look_from((0.0, 0.0, 2.0 * s))
    cam.look_at((0.0, 0.0, -1.0 * s))
    cam.set_vfov(60.0)
    cam.set_focus_dist(3.0 * s)   # the pixel grid's distance: at the default 10 the grid would vanish in the origin's rounding
    wall = Metal.new((0.9, 0.9, 0.9), 0.0)
    sc.add_element(Triangle.new((-6.0 * s, -4.0 * s, -4.0 * s), (6.0 * s, -4.0 * s, -4.0 * s), (6.0 * s, 4.0 * s, -4.0 * s), wall), "wall_a")
    sc.add_element(Triangle.new((-6.0 * s, -4.0 * s, -4.0 * s), (6.0 * s, 4.0 * s, -4.0 * s), (-6.0 * s, 4.0 * s, -4.0 * s), wall), "wall_b")
    sc.add_element(Sphere.new((0.0, 0.0, -6.0 * s), 1.0 * s, Lambertian.new_from_color((0.2, 0.2, 0.8), 1.0)), "behind_wall")
    sc.add_element(Sphere.new((1.0 * s, 0.5 * s, 6.0 * s), 2.0 * s, Lambertian.new_from_color((0.8, 0.4, 0.2), 1.0)), "behind_camera")
    sc.add_element(Sphere.new((-2.0 * s, -1.0 * s, 0.0), 0.7 * s, Dielectric.new(1.5)), "glass")
    return sc


def test_axis_parallel_rays_outside_the_screens_range(renderer, o64):
    """The unscreened path.  Raw sums (output_sum): the check of the means is not this test's subject."""
    sc = far_axis_scene()
    renderer.upload_scene(sc.flatten())
    img, st = pair(renderer, sc.scene_cam, output_sum=True)
    assert st["scene_in_lds"] == 1
    ref, rst = o64.render_image(sc, seed=SEED, sum_order=RELAX, output_sum=True)
    assert np.array_equal(img, ref, equal_nan=True)
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert rst["prim_tests"] > 0 and rst["segments"] > 32 * 18 * 8   # paths that hit and scatter


def test_counted_render_after_a_quiet_one_counts_from_zero(o64):
    """A quiet launch neither clears nor writes the handle's counters: the counted call after it clears them itself, and its
    four counters are the oracle's -- on a handle whose first call ever was quiet, and again after a quiet call that follows
    a counted one."""
    sc = book1()
    ref, rst = o64.render_image(sc, seed=SEED, sum_order=RELAX)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        for _ in range(2):
            quiet, _ = r.render(sc.scene_cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=False)
            assert np.array_equal(quiet, ref)
            img, st = r.render(sc.scene_cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=True)
            assert np.array_equal(img, ref)
            for k in COUNTERS:
                assert st[k] == rst[k], (k, st[k], rst[k])
            assert st["samples"] == 96 * 54 * 8 and st["kernel_ms"] > 0
    finally:
        r.close()


def test_host_and_device_entry_points_with_and_without_stats(renderer, book1_frame):
    """cr_render_host with a CrStats and with none (book1_frame is that pair), and cr_render_device likewise: four calls,
    one frame.  The host call without stats still checks its means: nan_pixels has nowhere to go, the error would."""
    import torch
    sc = book1()
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    want = torch.from_numpy(book1_frame[0])
    for want_stats in (False, True):
        out = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda:0")
        st = renderer.render_device(cam, out.data_ptr(), seed=SEED, real_type=F64, sum_order=RELAX, want_stats=want_stats)
        ms = renderer.last_kernel_ms()   # waits for the launch; cr_last_kernel_ms works for a quiet launch as for a counted one
        assert ms > 0
        assert torch.equal(out.cpu(), want), want_stats
        if want_stats:
            assert all(st[k] == book1_frame[1][k] for k in COUNTERS) and st["nan_pixels"] == 0
        else:
            assert st is None
    img, st = renderer.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=True)
    assert np.array_equal(img, book1_frame[0]) and st["nan_pixels"] == 0
