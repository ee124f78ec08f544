"""Every megakernel variant render_typed (crucible_amd/csrc/render.hip) and its walk_ladder (render.hpp) can select, in both sum orders, bit for bit against
the oracle in the same order: images and work counters.

A kernel is pathtrace_kernel<real, RES, ANIM, ORD, CAMK, RELAX, SCREEN> (or the 6-waves-per-SIMD entry point,
LATENCY).  The handle's knobs pick RES / SCREEN / LATENCY (they are read in cr_create, so every cell makes a fresh
Renderer), the scene picks ANIM / CAMK, CrRenderParams.sum_order picks RELAX and the tree mode picks ORD.  SELECTIONS
below has one row per launch_variant selection of walk_ladder (10 per tree order; launch_variant describes the kernel to the
unit's one launch<real, RELAX> as a MegaKernel: address, RES, keys, LATENCY); CELLS crosses them with the scene kinds and
the two orders.  The relaxed ANIM / CAMK cells also render a 3-frame batch (cr_render_frames_host), each frame against
the relaxed oracle."""
import collections

import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import (LERP, LOCAL, WORLD, CheckerTexture, Dielectric, HitList, Lambertian, Metal, Scene, Sphere,
                                Triangle)

pytestmark = pytest.mark.gpu

SEED = 0x5EED
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
F64, F32 = A.CR_REAL_F64, A.CR_REAL_F32
REF, RELAX = A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_RELAXED
RES_GLOBAL, RES_LDS, RES_TOP = "GLOBAL", "LDS", "TOP"
IN_LDS = {RES_GLOBAL: 0, RES_LDS: 1, RES_TOP: 2}   # CrStats.scene_in_lds of each residency

# the residencies: the whole scene in LDS (default); a 1 KB window of the tree's top (16 to 32 records) with the rest in
# global memory; everything in global memory
WINDOW = {"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "1"}
GLOBAL = {"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "0"}
LATENCY6 = {"CRUCIBLE_LATENCY_ENTRIES": "1", "CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LATENCY_TOP_KB": "1"}
NO_SCREEN = {"CRUCIBLE_SCREEN": "0"}

Sel = collections.namedtuple("Sel", "name real res ord latency screen env")


def _selections(ordered):
    """The launch_variant calls of one tree order.  f64 walks on its f32 screening records unless CRUCIBLE_SCREEN=0 (at LDS
    residency CRUCIBLE_SCREEN_LDS=0 stages the wrappers instead); the unordered f32 tree's walk also runs the SCREEN
    kernels (its link-layout records), the ordered f32 walk never does."""
    o = "ord" if ordered else "ref"
    return [
        Sel(f"{o}-f64-lds-screen", F64, RES_LDS, ordered, False, True, {}),
        Sel(f"{o}-f64-lds", F64, RES_LDS, ordered, False, False, {"CRUCIBLE_SCREEN_LDS": "0"}),
        Sel(f"{o}-f64-top-screen", F64, RES_TOP, ordered, False, True, dict(WINDOW)),
        Sel(f"{o}-f64-top", F64, RES_TOP, ordered, False, False, dict(WINDOW, **NO_SCREEN)),
        Sel(f"{o}-f64-global-screen", F64, RES_GLOBAL, ordered, False, True, dict(GLOBAL)),
        Sel(f"{o}-f64-global", F64, RES_GLOBAL, ordered, False, False, dict(GLOBAL, **NO_SCREEN)),
        Sel(f"{o}-f32-lds", F32, RES_LDS, ordered, False, not ordered, {}),
        Sel(f"{o}-f32-top", F32, RES_TOP, ordered, False, not ordered, dict(WINDOW)),
        Sel(f"{o}-f32-top-latency", F32, RES_TOP, ordered, True, False, dict(LATENCY6)),
        Sel(f"{o}-f32-global", F32, RES_GLOBAL, ordered, False, not ordered, dict(GLOBAL)),
    ]


SELECTIONS = _selections(False) + _selections(True)

# Further selections: the f64 LDS kernel without the screen reached through CRUCIBLE_SCREEN=0; the unordered f32 walk
# without its SCREEN kernels; RES_TOP with the materials and textures in global memory (CRUCIBLE_LDS_SIDE_KB=0)
EXTRA_SELECTIONS = [
    Sel("ref-f64-lds-screen-off", F64, RES_LDS, False, False, False, dict(NO_SCREEN)),
    Sel("ref-f32-lds-noscreen", F32, RES_LDS, False, False, False, dict(NO_SCREEN)),
    Sel("ref-f32-top-noscreen", F32, RES_TOP, False, False, False, dict(WINDOW, **NO_SCREEN)),
    Sel("ref-f32-global-noscreen", F32, RES_GLOBAL, False, False, False, dict(GLOBAL, **NO_SCREEN)),
    Sel("ref-f64-top-screen-side-global", F64, RES_TOP, False, False, True, dict(WINDOW, CRUCIBLE_LDS_SIDE_KB="0")),
    Sel("ref-f64-top-side-global", F64, RES_TOP, False, False, False, dict(WINDOW, CRUCIBLE_LDS_SIDE_KB="0", **NO_SCREEN)),
    Sel("ref-f32-top-side-global", F32, RES_TOP, False, False, True, dict(WINDOW, CRUCIBLE_LDS_SIDE_KB="0")),
    Sel("ord-f64-top-side-global", F64, RES_TOP, True, False, True, dict(WINDOW, CRUCIBLE_LDS_SIDE_KB="0")),
]

# The scene kinds and the kernel flag each selects.  A HitList element reaches the ANIM kernels through its leaf runs on
# the reference tree; on the SAH tree its objects are leaves of the tree themselves, so it runs the static kernel there.
KINDS = ["static", "camk", "anim", "list"]


def kernel_kind(kind, ordered):
    if kind == "list":
        return "static" if ordered else "ANIM"
    return {"static": "static", "camk": "CAMK", "anim": "ANIM"}[kind]


# one cell: (real, RES, ORD, LATENCY, SCREEN, kind, RELAX), the environment that selects it, the scene that makes the
# kind and the CrStats.scene_in_lds it must report
Cell = collections.namedtuple("Cell", "id real res ord latency screen kind relax env scene scene_in_lds")
CELLS = [Cell(f"{s.name}-{scene}-{'relaxed' if order == RELAX else 'reference'}", s.real, s.res, s.ord, s.latency, s.screen,
              kernel_kind(scene, s.ord), order == RELAX, s.env, scene, IN_LDS[s.res])
         for s in SELECTIONS + EXTRA_SELECTIONS for scene in KINDS for order in (REF, RELAX)]


def matrix_scene(kind, width=24, samples=3):
    """24x16 at 3 spp, depth 8: a ground, 180 small spheres and 24 triangles in all three materials (a few hundred
    wrappers, so a 1 KB window holds only the top of the tree).  camk: a keyed camera; anim: keyed spheres; list: a
    HitList element of twelve spheres among the others.  1 fps with a 360 degree shutter: frame f's rays are in [f, f+1]."""
    sc = Scene.new_image(1.5, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(8)
    cam.look_from((0.0, 4.0, 11.0))
    cam.look_at((0.0, 0.4, 0.0))
    cam.set_vfov(42.0)
    rs = np.random.RandomState(77)
    mats = [Lambertian.new_from_color((0.8, 0.3, 0.2), 1.0), Metal.new((0.8, 0.8, 0.9), 0.1), Dielectric.new(1.5),
            Lambertian.new_from_texture(CheckerTexture.new_from_color(0.3, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9)), 0.8),
            Metal.new((0.9, 0.7, 0.3), 0.0)]
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, mats[3]), "ground")
    listed = HitList.default()
    for k in range(180):
        x, z = -6.0 + 12.0 * rs.rand(), -6.0 + 10.0 * rs.rand()
        r = 0.12 + 0.2 * rs.rand()
        s = Sphere.new((x, r, z), r, mats[k % len(mats)])
        if kind == "list" and k < 12:
            listed.add(s)
        else:
            sc.add_element(s, f"s{k}")
    for k in range(24):
        x, z = -5.0 + 10.0 * rs.rand(), -5.0 + 8.0 * rs.rand()
        sc.add_element(Triangle.new((x, 0.0, z), (x + 0.5, 0.0, z + 0.1), (x + 0.2, 0.6, z - 0.1), mats[(k + 1) % len(mats)]),
                       f"t{k}")
    if kind == "list":
        sc.add_element(listed, "listed")
    if kind == "camk":
        sc.cam_translate_point((1.5, 0.5, -1.0), 1.0, LERP, WORLD, "from")
        sc.cam_translate_point((0.3, 0.0, 0.0), 2.0, LERP, WORLD, "at")
    if kind == "anim":
        sc.translate_point((0.0, 0.8, 0.0), 1.0, LERP, LOCAL, "s20")
        sc.translate_point((1.0, 0.0, 0.5), 2.0, LERP, LOCAL, "s21")
        sc.scale_r(0.5, 1.5, LERP, "s22")
    return sc


def same(img, st, ref, rst, what=""):
    assert img.dtype == ref.dtype and img.shape == ref.shape
    assert np.array_equal(img, ref), f"{what}: differing px = {(img != ref).any(axis=-1).sum()}"
    for k in COUNTERS:
        assert st[k] == rst[k], (what, k, st[k], rst[k])


def render_cell(monkeypatch, oracles, env, sc, rt, order, ordered, scene_in_lds, batch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED if ordered else A.CR_BVH_REFERENCE
    r = Renderer(0)   # the knobs are read in cr_create
    try:
        r.upload_scene(sc.flatten())
        img, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=order)
        assert st["scene_in_lds"] == scene_in_lds, st["scene_in_lds"]
        tree = r.export_bvh(rt) if ordered else None   # the ordered walk: the oracle walks the exported tree and its axes
        ref, rst = oracles[rt].render_image(sc, seed=SEED, tree=tree, sum_order=order)
        same(img, st, ref, rst, "single render")
        if batch:
            frames = [0, 1, 2]
            got, bst = r.render_frames(sc.scene_cam, frames, seed=SEED, real_type=rt, sum_order=order)
            cam = sc.scene_cam
            tot = {k: 0 for k in COUNTERS}
            try:
                for k, f in enumerate(frames):
                    cam.frame = f
                    want, wst = oracles[rt].render_image(sc, seed=SEED, tree=tree, sum_order=order)
                    assert np.array_equal(got[k], want), f"frame {f}: differing px = {(got[k] != want).any(axis=-1).sum()}"
                    for c in COUNTERS:
                        tot[c] += wst[c]
            finally:
                cam.frame = 0
            for c in COUNTERS:
                assert bst[c] == tot[c], (c, bst[c], tot[c])
            assert bst["scene_in_lds"] == scene_in_lds
        return st
    finally:
        r.close()


def test_the_table_covers_every_selection():
    """20 selections (10 per tree order) x 4 scene kinds x 2 orders, and every kernel flag of the table occurs."""
    assert len(SELECTIONS) == 20 and len({s.name for s in SELECTIONS}) == 20
    assert len({(s.real, s.res, s.ord, s.latency, s.screen) for s in SELECTIONS}) == 20
    assert len(CELLS) == (20 + len(EXTRA_SELECTIONS)) * 4 * 2 and len({c.id for c in CELLS}) == len(CELLS)
    assert {c.kind for c in CELLS} == {"static", "CAMK", "ANIM"} and {c.relax for c in CELLS} == {False, True}


@pytest.mark.parametrize("cell", CELLS, ids=[c.id for c in CELLS])
def test_kernel_variant_bit_exact(monkeypatch, oracles, cell):
    sc = matrix_scene(cell.scene)
    batch = cell.relax and cell.kind in ("ANIM", "CAMK")
    render_cell(monkeypatch, oracles, cell.env, sc, cell.real, RELAX if cell.relax else REF, cell.ord, cell.scene_in_lds,
                batch)


def fallback_scene():
    """About 5000 spheres (some 5000 wrappers: their 32-byte screening records fill the default 128 KB window, 4096 of
    them) seen at 8x6 pixels and 1 sample per pixel."""
    sc = Scene.new_image(8.0 / 6.0, 8, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(1)
    cam.set_max_depth(6)
    cam.look_from((0.0, 6.0, 14.0))
    cam.look_at((0.0, 0.0, 0.0))
    cam.set_vfov(50.0)
    rs = np.random.RandomState(5)
    mats = [Lambertian.new_from_color((0.7, 0.5, 0.3), 1.0), Metal.new((0.8, 0.8, 0.8), 0.2), Dielectric.new(1.5)]
    for k in range(5000):
        c = (-8.0 + 16.0 * rs.rand(), -2.0 + 4.0 * rs.rand(), -8.0 + 16.0 * rs.rand())
        sc.add_element(Sphere.new(c, 0.05 + 0.1 * rs.rand(), mats[k % 3]), f"s{k}")
    return sc


@pytest.mark.parametrize("rt,tag", [(F64, "f64"), (F32, "f32")], ids=["f64", "f32"])
@pytest.mark.parametrize("order", [RELAX, REF], ids=["relaxed", "reference"])
def test_relaxed_two_by_two_tile_fallback(monkeypatch, oracles, rt, tag, order):
    """launch(): at 1 sample per pixel the work tile is 8x8 pixels, and a 1024-thread group's relaxed accumulator slots
    (16 waves x 2 slots x 64 pixels x 3 words x 8 bytes = 48 KB) do not fit beside a full 128 KB tree window in 160 KB,
    so the relaxed kernels fall back to 2x2-pixel tiles (the surplus sample slots of their groups stay empty).  The
    reference order, which has no slots, runs the same scene as a control."""
    sc = fallback_scene()
    st = render_cell(monkeypatch, oracles, {}, sc, rt, order, False, IN_LDS[RES_TOP], False)
    assert st["bvh_entries"] * 32 >= 128 * 1024   # the window is full whatever the record (32 bytes at the least)
