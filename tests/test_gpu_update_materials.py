"""cr_update_materials on the device: the material and texture tables and the primitives' material indices of an uploaded
scene edited in place (include/crucible_hip.h).

The yardstick of every case is a FRESH handle that received cr_upload_scene of the edited description (shading_model.fresh):
output bytes, the four work counters, samples, bvh_entries and scene_in_lds are equal -- for the render in the suite's
reference order and with CR_SUM_RELAXED named, the guide pass's four layers, a region and an adaptive frame with its counts,
in f64 and f32.  Frames are 24 x 16 to 37 x 29 pixels at 4 to 8 samples."""
import ctypes as C
import struct

import numpy as np
import pytest

import scenes
import shading_model as sm
import update_model as um
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.group import RenderGroup
from crucible_amd.renderer import CrucibleError, Renderer
from shading_model import F32, F64, REALS

pytestmark = pytest.mark.gpu

L, M, D = A.CR_MAT_LAMBERTIAN, A.CR_MAT_METAL, A.CR_MAT_DIELECTRIC


@pytest.fixture
def r(hiplib):
    handle = Renderer(0)
    yield handle
    handle.close()


def first_material(p, kind, tex_kind=None):
    for i, m in enumerate(p["materials"]):
        if m.kind == kind and (tex_kind is None or p["textures"][m.texture].kind == tex_kind):
            return i
    raise AssertionError((kind, tex_kind))


def same_as_fresh(r, flat, cam, rt, what=sm.families):
    got, want = what(r, cam, rt), sm.fresh(flat, what, cam, rt)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k
    return got


# ---------------------------------------------------------------- 1. every family, every kind of edit
def edit_solid_colour(p):
    t = p["textures"][p["materials"][first_material(p, L, A.CR_TEX_SOLID)].texture]
    t.color[0], t.color[1], t.color[2] = 0.9, 0.4, 0.1
    return False, True


def edit_lambertian_param(p):
    p["materials"][first_material(p, L, A.CR_TEX_SOLID)].param = 0.35
    return True, False


def edit_metal(p):
    m = p["materials"][first_material(p, M)]
    m.param = 0.45
    m.albedo[0], m.albedo[1], m.albedo[2] = 0.3, 0.9, 0.5
    return True, False


def edit_dielectric(p):
    p["materials"][first_material(p, D)].param = 1.33
    return True, False


def edit_kind(p):
    i, j = first_material(p, M), first_material(p, L, A.CR_TEX_SOLID)
    p["materials"][i] = sm.dielectric(1.7)
    p["materials"][j] = sm.metal((0.9, 0.8, 0.2), 0.05)      # its solid texture is dead from here on
    return True, False


def edit_checker(p):
    top = max(i for i, t in enumerate(p["textures"]) if t.kind == A.CR_TEX_CHECKER)
    image = next(i for i, t in enumerate(p["textures"]) if t.kind == A.CR_TEX_IMAGE and i < top)
    p["textures"][top] = sm.checker(0.9, image, 1)            # another scale, other children: an image behind it
    return False, True


EDITS = {"solid_colour": edit_solid_colour, "lambertian_param": edit_lambertian_param, "metal": edit_metal, "dielectric": edit_dielectric,
         "kind": edit_kind, "checker": edit_checker}


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(EDITS))
def test_every_family_after_every_kind_of_edit(r, rt, tag, name):
    sc = scenes.mixed_scene(37, 4)
    flat = sc.flatten()
    cam = sm.camera(sc, (37, 29), 4, 8)
    p = sm.parts_of(flat)
    mats, texs = EDITS[name](p)
    after = sm.flat_of(p)
    r.upload_scene(flat)
    before = sm.families(r, cam, rt)
    r.update_materials(p["materials"] if mats else None, p["textures"] if texs else None)   # the other table stays
    got = same_as_fresh(r, after, cam, rt)
    assert got["relaxed"][0] != before["relaxed"][0]                                          # the edit shows
    if name in ("solid_colour", "metal"):
        assert got["aov"][0] != before["aov"][0]                                              # in the albedo layer too: the guide pass reads Mat


# ---------------------------------------------------------------- 2. table sizes and residency
def r16(n):
    return (n + 15) & ~15


# Mat<real>: albedo[3], param, kind, tex, aux; Tex<real>: color[3], inv_scale, kind, even, odd, image; both alignas(16)
MAT_BYTES = {F64: r16(struct.calcsize("<4d2id")), F32: r16(struct.calcsize("<4f2if"))}
TEX_BYTES = {F64: r16(struct.calcsize("<4d4i")), F32: r16(struct.calcsize("<4f4i"))}
LDS_SIDE_LIMIT, LDS_BYTES = 16 * 1024, 160 * 1024


def side_bytes(rt, n_mats, n_texs):
    return r16(n_mats * MAT_BYTES[rt]) + r16(n_texs * TEX_BYTES[rt])


def padded(materials, n):
    """The table grown to n records with metals no primitive names"""
    return [sm.rec(m) for m in materials] + [sm.metal((0.5, 0.25 + 0.5 * (k % 2), 0.5), 0.1) for k in range(n - len(materials))]


def both_orders(r, cam, rt):
    return {"reference": sm.frame(r, cam, rt, A.CR_SUM_REFERENCE_ORDER), "relaxed": sm.frame(r, cam, rt, A.CR_SUM_RELAXED)}


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_side_tables_cross_the_window_limit_and_come_back(r, rt, tag):
    """A tree too large for the LDS (its top sits in a window): the side tables join the window up to lds_side_limit.  The
    table grows to the last count that fits, to the first that does not, and shrinks to the short one again."""
    n = 6000
    g = np.arange(n)
    sc = scenes.sah_spheres(np.stack([(g % 20) * 1.0 - 10.0, ((g // 20) % 20) * 1.0 - 10.0, -(g // 400) * 1.0 - 4.0], axis=1), np.full(n, 0.4))
    sc.bvh_mode = A.CR_BVH_SAH
    sc.scene_cam.look_from((3.0, 5.0, 14.0))
    sc.scene_cam.look_at((0.0, 0.0, -8.0))
    sc.scene_cam.set_vfov(45.0)
    flat = sc.flatten()
    cam = sm.camera(sc, (32, 24), 4, 6)
    short =sm.parts_of(flat)["materials"]
    n_texs = 0          # the one Lambertian's texture is solid: folded into its material
    at_limit = max(k for k in range(1, LDS_SIDE_LIMIT // MAT_BYTES[rt] + 2) if side_bytes(rt, k, n_texs) <= LDS_SIDE_LIMIT)
    assert side_bytes(rt, at_limit, n_texs) <= LDS_SIDE_LIMIT < side_bytes(rt, at_limit + 1, n_texs) and at_limit > len(short)
    r.upload_scene(flat)
    first = both_orders(r, cam, rt)
    assert first["relaxed"][1][sm.COUNTERS.index("bvh_entries")] * 32 > LDS_BYTES      # not in LDS whole, whatever the record
    for count in (at_limit, at_limit + 1, len(short)):
        table = padded(short, count)
        r.update_materials(table)
        got = same_as_fresh(r, sm.edited(flat, materials=table), cam, rt, both_orders)
        assert got == first                                                            # the added records are never read


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_a_growing_table_pushes_the_scene_out_of_lds_and_back(r, rt, tag):
    sc = scenes.few_spheres(5, 24, 4)
    flat = sc.flatten()
    cam = sm.camera(sc, (24, 16), 4, 8)
    short = sm.parts_of(flat)["materials"]
    long_count = LDS_BYTES // MAT_BYTES[rt] + 1       # the materials alone no longer fit
    r.upload_scene(flat)
    seen = []
    for count in (len(short), long_count, len(short)):
        table = padded(short, count)
        r.update_materials(table)
        got = same_as_fresh(r, sm.edited(flat, materials=table), cam, rt, both_orders)
        seen.append(got["relaxed"][1][sm.COUNTERS.index("scene_in_lds")])
    assert seen[0] == seen[2] != seen[1], seen


# ---------------------------------------------------------------- 3. texture remap
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_a_dead_checker_becomes_live_and_goes_back_to_solid(r, rt, tag):
    """The device texture table changes size under the edit: 0 live textures, then a checker with a solid and an image
    texture behind it, then none again.  texel_fetches is among the counters compared."""
    sc = scenes.few_spheres(5, 37, 4)
    cam = sm.camera(sc, (37, 29), 4, 8)
    p = sm.parts_of(sc.flatten())
    p["images"].append(sm.seeded_image(64, 32, 5))
    ground = first_material(p, L, A.CR_TEX_SOLID)
    solid_tex = p["materials"][ground].texture
    p["textures"] += [sm.image_texture(0), sm.checker(3.0, solid_tex, len(p["textures"]))]   # no material names them: dead
    dead_checker = len(p["textures"]) - 1
    flat = sm.flat_of(p)
    r.upload_scene(flat)
    before = sm.families(r, cam, rt)
    assert before["relaxed"][1][sm.COUNTERS.index("texel_fetches")] == 0
    live = [sm.rec(m) for m in p["materials"]]
    live[ground].texture = dead_checker
    r.update_materials(live)
    got = same_as_fresh(r, sm.edited(flat, materials=live), cam, rt)
    assert got["relaxed"][1][sm.COUNTERS.index("texel_fetches")] > 0
    r.update_materials(p["materials"])
    assert same_as_fresh(r, flat, cam, rt) == before


# ---------------------------------------------------------------- 4. built state
def recoloured(flat):
    p = sm.parts_of(flat)
    edit_metal(p)
    edit_solid_colour(p)
    return p


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_an_edit_before_anything_is_built(r, rt, tag):
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    p = recoloured(flat)
    r.upload_scene(flat)
    r.update_materials(p["materials"], p["textures"], {1: 4})
    same_as_fresh(r, sm.edited(sm.flat_of(p), assign={1: 4}), cam, rt)


def test_an_edit_after_an_f64_render_only(r):
    """The f64 side is repacked in place; the f32 side builds later from the host copy."""
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    p = recoloured(flat)
    r.upload_scene(flat)
    sm.frame(r, cam, F64)
    r.update_materials(p["materials"], p["textures"], {1: 4, 6: 0})
    after = sm.edited(sm.flat_of(p), assign={1: 4, 6: 0})
    same_as_fresh(r, after, cam, F32)
    same_as_fresh(r, after, cam, F64)


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("order", ["refit_first", "materials_first"])
def test_with_a_refit_edit_of_coordinates(r, rt, tag, order):
    """cr_update_primitives(CR_UPDATE_REFIT) before and after this call: desc_pos and the tree are intact, so the renders
    and cr_export_bvh equal those of a fresh handle that got the edited shading at upload and the same refit."""
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    p = recoloured(flat)
    assign = {2: 5, 4: 0}
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    r.upload_scene(flat)
    r.build_info(rt)
    steps = [lambda: r.update_primitives(idx, rows), lambda: r.update_materials(p["materials"], p["textures"], assign)]
    for step in (steps if order == "refit_first" else steps[::-1]):
        step()

    def refitted(f, cam, rt):
        f.build_info(rt)
        f.update_primitives(idx, rows)
        return dict(sm.families(f, cam, rt), tree=sm.tree(f, rt), build=sm.build_facts(f, rt))

    want = sm.fresh(sm.edited(sm.flat_of(p), assign=assign), refitted, cam, rt)
    got = dict(sm.families(r, cam, rt), tree=sm.tree(r, rt), build=sm.build_facts(r, rt))
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_update_shading_says_this_description_same_geometry(r, rt, tag):
    """The mirror's one call for Scene-level code: both tables and every sphere's and triangle's material of a flattened
    description whose geometry is the uploaded one's."""
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    p = recoloured(flat)
    edit_kind(p)
    edit_checker(p)
    after = sm.edited(sm.flat_of(p), assign={1: 4, 4: 1, 6: 0})
    r.upload_scene(flat)
    before = sm.frame(r, cam, rt)
    r.update_shading(after)
    assert same_as_fresh(r, after, cam, rt)["relaxed"] != before


# ---------------------------------------------------------------- 5. assignment
MODES = {"reference": A.CR_BVH_REFERENCE, "sah": A.CR_BVH_SAH, "sah_ordered": A.CR_BVH_SAH_ORDERED, "lbvh": A.CR_BVH_LBVH,
         "sah_device": A.CR_BVH_SAH | A.CR_BVH_BUILD_DEVICE}


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_sphere_of_book1_gets_another_material(r, rt, tag, mode):
    sc = book1_end_scene(1, scene_seed=1, image_width=37, samples=4)
    sc.bvh_mode = MODES[mode]
    flat, cam = sc.flatten(), sm.camera(sc, (37, 29), 4, 8)
    d = flat.desc
    old = [flat.prims[i].material for i in range(d.n_prims)]
    perm = np.random.RandomState(17).permutation(d.n_prims)
    assign = {i: old[int(perm[i])] for i in range(d.n_prims)}
    assert sum(assign[i] != old[i] for i in assign) > d.n_prims // 2
    r.upload_scene(flat)
    before = sm.families(r, cam, rt)
    tree, build = sm.tree(r, rt), r.build_info(rt)
    r.update_materials(assign=assign)
    got = same_as_fresh(r, sm.edited(flat, assign=assign), cam, rt)
    assert got["relaxed"][0] != before["relaxed"][0]
    assert sm.tree(r, rt) == tree and r.build_info(rt) == build          # not rebuilt: the build that made the tree, clocks included


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_a_hidden_primitive_changes_in_the_host_copy_only(r, rt, tag):
    """Nothing of the frame changes; the host copy did, as the description of the next call shows: the hidden primitive alone
    names an appended material, so the table cannot shrink again until it is given another one.  A rebuild from the host
    copy (CR_UPDATE_REBUILD of another primitive's own coordinates) still renders the same frame."""
    sc = scenes.mixed_scene(32, 4)
    sc.hide_element("brass")
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    hidden = next(i for i in range(flat.desc.n_prims) if flat.prims[i].flags & A.CR_PRIM_HIDDEN)
    short = sm.parts_of(flat)["materials"]
    grown = padded(short, len(short) + 1)
    r.upload_scene(flat)
    before = sm.families(r, cam, rt)
    r.update_materials(grown, assign={hidden: len(short)})
    after = sm.edited(flat, materials=grown, assign={hidden: len(short)})
    assert same_as_fresh(r, after, cam, rt) == before
    with pytest.raises(CrucibleError, match="primitive material index out of range"):
        r.update_materials(short)
    row = np.array([list(flat.prims[1].v)])
    r.update_primitives([1], row, rebuild=True)                           # the trees rebuild from the host copy
    assert same_as_fresh(r, after, cam, rt) == before
    r.update_materials(short, assign={hidden: 0})
    assert same_as_fresh(r, sm.edited(flat, assign={hidden: 0}), cam, rt) == before


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("maker", ["list", "wrapped"])
def test_objects_of_lists_are_reassigned_at_the_cost_of_a_build(r, rt, tag, maker):
    sc = scenes.list_scene(37, 4) if maker == "list" else scenes.wrapped_scene(37, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (37, 29), 4, 8)
    d = flat.desc
    assert any(flat.prims[i].kind in (A.CR_PRIM_LIST, A.CR_PRIM_BVH) for i in range(d.n_prims))
    members = [i for i in range(d.n_prims) if flat.prims[i].flags & A.CR_PRIM_MEMBER]
    assign = {i: (flat.prims[i].material + 1 + k % 2) % d.n_materials for k, i in enumerate(members)}
    r.upload_scene(flat)
    before = both_orders(r, cam, rt)
    built = r.build_info(rt)["total_ms"]
    r.update_materials(assign=assign)
    got = same_as_fresh(r, sm.edited(flat, assign=assign), cam, rt, both_orders)
    assert got["relaxed"][0] != before["relaxed"][0]
    assert r.build_info(rt)["total_ms"] != built                          # another build ran


# ---------------------------------------------------------------- 6. frame trees
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_frame_trees_stay_for_tables_and_go_with_an_assignment(r, rt, tag):
    sc = scenes.moving_scene(32, 4, frame=1)
    sc.bvh_mode = A.CR_BVH_SAH
    flat = sc.flatten()
    cam = sm.camera(sc, (32, 24), 4, 8, refit_boxes="rebuild")
    r.upload_scene(flat)
    both_orders(r, cam, rt)
    info = r.frame_build_info(rt)
    assert info["n_wrappers"] > 0 and info["total_ms"] > 0
    p = sm.parts_of(flat)
    edit_metal(p)
    p["materials"] = padded(p["materials"], len(p["materials"]) + 3)
    r.update_materials(p["materials"])
    assert r.frame_build_info(rt) == info
    same_as_fresh(r, sm.flat_of(p), cam, rt, both_orders)
    assert r.frame_build_info(rt) == info                                 # the same ray times: nothing was built
    assign = {1: 2, 2: 1}
    r.update_materials(assign=assign)
    zero = r.frame_build_info(rt)
    assert all(v == 0 for v in zero.values()), zero
    same_as_fresh(r, sm.edited(sm.flat_of(p), assign=assign), cam, rt, both_orders)
    assert r.frame_build_info(rt)["n_wrappers"] == info["n_wrappers"]


# ---------------------------------------------------------------- 7. ordering
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_an_asynchronous_render_before_the_edit_sees_the_scene_as_it_was(r, rt, tag):
    import torch
    sc = scenes.mixed_scene(37, 8)
    flat, cam = sc.flatten(), sm.camera(sc, (37, 29), 8, 8)
    p = recoloured(flat)
    assign = {1: 4, 4: 1}
    after = sm.edited(sm.flat_of(p), assign=assign)
    dt = torch.float64 if rt == F64 else torch.float32
    a = torch.zeros((cam.image_height, cam.image_width, 3), dtype=dt, device="cuda:0")
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    r.upload_scene(flat)
    r.build_info(rt)
    assert r.render_device(cam, a.data_ptr(), seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED) is None   # asynchronous: no stats
    r.update_materials(p["materials"], p["textures"], assign)
    assert r.render_device(cam, b.data_ptr(), seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED) is None
    r.synchronize()
    pre, post = sm.fresh(flat, sm.frame, cam, rt)[0], sm.fresh(after, sm.frame, cam, rt)[0]
    assert a.cpu().numpy().tobytes() == pre and b.cpu().numpy().tobytes() == post and pre != post


# ---------------------------------------------------------------- 8. refusals
def refusal_cases(flat):
    """(arguments after the handle, status, whole message) for the mixed scene: 10 materials, 10 textures, no list records"""
    p = sm.parts_of(flat)
    mats, texs = p["materials"], p["textures"]
    n_p, n_m = len(p["prims"]), len(mats)
    bad = A.CR_ERR_INVALID_ARG
    I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31

    def with_material(i, m):
        out = [sm.rec(x) for x in mats]
        out[i] = m
        return out

    def with_texture(i, t):
        out = [sm.rec(x) for x in texs]
        out[i] = t
        return out

    deep = [sm.solid(0, 0, 0), sm.solid(1, 1, 1)] + [sm.checker(2.0, 1 + k, 0) for k in range(A.CR_MAX_CHECKER_DEPTH + 1)]
    deep += [sm.image_texture(0)] * 2       # the kept materials' texture indices stay in range
    lam = first_material(p, L)
    return [
        ((mats, -1, None, 0, None, None, 0), bad, "cr_update_materials: negative count"),
        ((None, 0, texs, I32_MIN, None, None, 0), bad, "cr_update_materials: negative count"),
        ((None, 0, None, 0, [0], [0], -1), bad, "cr_update_materials: negative count"),
        ((None, 3, None, 0, None, None, 0), bad, "cr_update_materials: a null table with a count that is not zero"),
        ((None, 0, None, I32_MAX, None, None, 0), bad, "cr_update_materials: a null table with a count that is not zero"),
        ((None, 0, None, 0, None, [0], 1), bad, "cr_update_materials: null assignment arrays"),
        ((None, 0, None, 0, [0], None, 1), bad, "cr_update_materials: null assignment arrays"),
        ((None, 0, None, 0, [0, n_p], [0, 0], 2), bad, "cr_update_materials: primitive index out of range"),
        ((None, 0, None, 0, [-1], [0], 1), bad, "cr_update_materials: primitive index out of range"),
        ((None, 0, None, 0, [I32_MAX], [0], 1), bad, "cr_update_materials: primitive index out of range"),
        ((None, 0, None, 0, [3, 5, 3], [0, 0, 0], 3), bad, "cr_update_materials: a primitive is named twice"),
        ((None, 0, None, 0, [2], [n_m], 1), bad, "primitive material index out of range"),
        ((None, 0, None, 0, [2], [-1], 1), bad, "primitive material index out of range"),
        ((mats[:n_m - 1], n_m - 1, None, 0, None, None, 0), bad, "primitive material index out of range"),     # shrinks under a primitive
        ((mats, 0, None, 0, None, None, 0), bad, "primitive material index out of range"),                      # an empty table
        ((with_material(1, A.CrMaterial(7, -1, (C.c_double * 3)(0, 0, 0), 1.0)), n_m, None, 0, None, None, 0), bad, "unknown material kind"),
        ((with_material(lam, sm.lambertian(len(texs))), n_m, None, 0, None, None, 0), bad, "material texture index out of range"),
        ((None, 0, texs[:2], 2, None, None, 0), bad, "material texture index out of range"),                    # new textures, kept materials
        ((with_material(1, sm.metal((0.5, 0.5, 0.5), 1.5)), n_m, None, 0, None, None, 0), bad, "A metal cannot have a fuzz factor above 1.0"),
        ((with_material(1, sm.metal((0.5, 0.5, 0.5), -0.5)), n_m, None, 0, None, None, 0), bad, "A metal cannot have a fuzz factor below 0.0"),
        ((with_material(1, sm.metal((0.5, 1.5, 0.5), 0.5)), n_m, None, 0, None, None, 0), bad, "colour component outside [0,1]"),
        ((with_material(1, sm.dielectric(float("nan"))), n_m, None, 0, None, None, 0), bad, "material parameter is not finite"),
        ((None, 0, with_texture(0, A.CrTexture(5, -1, -1, -1, (C.c_double * 3)(0, 0, 0), 0.0)), len(texs), None, None, 0), bad, "unknown texture kind"),
        ((None, 0, with_texture(2, sm.checker(1.0, 2, 0)), len(texs), None, None, 0), bad, "checker sub-textures must have smaller indices"),
        ((None, 0, with_texture(3, sm.image_texture(len(p["images"]))), len(texs), None, None, 0), bad, "texture image index out of range"),
        ((None, 0, with_texture(0, sm.solid(0.5, -0.1, 0.5)), len(texs), None, None, 0), bad, "colour component outside [0,1]"),
        ((None, 0, deep, len(deep), None, None, 0), A.CR_ERR_UNSUPPORTED, "checker textures nested deeper than CR_MAX_CHECKER_DEPTH (32)"),
        # double faults: the call's own refusals first, then the description's in cr_upload_scene's order
        ((mats, -1, None, 5, None, None, 1), bad, "cr_update_materials: negative count"),
        ((None, 0, None, 0, [3, 3, n_p], [0, 0, 0], 3), bad, "cr_update_materials: primitive index out of range"),
        ((None, 0, with_texture(0, sm.solid(2, 0, 0)), len(texs), [3, 3], [0, 0], 2), bad, "cr_update_materials: a primitive is named twice"),
        ((with_material(1, sm.metal((0.5, 0.5, 0.5), 1.5)), n_m, with_texture(0, sm.solid(2, 0, 0)), len(texs), None, None, 0), bad, "colour component outside [0,1]"),
        ((with_material(1, sm.metal((0.5, 0.5, 0.5), 1.5)), n_m, None, 0, [2], [n_m], 1), bad, "A metal cannot have a fuzz factor above 1.0"),
    ]


def everything(r, cam, rt):
    return dict(sm.families(r, cam, rt), tree=sm.tree(r, rt), build=r.build_info(rt))


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_refused_calls_say_why_and_change_nothing(hiplib, r, rt, tag):
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    assert hiplib.cr_update_materials(None, None, 0, None, 0, None, None, 0) == A.CR_ERR_INVALID_ARG           # a null handle
    assert sm.raw_materials(hiplib, r.h, None, 0, None, 0, None, None, 0) == (A.CR_ERR_NO_SCENE, "cr_update_materials before cr_upload_scene")
    assert sm.raw_materials(hiplib, r.h, None, -1, None, 0, None, None, 0) == (A.CR_ERR_INVALID_ARG, "cr_update_materials: negative count")
    r.upload_scene(flat)
    first = everything(r, cam, rt)
    assert sm.raw_materials(hiplib, r.h, None, 0, None, 0, None, None, 0)[0] == A.CR_OK                        # names nothing: does nothing
    assert sm.raw_materials(hiplib, r.h, None, 0, None, 0, [0], [0], 0)[0] == A.CR_OK
    for args, code, msg in refusal_cases(flat):
        assert sm.raw_materials(hiplib, r.h, *args) == (code, msg), msg
    with pytest.raises(CrucibleError, match="named twice"):
        r.update_materials(assign=([1, 1], [0, 0]))
    got = everything(r, cam, rt)
    assert got == first                                                                                         # clocks of the build included: nothing rebuilt
    want = sm.fresh(flat, sm.families, cam, rt)
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("maker", ["list", "wrapped"])
def test_a_list_record_has_no_material(hiplib, r, maker):
    sc = scenes.list_scene(32, 4) if maker == "list" else scenes.wrapped_scene(32, 4)
    flat = sc.flatten()
    record = next(i for i in range(flat.desc.n_prims) if flat.prims[i].kind in (A.CR_PRIM_LIST, A.CR_PRIM_BVH))
    r.upload_scene(flat)
    assert sm.raw_materials(hiplib, r.h, None, 0, None, 0, [record], [0], 1) == (A.CR_ERR_INVALID_ARG, "cr_update_materials: a list element has no material to assign")
    assert sm.raw_materials(hiplib, r.h, None, 0, None, 0, [record, flat.desc.n_prims], [0, 0], 2)[1] == "cr_update_materials: primitive index out of range"


# ---------------------------------------------------------------- 11. groups
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_a_two_member_group_follows_the_three_edits(hiplib, monkeypatch, rt, tag):
    """Both members edited through cr_group_update_materials, cr_group_update_image and cr_group_set_sky render the single
    handle's relaxed frame of the edited description bit for bit; a refusal leaves both members as they were."""
    monkeypatch.setenv("CRUCIBLE_GROUP_SAME_DEVICE", "1")
    sc = scenes.mixed_scene(32, 4)
    flat, cam = sc.flatten(), sm.camera(sc, (32, 24), 4, 8)
    p = recoloured(flat)
    assign = {1: 4, 4: 1}
    texels = sm.seeded_image(p["images"][0].shape[1], p["images"][0].shape[0], 23)
    p["images"][0] = texels
    p["sky"] = (A.CR_SKY_SPHERICAL, 0)
    after = sm.edited(sm.flat_of(p), assign=assign)
    g = RenderGroup.local([0, 0])
    try:
        g.upload_scene(flat)
        first, st = g.render(cam, seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
        assert st["members"] == 2 and first.tobytes() == sm.fresh(flat, sm.frame, cam, rt)[0]
        members = [C.c_void_p(hiplib.cr_group_handle(g.g, k)) for k in range(2)]
        for call in (lambda: sm.raw_materials(hiplib, g.g, None, 0, None, 0, [2, 2], [0, 0], 2, group=True),
                     lambda: (hiplib.cr_group_update_image(g.g, 9, 0, 0, 1, 1, texels.ctypes.data_as(C.POINTER(C.c_uint8))), hiplib.cr_group_last_error(g.g).decode()),
                     lambda: (hiplib.cr_group_set_sky(g.g, 7, 0), hiplib.cr_group_last_error(g.g).decode())):
            rc, msg = call()
            assert rc == A.CR_ERR_INVALID_ARG and msg in ("cr_update_materials: a primitive is named twice", "cr_update_image: image index out of range", "unknown sky kind")
        again, _ = g.render(cam, seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
        assert again.tobytes() == first.tobytes()
        g.update_materials(p["materials"], p["textures"], assign)
        g.update_image(0, texels)
        g.set_sky(A.CR_SKY_SPHERICAL, 0)
        got, st = g.render(cam, seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
        want = sm.fresh(after, sm.frame, cam, rt)
        assert got.tobytes() == want[0] and got.tobytes() != first.tobytes()
        for k, name in enumerate(sm.COUNTERS):
            if name not in ("scene_in_lds", "bvh_entries"):
                assert st[name] == want[1][k], name
        assert len(members) == 2
    finally:
        g.close()
