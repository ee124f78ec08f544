"""What tests/test_gpu_update_materials.py and tests/test_gpu_update_image.py share: flattened descriptions taken apart and put
together again with other tables, material indices, texels or sky (the "edited description" of include/crucible_hip.h), and
the yardstick of every case -- a FRESH handle that received cr_upload_scene of that description, compared with the edited
handle call by call: output bytes, the four work counters, samples, bvh_entries and scene_in_lds."""
import copy
import ctypes as C

import numpy as np

from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import FlatScene

F32, F64 = A.CR_REAL_F32, A.CR_REAL_F64
REALS = [(F64, "f64"), (F32, "f32")]
COUNTERS = ("samples", "segments", "node_tests", "prim_tests", "texel_fetches", "bvh_entries", "scene_in_lds")
SEED = 0x5EED
# adaptive calls: samples is a multiple of 2 * pass_samples
ADAPTIVE = dict(tolerance=0.02, min_samples=2, pass_samples=1, block=8)


def rec(x):
    return type(x).from_buffer_copy(x)


def parts_of(flat):
    """The description as Python lists of copied records (and the images' arrays), free to edit."""
    d = flat.desc
    return dict(prims=[rec(flat.prims[i]) for i in range(d.n_prims)], materials=[rec(flat.materials[i]) for i in range(d.n_materials)],
                textures=[rec(flat.textures[i]) for i in range(d.n_textures)], images=[im.copy() for im in flat._image_arrays],
                keys=[rec(flat.keys[i]) for i in range(d.n_keys)], sky=(d.sky_kind, d.sky_image), bvh_mode=d.bvh_mode)


def flat_of(parts):
    flat = FlatScene(parts["prims"], parts["materials"], parts["textures"], parts["images"], parts["keys"], *parts["sky"])
    flat.desc.bvh_mode = parts["bvh_mode"]
    return flat


def edited(flat, materials=None, textures=None, assign=None, sky=None, bvh_mode=None):
    """The description `flat` with other tables (whole), the materials {primitive: material} and / or another sky."""
    p = parts_of(flat)
    if materials is not None:
        p["materials"] = [rec(m) for m in materials]
    if textures is not None:
        p["textures"] = [rec(t) for t in textures]
    for i, m in (assign or {}).items():
        p["prims"][i].material = m
    if sky is not None:
        p["sky"] = sky
    if bvh_mode is not None:
        p["bvh_mode"] = bvh_mode
    return flat_of(p)


def solid(r, g, b):
    return A.CrTexture(A.CR_TEX_SOLID, -1, -1, -1, (C.c_double * 3)(r, g, b), 0.0)


def checker(inv_scale, even, odd):
    return A.CrTexture(A.CR_TEX_CHECKER, even, odd, -1, (C.c_double * 3)(0, 0, 0), inv_scale)


def image_texture(i):
    return A.CrTexture(A.CR_TEX_IMAGE, -1, -1, i, (C.c_double * 3)(0, 0, 0), 0.0)


def lambertian(texture, prob=1.0):
    return A.CrMaterial(A.CR_MAT_LAMBERTIAN, texture, (C.c_double * 3)(0, 0, 0), prob)


def metal(albedo, fuzz):
    return A.CrMaterial(A.CR_MAT_METAL, -1, (C.c_double * 3)(*albedo), fuzz)


def dielectric(ri):
    return A.CrMaterial(A.CR_MAT_DIELECTRIC, -1, (C.c_double * 3)(1, 1, 1), ri)


def camera(sc, size=(37, 29), samples=4, depth=8, **attrs):
    """A copy of the scene's camera at the tests' sizes: 24 x 16 to 37 x 29 pixels still reach edge tiles."""
    cam = copy.deepcopy(sc.scene_cam)
    cam.image_width, cam.image_height = size
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    for k, v in attrs.items():
        setattr(cam, k, v)
    return cam


def counters(st):
    return tuple(st[k] for k in COUNTERS)


def frame(r, cam, rt, order=A.CR_SUM_RELAXED):
    img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=order)
    return img.tobytes(), counters(st)


def families(r, cam, rt, region=(5, 3, 17, 11)):
    """Every family once on the handle `r`: the render in the suite's reference order and with relaxed sums named, the guide
    pass's four layers, a region, an adaptive frame with its counts.  name -> (bytes, ..., counters)"""
    out = {"reference": frame(r, cam, rt, A.CR_SUM_REFERENCE_ORDER), "relaxed": frame(r, cam, rt, A.CR_SUM_RELAXED)}
    planes, st = r.render_aov(cam, A.CR_AOV_ALL, seed=SEED, real_type=rt)
    out["aov"] = tuple(planes[k].tobytes() for k in ("albedo", "normal", "depth", "coverage")) + (counters(st),)
    img, st = r.render_region(cam, region, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    out["region"] = (img.tobytes(), counters(st))
    img, counts, st = r.render_adaptive(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED, **ADAPTIVE)
    out["adaptive"] = (img.tobytes(), counts.tobytes(), counters(st["render"]), st["passes"], st["blocks_stopped"])
    return out


def fresh(flat, what, *args, **kw):
    """what(renderer, ...) on a new handle that received cr_upload_scene(flat): the yardstick of every case."""
    r = Renderer(0)
    try:
        r.upload_scene(flat)
        return what(r, *args, **kw)
    finally:
        r.close()


def tree(r, rt):
    return tuple(a.tobytes() for a in r.export_bvh(rt))


def build_facts(r, rt):
    """cr_build_info without its clocks"""
    info = r.build_info(rt)
    return {k: v for k, v in info.items() if not k.endswith("_ms")}


def raw_materials(lib, h, materials, n_materials, textures, n_textures, index, material, n_assign, group=False):
    """The raw C call (for the cases the mirrors would refuse to build arguments for): (status, whole message)."""
    keep = []

    def table(records, ctype):
        if records is None:
            return None
        arr = (ctype * max(1, len(records)))(*records)
        keep.append(arr)
        return arr

    def ints(values):
        if values is None:
            return None
        arr = (C.c_int32 * max(1, len(values)))(*values)
        keep.append(arr)
        return arr

    fn = lib.cr_group_update_materials if group else lib.cr_update_materials
    rc = fn(h, table(materials, A.CrMaterial), n_materials, table(textures, A.CrTexture), n_textures, ints(index), ints(material), n_assign)
    err = lib.cr_group_last_error if group else lib.cr_last_error
    return rc, (err(h) or b"").decode()


def seeded_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
