"""cr_update_image and cr_set_sky on the device: texels of a rectangle of an uploaded image replaced in place, and the sky
switched (include/crucible_hip.h).  The yardstick of every case is a fresh handle that received
cr_upload_scene of the edited description (shading_model.fresh): bytes and counters, texel_fetches among them, are equal."""
import ctypes as C

import numpy as np
import pytest

import scenes
import shading_model as sm
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import ImageTexture, Lambertian, RTWImage, Sphere
from shading_model import REALS

pytestmark = pytest.mark.gpu


@pytest.fixture
def r(hiplib):
    handle = Renderer(0)
    yield handle
    handle.close()


def two_image_scene(size, use):
    """A few spheres, one wrapped in image 0 (size w x h, seeded); image 1, of another size, is the other user's: the sky when
    image 0 is a texture, a second sphere's texture when image 0 is the sky.  Its texels lie behind image 0's in the texel
    array, so an edit of image 0 that gets the offset arithmetic wrong shows in it."""
    w, h = size
    sc = scenes.few_spheres(4, 37, 4)
    first, second = RTWImage(sm.seeded_image(w, h, 31)), RTWImage(sm.seeded_image(7, 6, 32))
    if use == "texture":
        sc.add_element(Sphere.new((0.0, 1.6, -1.0), 0.9, Lambertian.new_from_texture(ImageTexture(first), 1.0)), "globe")
        sc.load_spherical_skybox(second)
    else:
        sc.load_spherical_skybox(first)
    flat = sc.flatten()
    p = sm.parts_of(flat)
    if use == "sky":      # image 0 is the sky's (flatten numbers images by first use: textures first): put it first
        assert len(p["images"]) == 1
        p["images"].append(second.rgb8.copy())
        p["textures"].append(sm.image_texture(1))
        p["materials"].append(sm.lambertian(len(p["textures"]) - 1))
        p["prims"][0].material = len(p["materials"]) - 1
        flat = sm.flat_of(p)
    assert flat._image_arrays[0].shape[:2] == (h, w) and flat.desc.n_images == 2
    return sc, flat


def rectangles(w, h):
    return {"top_left": (0, 0, 1, 1), "top_right": (w - 1, 0, 1, 1), "bottom_left": (0, h - 1, 1, 1), "bottom_right": (w - 1, h - 1, 1, 1),
            "row": (0, h // 2, w, 1), "column": (w // 2, 0, 1, h), "inside": (1, 1, w - 2, h - 2), "whole": (0, 0, w, h)}


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("use", ["texture", "sky"])
@pytest.mark.parametrize("size", [(5, 3), (64, 32)], ids=["5x3", "64x32"])
def test_rectangles_of_an_image(r, rt, tag, use, size):
    """Every rectangle in turn on one handle, each on top of the last: the frame equals the fresh upload of the image as
    edited so far, and the second image's users are untouched."""
    w, h = size
    sc, flat = two_image_scene(size, use)
    cam = sm.camera(sc, (37, 29), 4, 8)
    r.upload_scene(flat)
    first = sm.families(r, cam, rt)
    p = sm.parts_of(flat)
    for k, (name, (x0, y0, rw, rh)) in enumerate(rectangles(w, h).items()):
        block = sm.seeded_image(rw, rh, 100 + k)
        block[..., k % 3] = 255 - 40 * (k % 2)             # no rectangle repeats what it covers
        p["images"][0][y0:y0 + rh, x0:x0 + rw] = block
        r.update_image(0, block, (x0, y0, rw, rh))
        what = sm.families if name in ("top_left", "whole") else sm.frame
        got, want = what(r, cam, rt), sm.fresh(sm.flat_of(p), what, cam, rt)
        assert got == want, name
    assert got["relaxed"][0] != first["relaxed"][0]


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_the_whole_image_without_a_rectangle_and_a_device_render_before_it(r, rt, tag):
    import torch
    sc, flat = two_image_scene((64, 32), "texture")
    cam = sm.camera(sc, (37, 29), 8, 8)
    p = sm.parts_of(flat)
    p["images"][0] = sm.seeded_image(64, 32, 77)
    dt = torch.float64 if rt == sm.F64 else torch.float32
    a = torch.zeros((cam.image_height, cam.image_width, 3), dtype=dt, device="cuda:0")
    torch.cuda.synchronize()
    r.upload_scene(flat)
    r.build_info(rt)
    assert r.render_device(cam, a.data_ptr(), seed=sm.SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED) is None   # asynchronous
    r.update_image(0, p["images"][0])
    after = sm.frame(r, cam, rt)
    r.synchronize()
    assert a.cpu().numpy().tobytes() == sm.fresh(flat, sm.frame, cam, rt)[0]           # launched before: the texels as they were
    assert after == sm.fresh(sm.flat_of(p), sm.frame, cam, rt) and after[0] != a.cpu().numpy().tobytes()


# ---------------------------------------------------------------- sky
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_the_sky_default_spherical_another_image_default(r, rt, tag):
    sc, flat = two_image_scene((64, 32), "texture")
    p = sm.parts_of(flat)
    p["sky"] = (A.CR_SKY_DEFAULT, -1)
    cam = sm.camera(sc, (37, 29), 4, 8)
    r.upload_scene(sm.flat_of(p))
    seen = []
    for sky in ((A.CR_SKY_DEFAULT, -1), (A.CR_SKY_SPHERICAL, 1), (A.CR_SKY_SPHERICAL, 0), (A.CR_SKY_DEFAULT, -1)):
        r.set_sky(*sky)
        p["sky"] = sky
        got, want = sm.families(r, cam, rt), sm.fresh(sm.flat_of(p), sm.families, cam, rt)     # the guide pass's albedo on misses among them
        assert got == want, sky
        seen.append((got["relaxed"][0], got["aov"][0]))
    assert seen[0] == seen[3] and len({s[0] for s in seen}) == 3 and len({s[1] for s in seen}) == 3


# ---------------------------------------------------------------- refusals
def image_call(lib, h, image, x0, y0, w, h_, pixels):
    ptr = None if pixels is None else pixels.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.cr_update_image(h, image, x0, y0, w, h_, ptr)
    return rc, (lib.cr_last_error(h) or b"").decode()


def test_refused_calls_say_why_and_change_nothing(hiplib, r):
    rt = sm.F64
    sc, flat = two_image_scene((5, 3), "texture")
    cam = sm.camera(sc, (32, 24), 4, 8)
    px = sm.seeded_image(8, 8, 1)
    bad, I32_MAX, I32_MIN = A.CR_ERR_INVALID_ARG, 2 ** 31 - 1, -2 ** 31
    assert hiplib.cr_update_image(None, 0, 0, 0, 1, 1, px.ctypes.data_as(C.POINTER(C.c_uint8))) == bad
    assert hiplib.cr_set_sky(None, A.CR_SKY_DEFAULT, -1) == bad
    assert image_call(hiplib, r.h, 0, 0, 0, 1, 1, px) == (A.CR_ERR_NO_SCENE, "cr_update_image before cr_upload_scene")
    assert hiplib.cr_set_sky(r.h, A.CR_SKY_DEFAULT, -1) == A.CR_ERR_NO_SCENE and hiplib.cr_last_error(r.h) == b"cr_set_sky before cr_upload_scene"
    r.upload_scene(flat)
    first = dict(sm.families(r, cam, rt), tree=sm.tree(r, rt), build=r.build_info(rt))
    for args, msg in (((0, 0, 0, 1, 1, None), "cr_update_image: null texels"),
                      ((0, 0, 0, 0, 1, px), "cr_update_image: width or height below 1"),
                      ((0, 0, 0, 1, -3, px), "cr_update_image: width or height below 1"),
                      ((-1, 0, 0, 1, 1, px), "cr_update_image: image index out of range"),
                      ((2, 0, 0, 1, 1, px), "cr_update_image: image index out of range"),
                      ((I32_MAX, 0, 0, 1, 1, px), "cr_update_image: image index out of range"),
                      ((0, 1, 0, 5, 3, px), "cr_update_image: the rectangle leaves the image"),
                      ((0, 0, 1, 5, 3, px), "cr_update_image: the rectangle leaves the image"),
                      ((0, -1, 0, 1, 1, px), "cr_update_image: the rectangle leaves the image"),
                      ((0, 0, I32_MIN, 1, 1, px), "cr_update_image: the rectangle leaves the image"),
                      ((0, 2, 0, I32_MAX, 1, px), "cr_update_image: the rectangle leaves the image"),      # 2 + INT32_MAX wraps in 32 bits
                      ((0, I32_MAX, I32_MAX, I32_MAX, I32_MAX, px), "cr_update_image: the rectangle leaves the image"),
                      ((1, 0, 0, 8, 6, px), "cr_update_image: the rectangle leaves the image"),            # image 1 is 7 x 6
                      ((9, 0, 0, 0, 0, None), "cr_update_image: null texels"),                             # double faults, in the order of the checks
                      ((9, 0, 0, 0, 1, px), "cr_update_image: width or height below 1"),
                      ((9, -1, 0, 1, 1, px), "cr_update_image: image index out of range")):
        assert image_call(hiplib, r.h, *args) == (bad, msg), (args[:5], msg)
    for kind, image, msg in ((2, 0, "unknown sky kind"), (-1, 0, "unknown sky kind"), (A.CR_SKY_SPHERICAL, 2, "sky image index out of range"),
                             (A.CR_SKY_SPHERICAL, -1, "sky image index out of range"), (7, 9, "unknown sky kind")):
        assert (hiplib.cr_set_sky(r.h, kind, image), hiplib.cr_last_error(r.h).decode()) == (bad, msg)
    assert dict(sm.families(r, cam, rt), tree=sm.tree(r, rt), build=r.build_info(rt)) == first
    assert sm.fresh(flat, sm.families, cam, rt) == {k: first[k] for k in first if k not in ("tree", "build")}
