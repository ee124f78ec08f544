"""crucible_amd/csrc/scene_checks.hpp, the descriptor checks cr_upload_scene shares with cr_update_materials, cr_update_image
and cr_set_sky, checked without a device: tests/scene_checks_check.cpp compiles the header with g++ (plain, and with
-fsanitize=undefined,address as the stand-alone program it is) and prints one line per case; what each case must answer is
restated here from the contract in include/crucible_hip.h.  Every refusal is reached once with its code and whole message,
the order of two simultaneous faults is pinned, and the ends are covered: a checker chain of exactly CR_MAX_CHECKER_DEPTH and
one more, a materials table shrunk to the largest used index + 1 and one below that, counts and indices at the ends of
int32_t, a rectangle whose x0 + width overflows 32 bits, and live_texture_remap where the device table changes size."""
import os
import re
import subprocess

import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = A.CR_OK, A.CR_ERR_INVALID_ARG, A.CR_ERR_UNSUPPORTED

TEX_KIND = (INVALID, "unknown texture kind")
CHECKER = (INVALID, "checker sub-textures must have smaller indices")
TEX_IMAGE = (INVALID, "texture image index out of range")
COLOUR = (INVALID, "colour component outside [0,1]")
DEPTH = (UNSUPPORTED, "checker textures nested deeper than CR_MAX_CHECKER_DEPTH (32)")
MAT_KIND = (INVALID, "unknown material kind")
MAT_TEX = (INVALID, "material texture index out of range")
FUZZ_ABOVE = (INVALID, "A metal cannot have a fuzz factor above 1.0")
FUZZ_BELOW = (INVALID, "A metal cannot have a fuzz factor below 0.0")
PARAM = (INVALID, "material parameter is not finite")
PRIM_MAT = (INVALID, "primitive material index out of range")
SKY_KIND = (INVALID, "unknown sky kind")
SKY_IMAGE = (INVALID, "sky image index out of range")
NEGATIVE = (INVALID, "cr_update_materials: negative count")
NULL_TABLE = (INVALID, "cr_update_materials: a null table with a count that is not zero")
NULL_ARRAYS = (INVALID, "cr_update_materials: null assignment arrays")
RANGE = (INVALID, "cr_update_materials: primitive index out of range")
TWICE = (INVALID, "cr_update_materials: a primitive is named twice")
LIST = (INVALID, "cr_update_materials: a list element has no material to assign")
IMG_NULL = (INVALID, "cr_update_image: null texels")
IMG_SIZE = (INVALID, "cr_update_image: width or height below 1")
IMG_INDEX = (INVALID, "cr_update_image: image index out of range")
IMG_RECT = (INVALID, "cr_update_image: the rectangle leaves the image")
FINE = (OK, "")

WANT = {
    "tex_kind": TEX_KIND, "checker_self": CHECKER, "checker_forward": CHECKER, "tex_image": TEX_IMAGE, "tex_image_ok": FINE,
    "tex_colour": COLOUR, "tex_colour_nan": COLOUR, "depth_at_limit": FINE, "depth_over": DEPTH, "two_tex_faults_first_wins": COLOUR,
    "tex_empty": FINE,
    "mat_kind": MAT_KIND, "mat_kind_negative": MAT_KIND, "mat_texture": MAT_TEX, "mat_texture_negative": MAT_TEX, "mat_texture_ok": FINE,
    "fuzz_above": FUZZ_ABOVE, "fuzz_below": FUZZ_BELOW, "fuzz_nan": FUZZ_ABOVE, "metal_albedo": COLOUR,
    "param_nan": PARAM, "param_inf": PARAM, "param_neg_inf": PARAM, "two_mat_faults_first_wins": PARAM,
    "prim_material_at_count": PRIM_MAT, "prim_material_last": FINE, "prim_material_negative": PRIM_MAT, "prim_material_int_max": PRIM_MAT,
    "prim_material_int_min": PRIM_MAT,
    "sky_kind": SKY_KIND, "sky_kind_negative": SKY_KIND, "sky_default": FINE, "sky_image_at_count": SKY_IMAGE, "sky_image_negative": SKY_IMAGE,
    "sky_image_int_max": SKY_IMAGE, "sky_image_ok": FINE,
    "args_negative_materials": NEGATIVE, "args_negative_textures": NEGATIVE, "args_negative_assign": NEGATIVE,
    "args_null_materials_with_count": NULL_TABLE, "args_null_textures_with_count": NULL_TABLE, "args_null_index": NULL_ARRAYS,
    "args_null_material": NULL_ARRAYS, "args_nothing": FINE, "args_empty_tables": FINE,
    "args_negative_before_null": NEGATIVE, "args_contradiction_before_null_arrays": NULL_TABLE,
    "upd_nothing": FINE, "upd_index_negative": RANGE, "upd_index_at_count": RANGE, "upd_index_int_max": RANGE, "upd_index_int_min": RANGE,
    "upd_twice": TWICE, "upd_list": LIST, "upd_bvh": LIST, "upd_assign_ok": FINE,
    "upd_assign_at_count": PRIM_MAT, "upd_assign_negative": PRIM_MAT, "upd_assign_int_max": PRIM_MAT, "upd_assign_int_min": PRIM_MAT,
    # the scene's primitives use materials 0, 2, 1, 2: three records hold them, two do not -- unless both users of 2 move
    "upd_shrink_to_largest_used_plus_one": FINE, "upd_shrink_below_used": PRIM_MAT, "upd_shrink_one_still_uses_it": PRIM_MAT,
    "upd_shrink_with_reassign": FINE, "upd_empty_table_under_primitives": PRIM_MAT,
    "upd_new_materials_against_kept_textures": MAT_TEX, "upd_both_tables_grow": FINE,
    "upd_new_textures_against_kept_materials": MAT_TEX, "upd_no_textures_no_lambertian": FINE,
    "upd_texture_image_against_n_images": TEX_IMAGE, "upd_depth_over": DEPTH,
    "order_range_before_twice": RANGE, "order_range_before_list": RANGE, "order_twice_before_list": TWICE, "order_twice_before_texture": TWICE,
    "order_texture_before_material": COLOUR, "order_list_before_texture": LIST, "order_material_before_primitive": FUZZ_ABOVE,
    "img_whole": FINE, "img_corner": FINE, "img_null": IMG_NULL, "img_width_zero": IMG_SIZE, "img_height_negative": IMG_SIZE,
    "img_height_int_min": IMG_SIZE, "img_index_negative": IMG_INDEX, "img_index_at_count": IMG_INDEX, "img_index_int_max": IMG_INDEX,
    "img_x_one_over": IMG_RECT, "img_y_one_over": IMG_RECT, "img_x0_negative": IMG_RECT, "img_y0_int_min": IMG_RECT,
    "img_x_sum_overflows": IMG_RECT, "img_x_sum_wraps_to_small": IMG_RECT, "img_y_sum_overflows": IMG_RECT,
    "order_img_null_before_size": IMG_NULL, "order_img_size_before_index": IMG_SIZE, "order_img_index_before_rect": IMG_INDEX,
}

# textures 0, 1 solids; 2 checker(0, 1); 3 image; 4 checker(2, 3): new index of each, and the device table's size
REMAP = {
    "remap_all_solid": ([-1, -1, -1, -1, -1], 0),
    "remap_dead_checker_becomes_live": ([0, 1, 2, -1, -1], 3),      # the table grows from nothing to the checker and its two children
    "remap_checker_back_to_solid": ([-1, -1, -1, -1, -1], 0),       # and shrinks again
    "remap_image_alone": ([-1, -1, -1, 0, -1], 1),
    "remap_image_behind_a_checker_level": ([0, 1, 2, 3, 4], 5),
    "remap_metal_names_no_texture": ([-1, -1, -1, -1, -1], 0),
    "remap_no_textures": ([], 0),
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's lines by case name; the plain and the sanitized build agree and write nothing to stderr."""
    out = tmp_path_factory.mktemp("scene_checks_check")
    outs = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(out / f"scene_checks_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "scene_checks_check.cpp")])
        res = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    got = {}
    for line in outs[0].splitlines():
        name, rest = line.split("|", 1)
        assert name not in got, name
        got[name] = rest
    return got


def test_every_case_is_answered(lines):
    assert set(lines) == set(WANT) | set(REMAP)


@pytest.mark.parametrize("name", sorted(WANT))
def test_refusals_and_their_order(lines, name):
    code, msg = lines[name].split("|", 1)
    assert (int(code), msg) == WANT[name]


def test_every_refusal_of_the_contract_is_reached():
    reached = set(WANT.values())
    for refusal in (TEX_KIND, CHECKER, TEX_IMAGE, COLOUR, DEPTH, MAT_KIND, MAT_TEX, FUZZ_ABOVE, FUZZ_BELOW, PARAM, PRIM_MAT, SKY_KIND, SKY_IMAGE, NEGATIVE,
                    NULL_TABLE, NULL_ARRAYS, RANGE, TWICE, LIST, IMG_NULL, IMG_SIZE, IMG_INDEX, IMG_RECT):
        assert refusal in reached


@pytest.mark.parametrize("name", sorted(REMAP))
def test_live_texture_remap(lines, name):
    kind, idx, n = lines[name].split("|")
    assert kind == "remap" and ([int(v) for v in idx.split()], int(n)) == REMAP[name]


def test_the_library_runs_the_header():
    """scene.hip includes the header and both cr_upload_scene and the new calls go through its functions."""
    text = open(os.path.join(ROOT, "crucible_amd", "csrc", "scene.hip")).read()
    assert '#include "scene_checks.hpp"' in text
    upload = text[text.index("int32_t cr_upload_scene("):text.index("int32_t cr_update_primitives(")]
    for fn in ("check_textures(", "check_materials(", "check_prim_material(", "check_sky_kind(", "check_sky_image("):
        assert fn in upload, fn
    for fn in ("check_materials_args(", "check_materials_update(", "check_image_update(", "check_sky_kind(", "check_sky_image("):
        assert fn in text.replace(upload, ""), fn
    header = open(os.path.join(ROOT, "crucible_amd", "csrc", "scene_checks.hpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', header)
    assert includes and all(not i.startswith("hip/") and not i.endswith(".hpp") for i in includes), includes   # the C ABI header and the standard library
