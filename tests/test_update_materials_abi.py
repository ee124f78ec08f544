"""cr_update_materials, cr_update_image, cr_set_sky and their group forms at the boundary, without a GPU: the header declares
them with the signatures the issue of record gives, the ctypes table mirrors them, the export map lets them out and the built
library refuses a null handle, the Python mirrors expose the methods and build the calls' arguments, the C++ mirror and the
FFI block of INTEGRATION.md list them, and the ABI version is unchanged (symbols are only added)."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cr_update_materials", "cr_update_image", "cr_set_sky", "cr_group_update_materials", "cr_group_update_image", "cr_group_set_sky")


def squeezed(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_header_declares_the_six_signatures():
    text = squeezed("include", "crucible_hip.h")
    for who, first in (("cr_update_materials", "CrHandle* h"), ("cr_group_update_materials", "CrGroup* g")):
        assert (f"CR_API int32_t {who}({first}, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, "
                "int32_t n_textures, const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign);") in text
    for who, first in (("cr_update_image", "CrHandle* h"), ("cr_group_update_image", "CrGroup* g")):
        assert (f"CR_API int32_t {who}({first}, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, "
                "const uint8_t* rgb8);") in text
    assert "CR_API int32_t cr_set_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image);" in text
    assert "CR_API int32_t cr_group_set_sky(CrGroup* g, int32_t sky_kind, int32_t sky_image);" in text
    assert "#define CR_ABI_VERSION 4" in text


def test_python_table_mirrors_the_signatures():
    i32 = C.c_int32
    materials = [C.c_void_p, C.POINTER(A.CrMaterial), i32, C.POINTER(A.CrTexture), i32, C.POINTER(i32), C.POINTER(i32), i32]
    image = [C.c_void_p, i32, i32, i32, i32, i32, C.POINTER(C.c_uint8)]
    sky = [C.c_void_p, i32, i32]
    for name, want in zip(NAMES, (materials, image, sky) * 2):
        res, args = A.SYMBOLS[name]
        assert res is i32 and args == want, name
    assert A.CR_ABI_VERSION == 4


def test_export_map_lets_them_out():
    text = open(os.path.join(ROOT, "crucible_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", text)
    assert patterns
    globs = [p.strip() for p in patterns[0].split()]
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), name


def test_library_exports_the_calls_and_refuses_a_null_handle(hiplib):
    assert hiplib.cr_abi_version() == 4
    mat, tex = (A.CrMaterial * 1)(), (A.CrTexture * 1)()
    idx = (C.c_int32 * 1)(0)
    px = (C.c_uint8 * 3)(1, 2, 3)
    for fn in (hiplib.cr_update_materials, hiplib.cr_group_update_materials):
        assert fn(None, mat, 1, tex, 1, idx, idx, 1) == A.CR_ERR_INVALID_ARG
        assert fn(None, None, 0, None, 0, None, None, 0) == A.CR_ERR_INVALID_ARG
    for fn in (hiplib.cr_update_image, hiplib.cr_group_update_image):
        assert fn(None, 0, 0, 0, 1, 1, px) == A.CR_ERR_INVALID_ARG
    for fn in (hiplib.cr_set_sky, hiplib.cr_group_set_sky):
        assert fn(None, A.CR_SKY_DEFAULT, -1) == A.CR_ERR_INVALID_ARG


def test_python_mirrors_expose_the_methods():
    from crucible_amd.group import RenderGroup
    from crucible_amd.renderer import Renderer
    for cls in (Renderer, RenderGroup):
        for method in ("update_materials", "update_image", "set_sky"):
            assert callable(getattr(cls, method)), (cls, method)
    assert callable(Renderer.update_shading)


def test_material_arrays():
    from crucible_amd.renderer import material_arrays
    assert material_arrays() == (None, 0, None, 0, None, None, 0)
    m = [A.CrMaterial(A.CR_MAT_METAL, -1, (C.c_double * 3)(0.5, 0.5, 0.5), 0.25)] * 3
    mats, n_m, texs, n_t, idx, mat, n = material_arrays(m, [], {4: 2, 1: 0})
    assert n_m == 3 and mats[2].param == 0.25 and n_t == 0 and texs is not None      # an empty table is still a table
    assert n == 2 and [idx[0], idx[1]] == [4, 1] and [mat[0], mat[1]] == [2, 0]
    *_, idx, mat, n = material_arrays(assign=(np.arange(3), [2, 2, 1]))
    assert n == 3 and [idx[k] for k in range(3)] == [0, 1, 2] and [mat[k] for k in range(3)] == [2, 2, 1]
    table = (A.CrMaterial * 2)()
    assert material_arrays(table)[0] is table                                        # a ctypes table passes through
    with pytest.raises(ValueError):
        material_arrays(assign=([1, 2], [0]))


def test_shading_arrays_name_every_sphere_and_triangle():
    import scenes
    from crucible_amd.renderer import shading_arrays
    flat = scenes.mixed_scene(16, 1).flatten()
    d = flat.desc
    mats, n_m, texs, n_t, idx, mat, n = shading_arrays(flat)
    want = [i for i in range(d.n_prims) if d.prims[i].kind in (A.CR_PRIM_SPHERE, A.CR_PRIM_TRIANGLE)]
    assert (n_m, n_t, n) == (d.n_materials, d.n_textures, len(want)) and n > 0
    assert [idx[k] for k in range(n)] == want and [mat[k] for k in range(n)] == [d.prims[i].material for i in want]
    assert C.addressof(mats) == C.addressof(flat.materials) and C.addressof(texs) == C.addressof(flat.textures)


def test_image_arrays():
    from crucible_amd.renderer import image_arrays
    px = np.arange(5 * 3 * 3, dtype=np.uint8).reshape(3, 5, 3)
    x0, y0, w, h, ptr = image_arrays(px)
    assert (x0, y0, w, h) == (0, 0, 5, 3) and [ptr[k] for k in range(4)] == [0, 1, 2, 3]
    x0, y0, w, h, ptr = image_arrays(px[1:2, 2:4], rect=(2, 1, 2, 1))                 # a view is made contiguous
    assert (x0, y0, w, h) == (2, 1, 2, 1) and [ptr[k] for k in range(6)] == list(px[1, 2:4].ravel())
    with pytest.raises(ValueError):
        image_arrays(px, rect=(0, 0, 4, 3))
    with pytest.raises(ValueError):
        image_arrays(px.ravel())


def test_cpp_mirror_and_ffi_block_list_them():
    host = squeezed("crucible_amd", "host", "crucible.hpp")
    for call in ("cr_update_materials(h,", "cr_update_image(h,", "cr_set_sky(h,"):
        assert call in host, call
    assert "inline int32_t update_shading(CrHandle* h, const FlatScene& f)" in host
    text = squeezed("INTEGRATION.md")
    block = text[text.index('extern "C" {'):text.index("## 3. The call site")]
    for who, first in (("cr_update_materials", "h: *mut CrHandle"), ("cr_group_update_materials", "g: *mut CrGroup")):
        assert (f"pub fn {who}({first}, materials: *const CrMaterial, n_materials: i32, textures: *const CrTexture, n_textures: i32, "
                "prim_index: *const i32, prim_material: *const i32, n_assign: i32) -> i32;") in block
    for who, first in (("cr_update_image", "h: *mut CrHandle"), ("cr_group_update_image", "g: *mut CrGroup")):
        assert f"pub fn {who}({first}, image: i32, x0: i32, y0: i32, width: i32, height: i32, rgb8: *const u8) -> i32;" in block
    assert "pub fn cr_set_sky(h: *mut CrHandle, sky_kind: i32, sky_image: i32) -> i32;" in block
    assert "pub fn cr_group_set_sky(g: *mut CrGroup, sky_kind: i32, sky_image: i32) -> i32;" in block
