"""cr_update_primitives / cr_group_update_primitives at the boundary, without a GPU: the header declares them, the ctypes
table mirrors their signatures, the built library exports them and refuses a null handle, the ABI version is unchanged.
And the yardstick of tests/test_gpu_update.py is checked here first: the numpy box model of tests/update_model.py
reproduces the oracle's own reference-built tree exactly, and the oracle walking a reference-built tree of the edited
scenes agrees with its linear list to the cap the GPU tests hold the refitted renders to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenes
import update_model as um
from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
SCENES = {"mixed": lambda: scenes.mixed_scene(64, 2), "moving": lambda: scenes.moving_scene(64, 2)}


def test_header_declares_both_signatures():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crucible_hip.h")).read())
    assert "enum { CR_UPDATE_REFIT = 0, CR_UPDATE_REBUILD = 1 };" in text
    assert ("CR_API int32_t cr_update_primitives(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, "
            "int32_t flags);") in text
    assert ("CR_API int32_t cr_group_update_primitives(CrGroup* g, const int32_t* prim_index, const double* v, "
            "int32_t n, int32_t flags);") in text
    assert "#define CR_ABI_VERSION 4" in text


def test_python_table_mirrors_the_signatures():
    want = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.c_int32]
    for name in ("cr_update_primitives", "cr_group_update_primitives"):
        res, args = A.SYMBOLS[name]
        assert res is C.c_int32 and args == want, name
    assert (A.CR_UPDATE_REFIT, A.CR_UPDATE_REBUILD) == (0, 1)
    assert A.CR_ABI_VERSION == 4


def test_library_exports_the_calls_and_refuses_a_null_handle(hiplib):
    assert hiplib.cr_abi_version() == 4
    rows = np.zeros((1, 9))
    for group in (False, True):
        for flags in (A.CR_UPDATE_REFIT, A.CR_UPDATE_REBUILD):
            assert um.update_call(hiplib, None, None, rows, flags, group=group) == A.CR_ERR_INVALID_ARG
            assert um.update_call(hiplib, None, None, None, flags, n=0, group=group) == A.CR_ERR_INVALID_ARG


def test_python_wrappers_exist():
    from crucible_amd.group import RenderGroup
    from crucible_amd.renderer import Renderer, update_arrays
    assert callable(Renderer.update_primitives) and callable(RenderGroup.update_primitives)
    idx, v, n = update_arrays(None, np.arange(18.0))
    assert idx is None and v.shape == (2, 9) and n == 2
    idx, v, n = update_arrays([3, 1], np.zeros((2, 9), dtype=np.float32))
    assert n == 2 and v.dtype == np.float64 and [idx[0], idx[1]] == [3, 1]
    with pytest.raises(ValueError):
        update_arrays([1, 2, 3], np.zeros((2, 9)))


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("edit", [False, True], ids=["as_built", "edited"])
def test_box_model_reproduces_the_oracle_tree(oracles, rt, tag, name, edit):
    """Leaf boxes from the primitives in `real`, inner boxes from the children, bottom-up over `children`: applied to
    the oracle's own tree (oracle_bvh_dump) the model gives the oracle's boxes, bit for bit -- also for the tree the
    oracle builds of an edited description (its topology then differs from the unedited one's; the rule does not)."""
    o = oracles[rt]
    flat = SCENES[name]().flatten()
    if edit:
        um.apply_edit(flat, *um.seeded_edit(flat, um.EDIT_SEED))
    boxes, children = um.oracle_tree(o, flat)
    kind, flags, v = um.prim_arrays(flat)
    assert len(children) > 3
    named = sorted({int(~c) for c in children.ravel() if c < 0})
    assert named == [i for i in range(len(kind)) if not flags[i] & A.CR_PRIM_HIDDEN]
    model = um.model_boxes(children, kind, v, o.np_real)
    assert model.dtype == boxes.dtype and np.array_equal(model, boxes)


def test_box_model_sees_an_edit(o64):
    """The model is not vacuous: moving one sphere changes its leaf's box and the root's."""
    flat = scenes.mixed_scene(32, 1).flatten()
    boxes, children = um.oracle_tree(o64, flat)
    kind, _, v = um.prim_arrays(flat)
    v2 = v.copy()
    v2[4, :3] += (400.0, 0.0, 0.0)
    moved = um.model_boxes(children, kind, v2, np.float64)
    assert np.array_equal(um.model_boxes(children, kind, v, np.float64), boxes)
    assert moved[0, 1] > boxes[0, 1] and (moved != boxes).any(axis=1).sum() >= 2


def test_seeded_edit_moves_spheres_and_triangles_and_changes_radii():
    flat = scenes.mixed_scene(32, 1).flatten()
    kind, _, v = um.prim_arrays(flat)
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    assert len(set(idx.tolist())) == len(idx) and 3 <= len(idx) < len(kind) and 0 not in idx
    assert {int(kind[i]) for i in idx} == {A.CR_PRIM_SPHERE, A.CR_PRIM_TRIANGLE}
    spheres = kind[idx] == A.CR_PRIM_SPHERE
    assert (rows[spheres, 3] > 0).all() and np.isnan(rows[spheres, 4:]).all() and np.isfinite(rows[~spheres]).all()
    assert (rows[spheres, 3] != v[idx[spheres], 3]).any() and (np.abs(rows[:, :3] - v[idx, :3]).max(axis=1) > 0).all()
    um.apply_edit(flat, idx, rows)
    _, _, v2 = um.prim_arrays(flat)
    assert np.array_equal(v2[idx[spheres], 4:], v[idx[spheres], 4:]) and np.array_equal(v2[idx[~spheres]], rows[~spheres])


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_tree_of_the_edited_scene_meets_the_linear_list_cap(oracles, rt, tag, name):
    """The bar test_gpu_update.py sets for a refitted render -- at least 99.5 % of the pixels equal to the oracle's
    linear list of the edited scene -- is one the oracle's own reference-built tree of that scene meets: the pixels
    that differ are rays grazing a box face, not the edit."""
    o = oracles[rt]
    sc = SCENES[name]()
    sc.scene_cam.refit_boxes = True    # keyed primitives: boxes that follow them, as the GPU test renders them
    flat = sc.flatten()
    um.apply_edit(flat, *um.seeded_edit(flat, um.EDIT_SEED))
    truth, _ = um.oracle_render_flat(o, flat, sc.scene_cam, seed=99, linear_list=True)
    tree, _ = um.oracle_render_flat(o, flat, sc.scene_cam, seed=99)
    same = (tree == truth).all(axis=2).mean()
    print(name, tag, "pixels equal to the linear list:", same)
    assert same >= 0.995, same
