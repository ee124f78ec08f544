"""CR_BVH_BUILD_DEVICE: the CR_BVH_SAH / CR_BVH_SAH_ORDERED tree built on the device (crucible_amd/csrc/sah_device.hpp,
DESIGN.md 6.6) is held to the same independent CPU build as the host builder's (tests/sah_model.py), wrapper for
wrapper and with no tolerance: children, split_axis and boxes.  CRUCIBLE_SAH_SMALL=4 drives small scenes through many
level-synchronous rounds; the default sends them to the one-wave pass whole.  cr_build_info says which builder ran."""
import numpy as np
import pytest

import lbvh_model as L
import sah_model as M
from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError
from test_gpu_sah_build import SCENES, assert_equal_trees, edited_scene, model
from test_gpu_lbvh_build import random_spheres

pytestmark = pytest.mark.gpu

DEVICE = A.CR_BVH_BUILD_DEVICE
REALS = [(A.CR_REAL_F64, np.float64), (A.CR_REAL_F32, np.float32)]
REAL_IDS = ["f64", "f32"]
THRESHOLDS = [None, 4]            # CRUCIBLE_SAH_SMALL: the default, and many rounds on a small scene
THRESHOLD_IDS = ["default", "small4"]
DEFAULT_THRESHOLD = 256         # kSahSmallDefault (sah_device.hpp)
NAMES = [n for n in SCENES if "million" not in n]


def set_threshold(monkeypatch, small):
    if small is None:
        monkeypatch.delenv("CRUCIBLE_SAH_SMALL", raising=False)
    else:
        monkeypatch.setenv("CRUCIBLE_SAH_SMALL", str(small))


def export(renderer, sc, mode, rt):
    sc.bvh_mode = mode
    flat = sc.flatten()
    renderer.upload_scene(flat)
    return flat, renderer.export_bvh(rt)


# ------------------------------------------------------------------ 1. the tree equals the model
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("small", THRESHOLDS, ids=THRESHOLD_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_device_tree_equals_the_model(renderer, monkeypatch, name, small, rt, real):
    set_threshold(monkeypatch, small)
    flat, got = export(renderer, SCENES[name](), A.CR_BVH_SAH_ORDERED | DEVICE, rt)
    want = model(name, flat, real, A.CR_BVH_SAH_ORDERED)
    assert_equal_trees(got, want, name)
    info = renderer.build_info(rt)
    n = len(want.order)
    assert info["bvh_mode"] == A.CR_BVH_SAH_ORDERED and info["n_wrappers"] == len(want.children)
    assert info["built_on_device"] == (1 if n >= 3 else 0)        # fewer than 3 primitives are one leaf, written on the host
    if n < 3:
        assert info["small_threshold"] == 0 and info["device_rounds"] == 0 and info["small_subtrees"] == 0
    else:
        assert info["small_threshold"] == (small if small is not None else DEFAULT_THRESHOLD)   # no override leaks in from another test
        if n <= info["small_threshold"]:
            assert info["device_rounds"] == 0 and info["large_nodes"] == 0 and info["small_subtrees"] == 1
        else:
            # every range above the threshold is split in a round, every other child of such a range is a small subtree
            span = want.end - want.start
            large = span > info["small_threshold"]
            kids = want.children[large]
            assert info["large_nodes"] == int(large.sum())
            assert info["small_subtrees"] == int((~large[kids]).sum())
            assert info["device_rounds"] >= 1
    if small == 4 and name in ("r4097", "teapot"):
        assert info["device_rounds"] >= 8 and info["large_nodes"] > 100 and info["small_subtrees"] > 100
    if small is None and name == "r255":
        assert n == 255 < info["small_threshold"] == DEFAULT_THRESHOLD and info["device_rounds"] == 0 and info["small_subtrees"] == 1


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", ["mixed", "book1", "r4097", "lattice", "hand_square_xz"])
def test_plain_sah_on_the_device(renderer, monkeypatch, name, rt, real):
    set_threshold(monkeypatch, 64)
    flat, got = export(renderer, SCENES[name](), A.CR_BVH_SAH | DEVICE, rt)
    want = model(name, flat, real, A.CR_BVH_SAH)
    assert_equal_trees(got, want, name)
    assert (got[2] == -1).all()
    assert renderer.build_info(rt)["bvh_mode"] == A.CR_BVH_SAH


# ------------------------------------------------------------------ 2. the same as the host builder
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", ["book1", "teapot", "mixed", "r4097"])
def test_device_export_equals_the_host_export(renderer, monkeypatch, name, rt, real):
    set_threshold(monkeypatch, None)
    sc = SCENES[name]()
    _, host = export(renderer, sc, A.CR_BVH_SAH_ORDERED, rt)
    assert renderer.build_info(rt)["built_on_device"] == 0
    _, dev = export(renderer, sc, A.CR_BVH_SAH_ORDERED | DEVICE, rt)
    assert renderer.build_info(rt)["built_on_device"] == 1
    for x, y in zip(host, dev):
        assert x.shape == y.shape and np.array_equal(x, y)


# ------------------------------------------------------------------ 3. deterministic
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_device_build_twice(renderer, monkeypatch, rt, real):
    """20000 random spheres at a threshold of 64: several large nodes per round over several rounds, chunks of the
    order that straddle node boundaries.  Built twice, both exports equal each other and the model."""
    set_threshold(monkeypatch, 64)
    sc = random_spheres(20000, seed=2, half=200.0)
    flat, first = export(renderer, sc, A.CR_BVH_SAH_ORDERED | DEVICE, rt)
    info = renderer.build_info(rt)
    _, second = export(renderer, sc, A.CR_BVH_SAH_ORDERED | DEVICE, rt)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    assert_equal_trees(first, model("device_twice", flat, real, A.CR_BVH_SAH_ORDERED), "device_twice")
    assert info["device_rounds"] >= 6 and info["large_nodes"] > 2 * info["device_rounds"] and info["small_threshold"] == 64


# ------------------------------------------------------------------ 4. edits
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_rebuild_and_refit_after_an_edit(renderer, monkeypatch, rt, real):
    import update_model as um
    set_threshold(monkeypatch, 16)
    mode = A.CR_BVH_SAH_ORDERED
    sc, idx, rows, mover = edited_scene(real)
    flat, before = export(renderer, sc, mode | DEVICE, rt)
    want0 = M.build(flat, real, mode)
    assert_equal_trees(before, want0, "before the edit")
    renderer.update_primitives(idx, rows)                     # refit: the original topology, the edited boxes
    um.apply_edit(flat, idx, rows)
    recs = L.prim_records(flat)
    pbox = L.prim_boxes(recs["kind"], recs["v"], real)
    refit = want0._replace(boxes=L.union_boxes(want0.children, lambda i: pbox[i], real))
    assert not np.array_equal(refit.boxes, want0.boxes)
    assert_equal_trees(renderer.export_bvh(rt), refit, "refit")
    renderer.update_primitives(idx[:1], rows[:1], rebuild=True)
    want1 = M.build(flat, real, mode)
    assert_equal_trees(renderer.export_bvh(rt), want1, "rebuild")
    info = renderer.build_info(rt)
    assert info["built_on_device"] == 1 and info["device_rounds"] >= 1
    assert not np.array_equal(want1.children, want0.children)


# ------------------------------------------------------------------ 5. renders
def book1_small():
    sc = SCENES["book1"]()
    cam = sc.scene_cam
    cam.image_width, cam.image_height = 48, 32
    cam.set_samples(4)
    return sc, cam


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_render_equals_the_host_built_tree(renderer, monkeypatch, rt, real):
    set_threshold(monkeypatch, 32)
    sc, cam = book1_small()
    frames = []
    for mode in (A.CR_BVH_SAH_ORDERED, A.CR_BVH_SAH_ORDERED | DEVICE):
        sc.bvh_mode = mode
        renderer.upload_scene(sc.flatten())
        frames.append(renderer.render(cam, seed=0xC0FFEE, real_type=rt))
    (img0, st0), (img1, st1) = frames
    assert img0.shape == (32, 48, 3) and np.array_equal(img0, img1)
    for k in ("segments", "node_tests", "prim_tests", "texel_fetches"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert st0["bvh_entries"] == st1["bvh_entries"] and st0["prim_tests"] > 0


def test_render_matches_the_oracle_walking_the_model_tree(renderer, oracles, monkeypatch):
    set_threshold(monkeypatch, 32)
    rt, real = A.CR_REAL_F64, np.float64
    sc, cam = book1_small()
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED | DEVICE
    flat = sc.flatten()
    renderer.upload_scene(flat)
    img, st = renderer.render(cam, seed=0xC0FFEE, real_type=rt, sum_order=A.CR_SUM_REFERENCE_ORDER)
    want = M.build(flat, real, M.ORDERED)
    ref, rst = oracles[rt].render_image(sc, seed=0xC0FFEE, tree=(want.boxes, want.children, want.split_axis))
    assert np.array_equal(img, ref), f"differing px = {(img != ref).any(axis=2).sum()}"
    for k in ("segments", "node_tests", "prim_tests", "texel_fetches"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["bvh_entries"] == len(want.children)


# ------------------------------------------------------------------ 6. refusals
def test_reference_mode_has_no_device_build(renderer):
    sc, cam = book1_small()
    sc.bvh_mode = A.CR_BVH_SAH
    renderer.upload_scene(sc.flatten())
    img0, _ = renderer.render(cam, seed=7, real_type=A.CR_REAL_F32)
    sc.bvh_mode = A.CR_BVH_REFERENCE | DEVICE
    with pytest.raises(CrucibleError) as err:
        renderer.upload_scene(sc.flatten())
    assert err.value.code == A.CR_ERR_UNSUPPORTED
    img1, _ = renderer.render(cam, seed=7, real_type=A.CR_REAL_F32)       # the previous scene still renders
    assert np.array_equal(img0, img1)
    assert renderer.build_info(A.CR_REAL_F32)["bvh_mode"] == A.CR_BVH_SAH


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_lbvh_takes_the_flag_and_ignores_it(renderer, rt, real):
    sc = SCENES["r4097"]()
    _, plain = export(renderer, sc, A.CR_BVH_LBVH, rt)
    _, flagged = export(renderer, sc, A.CR_BVH_LBVH | DEVICE, rt)
    for x, y in zip(plain, flagged):
        assert np.array_equal(x, y)
    info = renderer.build_info(rt)
    assert info["bvh_mode"] == A.CR_BVH_LBVH and info["built_on_device"] == 1 and info["device_rounds"] == 0


@pytest.mark.parametrize("mode", [A.CR_BVH_SAH | 0x200, A.CR_BVH_SAH | DEVICE | 0x1000, 7 | DEVICE, 4, A.CR_BVH_SAH | (1 << 30), -1])
def test_unknown_bits_are_refused(renderer, mode):
    sc = SCENES["n5"]()
    sc.bvh_mode = mode
    with pytest.raises(CrucibleError) as err:
        renderer.upload_scene(sc.flatten())
    assert err.value.code == A.CR_ERR_INVALID_ARG


def test_build_info_error_codes(hiplib, renderer):
    import ctypes as C
    from crucible_amd.renderer import Renderer
    info = A.CrBuildInfo()
    assert hiplib.cr_build_info(None, A.CR_REAL_F32, C.byref(info)) == A.CR_ERR_INVALID_ARG
    fresh = Renderer(0)
    try:
        assert hiplib.cr_build_info(fresh.h, A.CR_REAL_F32, C.byref(info)) == A.CR_ERR_NO_SCENE
        assert hiplib.cr_build_info(fresh.h, A.CR_REAL_F32, None) == A.CR_ERR_INVALID_ARG
    finally:
        fresh.close()
    renderer.upload_scene(SCENES["n5"]().flatten())
    assert hiplib.cr_build_info(renderer.h, A.CR_REAL_F32, None) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_build_info(renderer.h, 2, C.byref(info)) == A.CR_ERR_INVALID_ARG
    assert hiplib.cr_build_info(renderer.h, A.CR_REAL_F64, C.byref(info)) == A.CR_OK
    assert info.n_wrappers > 0 and info.built_on_device == 0 and info.bvh_mode == A.CR_BVH_REFERENCE and info.total_ms > 0
