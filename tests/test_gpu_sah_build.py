"""The host-built CR_BVH_SAH / CR_BVH_SAH_ORDERED trees against an independent CPU build (tests/sah_model.py, itself
pinned on the CPU by tests/test_sah_model_host.py): cr_export_bvh's boxes, children and split_axis must equal the model's
exactly, wrapper for wrapper, in both modes and in f32 and f64.

The other checks of these modes cannot see a builder that is merely worse: the bit-exact renders hand the exported tree
to the oracle, which then walks whatever was built; the well-formedness test accepts any proper tree; the box test
recomputes the boxes of whatever topology came out; and the node-test bar is one number on one scene.  Fewer bins, a
cost without the counts, one axis tried, an unstable partition, ties to the last candidate, a wrong split axis: each
costs speed at most, none a pixel.  Here every one of them changes `children` or `split_axis`.  No tolerance anywhere."""
import time

import numpy as np
import pytest

import lbvh_model as L
import sah_model as M
import scenes
from crucible_amd import _abi as A
from test_gpu_lbvh_build import SCENES as LBVH_SCENES
from scenes import SAH_HAND as HAND
from scenes import subnormal_extent_scene
from test_gpu_lbvh_build import random_spheres      # with SCENES: the LBVH file's table and its maker of random spheres

pytestmark = pytest.mark.gpu

REALS = [(A.CR_REAL_F64, np.float64), (A.CR_REAL_F32, np.float32)]
REAL_IDS = ["f64", "f32"]
MODES = [A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED]
MODE_IDS = ["sah", "ordered"]
assert (M.SAH, M.ORDERED) == (A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED)

THREADED = 70000     # the root and the two ranges below it span >= 2^15: the builder's std::thread branch, two deep


def nan_centroid_scene():
    """In f32 one triangle reaches from -inf to inf along x: its box midpoint is no number, bounds nothing and falls
    into bin 0 by definition; the others split around it."""
    rng = np.random.RandomState(41)
    v = rng.uniform(-4, 4, (12, 9))
    v[5, 0], v[5, 3] = -1e39, 1e39
    return scenes.ArrayScene(np.full(12, L.TRIANGLE, dtype=np.int32), v)


SCENES = dict(LBVH_SCENES)
SCENES.update({
    "n0": lambda: scenes.few_spheres(0), "list_scene": lambda: scenes.list_scene(48, 2),
    "wrapped_scene": lambda: scenes.wrapped_scene(48, 2), "r300": lambda: random_spheres(300, seed=5, half=5.0),
    "subnormal_extent": subnormal_extent_scene, "nan_centroid": nan_centroid_scene,
})
SCENES.update({"hand_" + name: case[0] for name, case in HAND.items()})

_models = {}


def model(name, flat, real, mode):
    """The model's tree of a named scene: built once per real type, the two modes differ in split_axis only."""
    key = (name, real)
    if key not in _models:
        _models[key] = M.build(flat, real, M.ORDERED)
    t = _models[key]
    return t if mode == A.CR_BVH_SAH_ORDERED else t._replace(split_axis=np.full(len(t.children), -1, dtype=np.int32))


def export(renderer, sc, mode, rt):
    sc.bvh_mode = mode
    flat = sc.flatten()
    renderer.upload_scene(flat)
    return flat, renderer.export_bvh(rt)


def assert_equal_trees(got, want, what):
    """Every wrapper: children, boxes, split_axis."""
    boxes, kids, axis = got
    if len(want.children) == 0:
        assert len(kids) == 0, what
        return
    assert kids.shape == want.children.shape, (what, kids.shape, want.children.shape)
    bad = np.nonzero((kids != want.children).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(kids)} wrappers differ in children, first {bad[0]}: {kids[bad[0]]} != {want.children[bad[0]]}"
    bad = np.nonzero(axis != want.split_axis)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(kids)} wrappers differ in split_axis, first {bad[0]}: {axis[bad[0]]} != {want.split_axis[bad[0]]}"
    bad = np.nonzero((boxes != want.boxes).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(kids)} boxes differ, first {bad[0]}: {boxes[bad[0]]} != {want.boxes[bad[0]]}"
    assert np.array_equal(kids, want.children) and np.array_equal(boxes, want.boxes) and np.array_equal(axis, want.split_axis)


# ------------------------------------------------------------------ the builder against the model
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_sah_tree_equals_the_model(renderer, name, mode, rt, real):
    sc = SCENES[name]()
    flat, got = export(renderer, sc, mode, rt)
    want = model(name, flat, real, mode)
    assert_equal_trees(got, want, name)
    inner = want.children[:, 0] >= 0
    # the scenes do hold what their names promise
    if name.startswith("hand_"):
        _, children, axis, _ = HAND[name[5:]]
        assert got[1].tolist() == children
        assert got[2].tolist() == (axis if mode == A.CR_BVH_SAH_ORDERED else [-1] * len(axis))
    if name.startswith("concentric"):
        # one centre, but (c - r) + (c + r) rounds: some box midpoints sit an ulp off it, and extents of an ulp do split
        n_mid = int((want.plane[inner] == -1).sum())
        assert inner.sum() // 2 < n_mid < inner.sum()
    if name in ("huge_1e300", "huge_1.5e308", "beyond_f32") and real == np.float32:
        # all but one primitive have an infinite coordinate, so no side's area is finite: midpoint splits only
        assert (want.plane[inner] == -1).all() and inner.sum() > 10
    if name == "subnormal_extent":
        assert want.axis[0] == (0 if real == np.float64 else 2)
    if name == "nan_centroid" and real == np.float32:
        assert np.isinf(want.boxes[0, 0:2]).all() and (want.axis[inner] != 0).any()
    if name in ("mixed", "list_scene", "wrapped_scene"):
        recs = L.prim_records(flat)
        assert ((recs["flags"][want.order] & L.MEMBER) != 0).sum() > 5         # members stand in for their list or wrapper
        if name == "mixed":
            assert len(want.order) < (recs["kind"] <= 1).sum()                    # ... the hidden ones left out
    if name == "teapot":
        assert (L.prim_records(flat)["kind"][want.order] == L.TRIANGLE).sum() == 6320


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_threaded_build_twice(renderer, mode, rt, real):
    """70000 random spheres: the top of the tree is built by concurrent threads.  Built twice, both exports equal each
    other and the model, every wrapper compared.  The times of this run are printed."""
    sc = random_spheres(THREADED, seed=2, half=200.0)
    t0 = time.time()
    flat, first = export(renderer, sc, mode, rt)
    _, second = export(renderer, sc, mode, rt)
    t1 = time.time()
    want = model("threaded", flat, real, mode)
    print(f"n = {THREADED}: two uploads + exports {t1 - t0:.2f} s, model {time.time() - t1:.2f} s (0 when shared with the other mode)")
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    assert_equal_trees(first, want, "threaded")
    inner = want.children[:, 0] >= 0
    big = (want.end - want.start) >= (1 << 15)
    assert big[0] and big[want.children[0]].all() and big.sum() >= 3 and (want.plane[inner & big] >= 0).all()


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", ["mixed", "book1", "r4097", "lattice", "hand_square_xz"])
def test_the_two_modes_share_a_topology(renderer, name, rt, real):
    sc = SCENES[name]()
    _, (b1, k1, a1) = export(renderer, sc, A.CR_BVH_SAH, rt)
    _, (b2, k2, a2) = export(renderer, sc, A.CR_BVH_SAH_ORDERED, rt)
    assert np.array_equal(k1, k2) and np.array_equal(b1, b2)
    inner = k1[:, 0] >= 0
    assert (a1 == -1).all() and (a2[inner] >= 0).all() and (a2[~inner] == -1).all()


# ------------------------------------------------------------------ edits of an uploaded scene
def edited_scene(real):
    """300 random spheres and an edit: a third of them moved and resized at random, and sphere `mover` carried along
    the root's split axis from the left of the root's plane to the right of it, inside the centroid bounds (which two
    untouched spheres hold): measured in the bins of the uploaded scene's root it crosses the plane."""
    sc = random_spheres(300, seed=11, half=6.0)
    flat = sc.flatten()
    v = L.prim_records(flat)["v"].copy()
    t = M.build(flat, real)
    a, plane = int(t.axis[0]), int(t.plane[0])
    assert plane >= 0
    cen = 0.5 * (t.prim_boxes[:, 0::2].astype(np.float64) + t.prim_boxes[:, 1::2].astype(np.float64))
    clo, chi = cen[:, a].min(), cen[:, a].max()
    keep = {int(cen[:, a].argmin()), int(cen[:, a].argmax())}
    scale = 16.0 / (chi - clo)
    bins = M.bin_index((cen[:, a] - clo) * scale)
    mover = next(i for i in np.nonzero(bins <= plane)[0] if int(i) not in keep)
    rs = np.random.RandomState(12)
    idx = np.array(sorted({int(mover)} | {int(i) for i in np.nonzero(rs.uniform(size=300) < 0.3)[0] if int(i) not in keep}), dtype=np.int32)
    rows = v[idx].copy()
    rows[:, 0:3] += rs.uniform(-1.0, 1.0, (len(idx), 3))
    rows[:, 3] *= rs.uniform(0.6, 1.5, len(idx))
    at = int(np.nonzero(idx == mover)[0][0])
    rows[at] = v[mover]
    rows[at, a] = clo + (plane + 2.5) / scale          # a bin and a half beyond the plane
    new_bin = int(M.bin_index((float(real(rows[at, a])) - clo) * scale))
    assert bins[mover] <= plane < new_bin              # the edit does cross the root's plane
    return sc, idx, rows, int(mover)


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_rebuild_and_refit_after_an_edit(renderer, mode, rt, real):
    import update_model as um
    sc, idx, rows, mover = edited_scene(real)
    flat, before = export(renderer, sc, mode, rt)
    want0 = M.build(flat, real, mode)
    assert_equal_trees(before, want0, "before the edit")
    # refit: the topology of the original description, the boxes of the edited primitives
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)
    recs = L.prim_records(flat)
    pbox = L.prim_boxes(recs["kind"], recs["v"], real)
    refit = want0._replace(boxes=L.union_boxes(want0.children, lambda i: pbox[i], real))
    assert not np.array_equal(refit.boxes, want0.boxes)
    assert_equal_trees(renderer.export_bvh(rt), refit, "refit")
    # rebuild: the model of the edited description
    renderer.update_primitives(idx[:1], rows[:1], rebuild=True)
    want1 = M.build(flat, real, mode)
    assert_equal_trees(renderer.export_bvh(rt), want1, "rebuild")
    assert not np.array_equal(want1.children, want0.children)


# ------------------------------------------------------------------ the render, on the model's tree
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_ordered_render_matches_the_oracle_walking_the_model_tree(renderer, oracles, rt, real):
    """The bit-exact renders elsewhere hand the oracle the EXPORTED tree and axes; here it walks the model's, so image
    and work counters are pinned to a tree and to split axes the library had no part in."""
    sc = random_spheres(300, seed=5, half=5.0)
    cam = sc.scene_cam
    cam.image_width, cam.image_height = 24, 16
    cam.set_samples(2)
    cam.look_from((3.0, 5.0, 14.0))
    cam.look_at((0.0, 0.0, 0.0))
    cam.set_vfov(45.0)
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED
    flat = sc.flatten()
    renderer.upload_scene(flat)
    img, st = renderer.render(cam, seed=0xC0FFEE, real_type=rt)
    want = M.build(flat, real, M.ORDERED)
    ref, rst = oracles[rt].render_image(sc, seed=0xC0FFEE, tree=(want.boxes, want.children, want.split_axis))
    assert img.shape == (16, 24, 3)
    assert np.array_equal(img, ref), f"differing px = {(img != ref).any(axis=2).sum()}"
    for k in ("segments", "node_tests", "prim_tests", "texel_fetches"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["bvh_entries"] == len(want.children)
    assert st["prim_tests"] > 0 and (img != img[0, 0]).any()      # the camera does see the spheres
