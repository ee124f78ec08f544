"""cr_update_primitives on the device: primitives of an uploaded scene edited in place.

Nothing of the reference's edits a built world, so what pins the feature is the library's own contract
(include/crucible_hip.h): after CR_UPDATE_REFIT the exported tree keeps its topology and carries the boxes an
independent numpy model derives from the edited primitives (tests/update_model.py, itself held against the oracle's
tree in tests/test_update_abi.py), and the render is the oracle's of the edited description on that exported tree, bit
for bit; after CR_UPDATE_REBUILD the handle is a fresh upload of the edited description.  Against ground truth -- the
oracle's linear list of the edited scene -- a refitted render agrees except for box-grazing rays (the 99.5 % cap of
tests/test_gpu_refit.py and tests/test_gpu_bvh_modes.py; test_update_abi.py checks that the oracle's own tree of these
edited scenes meets it)."""
import numpy as np
import pytest

import scenes
import update_model as um
from crucible_amd import _abi as A
from crucible_amd.demo_builder import million_spheres
from crucible_amd.renderer import CrucibleError, Renderer

pytestmark = pytest.mark.gpu

REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
MODES = [A.CR_BVH_REFERENCE, A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH]
MODE_IDS = ["reference", "sah", "ordered", "lbvh"]
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
SEED = 20260
both = lambda f: pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])(  # noqa: E731
    pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)(f))


def other(rt):
    return A.CR_REAL_F32 if rt == A.CR_REAL_F64 else A.CR_REAL_F64


def upload(r, sc, mode):
    sc.bvh_mode = mode
    flat = sc.flatten()
    r.upload_scene(flat)
    return flat


def shot(r, cam, rt, order=A.CR_SUM_DEFAULT):
    img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=order)
    return img, {k: st[k] for k in COUNTERS + ("bvh_entries", "scene_in_lds")}


def same_shot(a, b):
    assert np.array_equal(a[0], b[0]), f"differing px = {(a[0] != b[0]).any(axis=2).sum()}"
    assert a[1] == b[1], (a[1], b[1])


def same_tree(a, b):
    for x, y, what in zip(a, b, ("boxes", "children", "split_axis")):
        assert np.array_equal(x, y), what


def assert_oracle(oracles, rt, flat, cam, r, order=A.CR_SUM_REFERENCE_ORDER):
    """The device render of the scene on `r` against the oracle rendering `flat` on the tree `r` exports."""
    tree = r.export_bvh(rt)
    img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=order)
    ref, rst = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, tree=tree, sum_order=order)
    assert np.array_equal(img, ref), f"differing px = {(img != ref).any(axis=2).sum()}"
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    return img, tree


def assert_model_boxes(flat, rt, tree0, tree1):
    """Same topology as before the update; boxes = the numpy model over the (edited) primitives of `flat`, exactly."""
    assert np.array_equal(tree0[1], tree1[1]) and np.array_equal(tree0[2], tree1[2])
    kind, _, v = um.prim_arrays(flat)
    dtype = np.float64 if rt == A.CR_REAL_F64 else np.float32
    model = um.model_boxes(tree1[1], kind, v, dtype).astype(np.float64)
    assert np.array_equal(tree1[0], model), f"differing wrappers = {(tree1[0] != model).any(axis=1).sum()}"


# ---- 1
@both
def test_identity_update_changes_nothing(renderer, rt, tag, mode):
    sc = scenes.mixed_scene(48, 2)
    flat = upload(renderer, sc, mode)
    before, tree = shot(renderer, sc.scene_cam, rt), renderer.export_bvh(rt)
    shot(renderer, sc.scene_cam, other(rt))                      # both precisions built: the update reaches both
    tree_other = renderer.export_bvh(other(rt))
    _, _, v = um.prim_arrays(flat)
    renderer.update_primitives(None, v)                          # every primitive, its own values
    same_shot(before, shot(renderer, sc.scene_cam, rt))
    same_tree(tree, renderer.export_bvh(rt))
    same_tree(tree_other, renderer.export_bvh(other(rt)))
    some = np.array([9, 2, 5], dtype=np.int32)
    renderer.update_primitives(some, v[some])                    # and a few named ones
    same_shot(before, shot(renderer, sc.scene_cam, rt))
    same_tree(tree, renderer.export_bvh(rt))
    renderer.update_primitives(None, np.zeros((0, 9)))           # n == 0
    same_shot(before, shot(renderer, sc.scene_cam, rt))


# ---- 2
@both
def test_refit_matches_the_model_the_oracle_and_the_linear_list(renderer, oracles, rt, tag, mode):
    sc = scenes.mixed_scene(64, 2)
    flat = upload(renderer, sc, mode)
    cam = sc.scene_cam
    before = shot(renderer, cam, rt)
    tree0 = renderer.export_bvh(rt)
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)                               # `flat` is now the edited description
    assert_model_boxes(flat, rt, tree0, renderer.export_bvh(rt))
    img, tree = assert_oracle(oracles, rt, flat, cam, renderer, A.CR_SUM_REFERENCE_ORDER)
    assert_oracle(oracles, rt, flat, cam, renderer, A.CR_SUM_RELAXED)
    assert not np.array_equal(img, before[0])
    truth, _ = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, linear_list=True)
    same = (img == truth).all(axis=2).mean()
    print(tag, MODE_IDS[mode], "pixels equal to the linear list:", same)
    assert same >= 0.995, same


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_refit_reaches_both_precisions_and_one_built_later(renderer, oracles, mode):
    """f32 and f64 built before the update are both refitted; on a second scene only f32 is built, and f64 builds at
    first use from the edited host copy."""
    for build_both in (True, False):
        sc = scenes.mixed_scene(48, 2)
        flat = upload(renderer, sc, mode)
        shot(renderer, sc.scene_cam, A.CR_REAL_F32)
        trees = {A.CR_REAL_F32: renderer.export_bvh(A.CR_REAL_F32)}
        if build_both:
            trees[A.CR_REAL_F64] = renderer.export_bvh(A.CR_REAL_F64)
        idx, rows = um.seeded_edit(flat, um.EDIT_SEED + 1)
        renderer.update_primitives(idx, rows)
        um.apply_edit(flat, idx, rows)
        for rt, tree0 in trees.items():
            assert_model_boxes(flat, rt, tree0, renderer.export_bvh(rt))
        for rt in (A.CR_REAL_F32, A.CR_REAL_F64):
            assert_oracle(oracles, rt, flat, sc.scene_cam, renderer)
        if not build_both:                                       # built from the edited description: a fresh upload's tree
            fresh = Renderer(0)
            try:
                fresh.upload_scene(flat)
                same_tree(fresh.export_bvh(A.CR_REAL_F64), renderer.export_bvh(A.CR_REAL_F64))
            finally:
                fresh.close()


# ---- 3
@both
def test_rebuild_is_a_fresh_upload_of_the_edited_description(renderer, rt, tag, mode):
    sc = scenes.mixed_scene(48, 2)
    flat = upload(renderer, sc, mode)
    before = shot(renderer, sc.scene_cam, rt)
    shot(renderer, sc.scene_cam, other(rt))
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    renderer.update_primitives(idx, rows, rebuild=True)
    after, tree = shot(renderer, sc.scene_cam, rt), renderer.export_bvh(rt)
    after_other, tree_other = shot(renderer, sc.scene_cam, other(rt)), renderer.export_bvh(other(rt))
    um.apply_edit(flat, idx, rows)
    fresh = Renderer(0)
    try:
        fresh.upload_scene(flat)
        same_shot(after, shot(fresh, sc.scene_cam, rt))
        same_tree(tree, fresh.export_bvh(rt))
        same_shot(after_other, shot(fresh, sc.scene_cam, other(rt)))
        same_tree(tree_other, fresh.export_bvh(other(rt)))
    finally:
        fresh.close()
    assert not np.array_equal(after[0], before[0])


# ---- 4
@both
@pytest.mark.parametrize("refit_boxes", [False, True], ids=["stale", "refit_boxes"])
def test_keyed_primitives_take_the_new_values_as_their_initial_transform(renderer, oracles, rt, tag, mode, refit_boxes):
    sc = scenes.moving_scene(64, 3)
    sc.scene_cam.refit_boxes = refit_boxes
    flat = upload(renderer, sc, mode)
    cam = sc.scene_cam
    shot(renderer, cam, rt)
    tree0 = renderer.export_bvh(rt)
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    keyed = [int(i) for i in idx if flat.prims[int(i)].key_count > 0]
    assert len(keyed) >= 2 and len(keyed) < len(idx)
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)
    assert_model_boxes(flat, rt, tree0, renderer.export_bvh(rt))  # construction-time boxes: the keys are not applied
    for frame in (0, 1, 2):
        cam.frame = frame
        assert_oracle(oracles, rt, flat, cam, renderer)
        assert_oracle(oracles, rt, flat, cam, renderer, A.CR_SUM_RELAXED)


# ---- 5
@both
def test_refit_of_a_tree_in_global_memory(renderer, oracles, rt, tag, mode):
    """6401 spheres: the tree does not fit LDS (RES_TOP kernels reading wrappers, or f64 screening records, through L2)."""
    sc = million_spheres(1, scene_seed=2, half_extent=40, image_width=96, samples=2)
    flat = upload(renderer, sc, mode)
    cam = sc.scene_cam
    _, st = shot(renderer, cam, rt)
    assert st["scene_in_lds"] == 2
    tree0 = renderer.export_bvh(rt)
    rs = np.random.RandomState(5)
    n = flat.desc.n_prims
    idx = (1 + np.nonzero(rs.uniform(size=n - 1) < 1.0 / 3.0)[0]).astype(np.int32)
    rows = flat._np[0]["v"][idx].copy()
    rows[:, 0] += rs.uniform(-1.5, 1.5, len(idx))
    rows[:, 1] += rs.uniform(0.0, 0.6, len(idx))
    rows[:, 2] += rs.uniform(-1.5, 1.5, len(idx))
    rows[:, 3] *= rs.uniform(0.6, 1.5, len(idx))
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)
    assert_model_boxes(flat, rt, tree0, renderer.export_bvh(rt))
    assert_oracle(oracles, rt, flat, cam, renderer)
    assert_oracle(oracles, rt, flat, cam, renderer, A.CR_SUM_RELAXED)
    _, st = shot(renderer, cam, rt)
    assert st["scene_in_lds"] == 2


# ---- 6
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_update_is_ordered_after_an_asynchronous_render(renderer, rt, tag):
    import torch
    sc = scenes.mixed_scene(256, 12)
    flat = upload(renderer, sc, A.CR_BVH_SAH)
    cam = sc.scene_cam
    pre, _ = renderer.render(cam, seed=SEED, real_type=rt)
    dt = torch.float64 if rt == A.CR_REAL_F64 else torch.float32
    t1 = torch.zeros((cam.image_height, cam.image_width, 3), dtype=dt, device="cuda:0")
    t2 = torch.zeros_like(t1)
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    assert renderer.render_device(cam, t1.data_ptr(), seed=SEED, real_type=rt) is None   # asynchronous: no stats
    renderer.update_primitives(idx, rows)
    assert renderer.render_device(cam, t2.data_ptr(), seed=SEED, real_type=rt) is None
    renderer.synchronize()
    post, _ = renderer.render(cam, seed=SEED, real_type=rt)
    assert np.array_equal(t1.cpu().numpy(), pre)
    assert np.array_equal(t2.cpu().numpy(), post)
    assert not np.array_equal(pre, post)


# ---- 7
@both
def test_frame_batch_after_an_update_equals_single_renders(renderer, rt, tag, mode):
    sc = scenes.moving_scene(64, 3)
    flat = upload(renderer, sc, mode)
    cam = sc.scene_cam
    frames = [0, 2, 1, 5]
    old, _ = renderer.render_frames(cam, frames, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    renderer.update_primitives(idx, rows)
    batch, bst = renderer.render_frames(cam, frames, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    total = dict.fromkeys(COUNTERS, 0)
    for k, f in enumerate(frames):
        cam.frame = f
        img, st = renderer.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
        assert np.array_equal(batch[k], img), (f, (batch[k] != img).any(axis=2).sum())
        for c in COUNTERS:
            total[c] += st[c]
    assert {c: bst[c] for c in COUNTERS} == total
    assert not np.array_equal(batch, old)


# ---- 8
def test_rejected_calls_change_nothing(renderer, hiplib):
    sc = scenes.mixed_scene(40, 2)
    sc.hide_element("mirror")
    flat = upload(renderer, sc, A.CR_BVH_REFERENCE)
    cam = sc.scene_cam
    kind, flags, v = um.prim_arrays(flat)
    n = len(kind)
    hidden = int(np.nonzero(flags & A.CR_PRIM_HIDDEN)[0][0])
    sphere, tri = int(np.nonzero(kind == A.CR_PRIM_SPHERE)[0][2]), int(np.nonzero(kind == A.CR_PRIM_TRIANGLE)[0][0])
    before = {rt: (shot(renderer, cam, rt), renderer.export_bvh(rt)) for rt, _ in REALS}

    def unchanged():
        for rt, _ in REALS:
            same_shot(before[rt][0], shot(renderer, cam, rt))
            same_tree(before[rt][1], renderer.export_bvh(rt))

    moved = v.copy()
    moved[:, :3] += 0.75
    bad = lambda i, k, x: np.where(np.arange(9) == k, x, moved[i])[None]   # noqa: E731
    R, B, h = A.CR_UPDATE_REFIT, A.CR_UPDATE_REBUILD, renderer.h
    cases = [
        ("n < 0", dict(idx=[sphere], rows=moved[[sphere]], n=-1), None),
        ("null v", dict(idx=[sphere], rows=None, n=1), None),
        ("unknown flags", dict(idx=[sphere], rows=moved[[sphere]], flags=2), None),
        ("negative flags", dict(idx=[sphere], rows=moved[[sphere]], flags=-1), None),
        ("index below range", dict(idx=[sphere, -1], rows=moved[[sphere, tri]]), None),
        ("index above range", dict(idx=[sphere, n], rows=moved[[sphere, tri]]), None),
        ("more rows than primitives", dict(idx=None, rows=np.concatenate([moved, moved[:1]])), None),
        ("repeated index", dict(idx=[sphere, tri, sphere], rows=moved[[sphere, tri, sphere]]), None),
        ("nan coordinate", dict(idx=[tri, sphere], rows=np.concatenate([moved[[tri]], bad(sphere, 1, np.nan)])), b"primitive coordinate is not finite"),
        ("inf coordinate", dict(idx=[tri], rows=bad(tri, 8, np.inf)), b"primitive coordinate is not finite"),
        ("-inf radius", dict(idx=[sphere], rows=bad(sphere, 3, -np.inf)), b"primitive coordinate is not finite"),
        ("negative radius", dict(idx=[tri, sphere], rows=np.concatenate([moved[[tri]], bad(sphere, 3, -0.25)])), b"Cannot make a sphere with negative radius"),
    ]
    for what, kw, msg in cases:
        for flags in (R, B):
            rc = um.update_call(hiplib, h, kw["idx"], kw["rows"], kw.get("flags", flags), n=kw.get("n"))
            assert rc == A.CR_ERR_INVALID_ARG, (what, rc)
            if msg:
                assert msg in hiplib.cr_last_error(h), (what, hiplib.cr_last_error(h))
        unchanged()
    with pytest.raises(CrucibleError) as e:
        renderer.update_primitives([sphere, sphere], moved[[sphere, sphere]])
    assert e.value.code == A.CR_ERR_INVALID_ARG
    # a hidden primitive has no device record: CR_OK, only the host copy changes ...
    assert um.update_call(hiplib, h, [hidden], moved[[hidden]], R) == A.CR_OK
    unchanged()
    # ... which a rebuild then uses: still hidden, so still the same frame and tree
    assert um.update_call(hiplib, h, [hidden], moved[[hidden]], B) == A.CR_OK
    unchanged()
    assert um.update_call(hiplib, h, None, None, R, n=0) == A.CR_OK and um.update_call(hiplib, h, None, None, B, n=0) == A.CR_OK
    unchanged()
    # the ignored tail of a sphere's row may hold anything
    assert um.update_call(hiplib, h, [sphere], np.where(np.arange(9) >= 4, np.nan, v[sphere])[None], R) == A.CR_OK
    unchanged()


def test_update_before_an_upload_is_refused(hiplib):
    r = Renderer(0)
    try:
        for flags in (A.CR_UPDATE_REFIT, A.CR_UPDATE_REBUILD):
            assert um.update_call(hiplib, r.h, None, np.zeros((1, 9)), flags) == A.CR_ERR_NO_SCENE
    finally:
        r.close()


@pytest.mark.parametrize("build", [lambda: scenes.list_scene(48, 2), lambda: scenes.wrapped_scene(48, 2)], ids=["list_scene", "wrapped_scene"])
@pytest.mark.parametrize("mode", [A.CR_BVH_REFERENCE, A.CR_BVH_SAH], ids=["reference", "sah"])
def test_scenes_with_list_elements_are_unsupported(renderer, hiplib, build, mode):
    sc = build()
    flat = upload(renderer, sc, mode)
    cam = sc.scene_cam
    kind, flags, v = um.prim_arrays(flat)
    before = shot(renderer, cam, A.CR_REAL_F32)
    plain = int(np.nonzero((kind == A.CR_PRIM_SPHERE) & (flags == 0))[0][0])       # a top-level sphere
    member = int(np.nonzero((kind <= A.CR_PRIM_TRIANGLE) & (flags & A.CR_PRIM_MEMBER != 0))[0][0])
    element = int(np.nonzero(kind >= A.CR_PRIM_LIST)[0][0])
    moved = v.copy()
    moved[:, :3] += 0.5
    for flags_ in (A.CR_UPDATE_REFIT, A.CR_UPDATE_REBUILD):
        for i in (plain, member):
            assert um.update_call(hiplib, renderer.h, [i], moved[[i]], flags_) == A.CR_ERR_UNSUPPORTED
        assert um.update_call(hiplib, renderer.h, None, moved, flags_) == A.CR_ERR_INVALID_ARG   # names the list records too
        assert um.update_call(hiplib, renderer.h, [element], moved[[element]], flags_) == A.CR_ERR_INVALID_ARG
    same_shot(before, shot(renderer, cam, A.CR_REAL_F32))


# ---- 9
@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
def test_one_member_group_update_equals_the_handle_path(renderer, hiplib, rt, tag, rebuild):
    import torch
    from crucible_amd.group import RenderGroup
    sc = scenes.mixed_scene(48, 2)
    flat = upload(renderer, sc, A.CR_BVH_SAH)
    cam = sc.scene_cam
    idx, rows = um.seeded_edit(flat, um.EDIT_SEED)
    g = RenderGroup.local([0])
    try:
        g.upload_scene(flat)
        t = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
        g.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt)
        first, _ = renderer.render(cam, seed=SEED, real_type=rt)
        assert np.array_equal(t.cpu().numpy(), first)
        # a refused call: the first member's error, nothing changed
        assert um.update_call(hiplib, g.g, [3, 3], rows[:2], A.CR_UPDATE_REFIT, group=True) == A.CR_ERR_INVALID_ARG
        assert b"twice" in hiplib.cr_group_last_error(g.g)
        g.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt)
        assert np.array_equal(t.cpu().numpy(), first)
        g.update_primitives(idx, rows, rebuild=rebuild)
        renderer.update_primitives(idx, rows, rebuild=rebuild)
        gst = g.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt)
        img, st = renderer.render(cam, seed=SEED, real_type=rt)
        assert np.array_equal(t.cpu().numpy(), img) and not np.array_equal(img, first)
        for k in COUNTERS:
            assert gst[k] == st[k], k
        host, _ = g.render(cam, seed=SEED, real_type=rt)
        assert np.array_equal(host, img)
    finally:
        g.close()
