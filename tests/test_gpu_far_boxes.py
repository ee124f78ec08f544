"""Renders of trees whose boxes leave the f32 range (tests/far_corpus.py), on every path that decides whether the f64
megakernels may screen their box tests on f32 records, and through every consumer of that decision.

The screen is usable only while no finite f64 plane of the tree is infinite in f32 (screen_plane, pathtrace.hpp).  That is
decided in four places -- at upload (build.hip finish_boxes), per render for refitted boxes (render.hip prepare_args), after
cr_update_primitives (scene.hip refit_updated) and for the frame tree of CR_REFIT_REBUILD (build.hip build_frame_scene) --
and a walk that screened on such a tree anyway would count box hits Aabb::hit does not have
(tests/test_far_boxes_host.py measures how many on these scenes).  So every render here is held to the oracle walking the
tree the handle exports: the frame byte for byte (the positions of NaNs first, where f32 makes them) and the four work
counters for equality, node_tests among them.  Nothing is compared with another device render except where a test says so."""
import numpy as np
import pytest

import far_corpus as F
import test_gpu_aov as G
import update_model as um
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from test_far_boxes_host import CAP, overflowing, same_boxes
from test_gpu_fuzz_regions_adaptive import Want, adaptive_kw, device_adaptive, pass_words, same_image
from test_gpu_region import crop

pytestmark = pytest.mark.gpu

REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
REAL_IDS = ["f64", "f32"]
DEVICE = A.CR_BVH_BUILD_DEVICE
MODES = [A.CR_BVH_REFERENCE, A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH, A.CR_BVH_SAH | DEVICE, A.CR_BVH_SAH_ORDERED | DEVICE]
MODE_IDS = ["reference", "sah", "ordered", "lbvh", "sah-device", "ordered-device"]
ORDERS = [A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_RELAXED]
RELAX = A.CR_SUM_RELAXED
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
SEED = 3838
SMALL = 4                  # CRUCIBLE_SAH_SMALL: the device builder splits these 20-odd primitives in rounds, then in wave subtrees
UPLOADS = [("far", 0), ("edge_in", 0), ("edge_out", 0), ("keyed", 0)]
UPLOAD_IDS = [n for n, _ in UPLOADS]


class Described:
    """A flattened description and its camera where a scene is expected (tests/test_gpu_aov.py's model, OracleScene)."""

    def __init__(self, flat, cam):
        self.flat, self.scene_cam = flat, cam

    def flatten(self):
        return self.flat


def upload(r, sc, mode, monkeypatch):
    if mode & DEVICE:
        monkeypatch.setenv("CRUCIBLE_SAH_SMALL", str(SMALL))
    sc.bvh_mode = mode
    flat = sc.flatten()
    r.upload_scene(flat)
    return flat


def shot(r, cam, rt, order):
    """cr_render_device into a tensor: the device form runs no Color::new check, so a frame with NaN pixels comes back."""
    import torch
    t = torch.full((cam.image_height, cam.image_width, 3), -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    st = r.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt, sum_order=order, want_stats=True)
    r.synchronize()
    return t.cpu().numpy(), st


def same_shot(a, b, what):
    same_image(a[0], b[0], what)
    for k in COUNTERS + ("bvh_entries", "scene_in_lds"):
        assert a[1][k] == b[1][k], (what, k, a[1][k], b[1][k])


def same_export(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def against_oracle(oracles, rt, flat, cam, r, order, tree=None, what=""):
    """The device's frame and counters against the oracle rendering `flat` on `tree` (default: the tree the handle exports;
    with cam.refit_boxes the oracle refits the tree it is handed, tests/test_gpu_refit.py).  Returns the frame and stats."""
    tree = r.export_bvh(rt) if tree is None else tree
    img, st = shot(r, cam, rt, order)
    ref, rst = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, tree=tree, sum_order=order)
    same_image(img, ref, what)
    for k in COUNTERS:
        assert st[k] == rst[k], (what, k, st[k], rst[k])
    return img, st


def linear_list_share(oracles, rt, flat, cam, img):
    truth, _ = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, linear_list=True)
    assert np.array_equal(np.isnan(img), np.isnan(truth))
    return ((img == truth) | np.isnan(truth)).all(axis=2).mean()


# ---------------------------------------------------------------- 1. upload: finish_boxes
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,frame", UPLOADS, ids=UPLOAD_IDS)
def test_upload(renderer, oracles, monkeypatch, name, frame, mode, rt, tag):
    """Every far scene under every tree mode and builder, both sum orders, then the linear-list cap.  "keyed" is rendered with
    its construction-time boxes here, at frame 0, during which nothing of it moves."""
    sc = F.scene(name, frame)
    cam = sc.scene_cam
    cam.refit_boxes = False
    flat = upload(renderer, sc, mode, monkeypatch)
    boxes = renderer.export_bvh(rt)[0]
    if rt == A.CR_REAL_F64:
        assert overflowing(boxes).any() == (name in ("far", "edge_out"))   # the screen is off exactly for these two
    img, _ = against_oracle(oracles, rt, flat, cam, renderer, A.CR_SUM_REFERENCE_ORDER, what=f"{name} {tag}")
    against_oracle(oracles, rt, flat, cam, renderer, RELAX, what=f"{name} {tag} relaxed")
    share = linear_list_share(oracles, rt, flat, cam, img)
    print(f"{name} {MODE_IDS[MODES.index(mode)]} {tag}: {share:.5f} of the pixels equal the linear list's")
    assert share >= CAP, share


# ---------------------------------------------------------------- 2. the boundary pair
@pytest.mark.parametrize("order", ORDERS, ids=["reference-order", "relaxed"])
@pytest.mark.parametrize("mode", [A.CR_BVH_REFERENCE, A.CR_BVH_SAH_ORDERED], ids=["reference", "ordered"])
def test_boundary_pair(renderer, oracles, monkeypatch, mode, order):
    """FLT_MAX as the largest plane leaves the screen usable, the smallest double that rounds to infinity does not: the two
    trees have the same topology and differ in that plane alone, and both f64 frames are the oracle's."""
    rt = A.CR_REAL_F64
    trees = {}
    for name in ("edge_in", "edge_out"):
        sc = F.scene(name)
        flat = upload(renderer, sc, mode, monkeypatch)
        trees[name] = renderer.export_bvh(rt)
        assert trees[name][0].max() == F.largest_plane(name)
        against_oracle(oracles, rt, flat, sc.scene_cam, renderer, order, what=name)
    assert not overflowing(trees["edge_in"][0]).any() and overflowing(trees["edge_out"][0]).any()
    assert np.array_equal(trees["edge_in"][1], trees["edge_out"][1])
    a, b = trees["edge_in"][0], trees["edge_out"][0]
    assert np.array_equal(a == F.largest_plane("edge_in"), b == F.largest_plane("edge_out")) and np.array_equal(a[a != a.max()], b[b != b.max()])


# ---------------------------------------------------------------- 3. residency, and the screen switched off
@pytest.mark.parametrize("order", ORDERS, ids=["reference-order", "relaxed"])
@pytest.mark.parametrize("where", ["lds", "global-memory", "no-screen"])
@pytest.mark.parametrize("name", ["far", "edge_in"])
def test_residency(oracles, monkeypatch, name, where, order):
    """The f64 scene whole in LDS as it falls, with the tree pushed to global memory, and with CRUCIBLE_SCREEN=0 (fresh
    handles: the knobs are read in cr_create): each is the oracle's frame with the oracle's counters, for the tree that must
    not be screened and for the one that may."""
    rt = A.CR_REAL_F64
    if where == "global-memory":
        monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
        monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    if where == "no-screen":
        monkeypatch.setenv("CRUCIBLE_SCREEN", "0")
    r = Renderer(0)
    try:
        sc = F.scene(name)
        flat = upload(r, sc, A.CR_BVH_SAH, monkeypatch)
        _, st = against_oracle(oracles, rt, flat, sc.scene_cam, r, order, what=f"{name} {where}")
        assert st["scene_in_lds"] == (0 if where == "global-memory" else 1)
    finally:
        r.close()


# ---------------------------------------------------------------- 4. refit: decided per render, not sticky
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("order", ORDERS, ids=["reference-order", "relaxed"])
@pytest.mark.parametrize("mode", MODES[:4], ids=MODE_IDS[:4])
def test_refit_is_decided_per_render(renderer, oracles, monkeypatch, mode, order, rt, tag):
    """One handle, refit_boxes = 1: frame 0 (no plane beyond the range), frame 1 (the rovers' boxes beyond it), frame 0 again,
    frame 2, each against the oracle's refit of that frame on the exported topology; the two renders of frame 0 are byte for
    byte the same.  Then refit_boxes = 0: the stale boxes, still the oracle's."""
    sc = F.scene("keyed")
    cam = sc.scene_cam
    flat = upload(renderer, sc, mode, monkeypatch)
    base = renderer.export_bvh(rt)
    shots = []
    for frame in (0, F.KEYED_FAR_FRAME, 0, 2):
        cam.frame = frame
        shots.append(against_oracle(oracles, rt, flat, cam, renderer, order, tree=base, what=f"refit frame {frame} {tag}"))
        walked = renderer.export_render_bvh(rt)
        assert np.array_equal(walked[1], base[1]) and not np.array_equal(walked[0], base[0])
        if rt == A.CR_REAL_F64:
            assert overflowing(walked[0]).any() == (frame == F.KEYED_FAR_FRAME)
        assert same_export(renderer.export_bvh(rt), base)
    same_shot(shots[0], shots[2], "frame 0 before and after the far frame")
    assert not np.array_equal(shots[0][0], shots[1][0])
    cam.refit_boxes = False
    for frame in (F.KEYED_FAR_FRAME, 0):
        cam.frame = frame
        against_oracle(oracles, rt, flat, cam, renderer, order, tree=base, what=f"stale frame {frame} {tag}")
        assert same_export(renderer.export_render_bvh(rt), base)


# ---------------------------------------------------------------- 5. cr_update_primitives: refit_updated
def model_of(flat, rt, children):
    kind, _, v = um.prim_arrays(flat)
    return um.model_boxes(children, kind, v, np.float64 if rt == A.CR_REAL_F64 else np.float32).astype(np.float64)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_update_refit_round_trip(renderer, oracles, monkeypatch, mode):
    """The hostile edit (CR_UPDATE_REFIT) on "near" with both precisions built: same topology, the boxes of the numpy model
    (NaN planes where f32 has inf - inf), the oracle's frame on the exported tree under both sum orders; the f64 tree now has
    planes beyond the f32 range.  The inverse edit brings export and frames back byte for byte: screen_usable went from true
    to false and to true again.
    The f32 half is what showed two things about a plane that is inf - inf (the row with centre DBL_MAX and radius 1e300):
    the refit dropped that sphere's box where a build keeps it, and with the box kept the min/max form of the box test
    reached fewer leaves than Aabb::hit (prim_tests 13023 against the oracle's 16659 under CR_BVH_SAH, frames equal).  Such a
    tree is now walked with Aabb::hit's own form (KernelArgs::exact_boxes)."""
    sc = F.scene("near")
    cam = sc.scene_cam
    flat = upload(renderer, sc, mode, monkeypatch)
    idx, rows, back = F.hostile_edit(flat)
    before = {}
    for rt, tag in REALS:
        shots = [against_oracle(oracles, rt, flat, cam, renderer, order, what=f"before {tag}") for order in ORDERS]
        before[rt] = (renderer.export_bvh(rt), shots)
    assert not overflowing(before[A.CR_REAL_F64][0][0]).any()
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)
    for rt, tag in REALS:
        tree = renderer.export_bvh(rt)
        assert np.array_equal(tree[1], before[rt][0][1]) and np.array_equal(tree[2], before[rt][0][2])
        same_boxes(tree[0], model_of(flat, rt, tree[1]), f"edited {tag}")
        if rt == A.CR_REAL_F64:
            assert overflowing(tree[0]).any() and not np.isnan(tree[0]).any()
        else:
            assert np.isinf(tree[0]).any()
        for k, order in enumerate(ORDERS):
            img, _ = against_oracle(oracles, rt, flat, cam, renderer, order, tree=tree, what=f"edited {tag}")
            assert not np.array_equal(img, before[rt][1][k][0])
    renderer.update_primitives(idx, back)
    um.apply_edit(flat, idx, back)
    for rt, tag in REALS:
        assert same_export(renderer.export_bvh(rt), before[rt][0]), tag
        for k, order in enumerate(ORDERS):
            same_shot(shot(renderer, cam, rt, order), before[rt][1][k], f"restored {tag}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_update_rebuild_is_a_fresh_upload(renderer, monkeypatch, mode):
    """The hostile edit with CR_UPDATE_REBUILD: export bytes, frame and counters of a fresh upload of the edited description,
    in both precisions, under every builder."""
    sc = F.scene("near")
    cam = sc.scene_cam
    flat = upload(renderer, sc, mode, monkeypatch)
    idx, rows, _ = F.hostile_edit(flat)
    for rt, _ in REALS:
        shot(renderer, cam, rt, RELAX)
    renderer.update_primitives(idx, rows, rebuild=True)
    um.apply_edit(flat, idx, rows)
    fresh = Renderer(0)
    try:
        fresh.upload_scene(flat)
        for rt, tag in REALS:
            for order in ORDERS:
                same_shot(shot(renderer, cam, rt, order), shot(fresh, cam, rt, order), f"rebuilt {tag}")
            assert same_export(renderer.export_bvh(rt), fresh.export_bvh(rt)), tag
    finally:
        fresh.close()


# ---------------------------------------------------------------- 6. the frame tree of CR_REFIT_REBUILD: build_frame_scene
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH, A.CR_BVH_SAH | DEVICE], ids=["sah", "sah-device"])
def test_frame_tree(renderer, oracles, monkeypatch, mode, rt, tag):
    """refit_boxes = "rebuild" on "keyed": the far frame and then the near frame, each the oracle's on the tree
    cr_export_render_bvh returns; an update then drops the frame tree, and the next render is the oracle's of the edited
    description on its new frame tree."""
    sc = F.scene("keyed", F.KEYED_FAR_FRAME)
    cam = sc.scene_cam
    flat = upload(renderer, sc, mode, monkeypatch)

    def frame_render(order, what):
        cam.refit_boxes = "rebuild"
        img, st = shot(renderer, cam, rt, order)
        tree = renderer.export_render_bvh(rt)
        assert renderer.frame_build_info(rt)["n_wrappers"] == len(tree[1]) > 0
        cam.refit_boxes = True                                                # the oracle refits the tree it is handed
        ref, rst = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, tree=tree, sum_order=order)
        same_image(img, ref, what)
        for k in COUNTERS:
            assert st[k] == rst[k], (what, k, st[k], rst[k])
        return tree

    for order in ORDERS:
        far = frame_render(order, f"far frame {tag}")
    if rt == A.CR_REAL_F64:
        assert overflowing(far[0]).any()
    cam.frame = 0
    near = frame_render(A.CR_SUM_REFERENCE_ORDER, f"near frame {tag}")
    if rt == A.CR_REAL_F64:
        assert not overflowing(near[0]).any()
    idx = np.array([2, 1 + F.N_SPHERES], dtype=np.int32)                      # a sphere and a triangle of the cluster
    rows = np.array([list(flat.prims[int(i)].v) for i in idx], dtype=np.float64)
    rows[:, 0:3] += (0.4, -0.3, 0.5)
    rows[1, 3:6] += (0.4, -0.3, 0.5)
    rows[1, 6:9] += (0.4, -0.3, 0.5)
    renderer.update_primitives(idx, rows)
    assert renderer.frame_build_info(rt)["n_wrappers"] == 0                  # drop_frame_trees
    um.apply_edit(flat, idx, rows)
    cam.frame = F.KEYED_FAR_FRAME
    frame_render(A.CR_SUM_REFERENCE_ORDER, f"far frame after the update {tag}")


# ---------------------------------------------------------------- 7. the consumers
def handle_state(r, state, monkeypatch):
    """(description, camera): "far" uploaded as it is under the reference tree, or "near" under CR_BVH_SAH with the hostile
    edit applied by CR_UPDATE_REFIT after both precisions were built."""
    if state == "far":
        sc = F.scene("far")
        return upload(r, sc, A.CR_BVH_REFERENCE, monkeypatch), sc.scene_cam
    sc = F.scene("near")
    flat = upload(r, sc, A.CR_BVH_SAH, monkeypatch)
    for rt, _ in REALS:
        shot(r, sc.scene_cam, rt, RELAX)                                      # both precisions built: the update refits both
    idx, rows, _ = F.hostile_edit(flat)
    r.update_primitives(idx, rows)
    return um.apply_edit(flat, idx, rows), sc.scene_cam


STATES = ["far", "updated"]


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("state", STATES)
def test_regions(renderer, oracles, monkeypatch, state, rt, tag):
    """A 2 x 2 partition (13 | 19 columns, 10 | 14 rows): every crop is the whole frame's and the relaxed oracle's, the
    counters add up to the frame's and to the oracle's."""
    flat, cam = handle_state(renderer, state, monkeypatch)
    W, H = cam.image_width, cam.image_height
    tree = renderer.export_bvh(rt)
    full, fst = shot(renderer, cam, rt, RELAX)
    ref, rst = um.oracle_render_flat(oracles[rt], flat, cam, seed=SEED, tree=tree, sum_order=RELAX)
    same_image(full, ref, f"{state} {tag}")
    tot = dict.fromkeys(COUNTERS + ("samples",), 0)
    import torch
    for reg in [(0, 0, 13, 10), (13, 0, W - 13, 10), (0, 10, 13, H - 10), (13, 10, W - 13, H - 10)]:
        d = torch.full((reg[3], reg[2], 3), -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        st = renderer.render_region_device(cam, reg, d.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX, want_stats=True)
        renderer.synchronize()
        same_image(d.cpu().numpy(), crop(ref, reg), f"{state} {tag} region {reg}")
        for c in tot:
            tot[c] += st[c]
    for c in COUNTERS:
        assert tot[c] == fst[c] == rst[c], (c, tot[c], fst[c], rst[c])
    assert tot["samples"] == W * H * cam.samples


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("state", STATES)
def test_guide_layers(renderer, oracles, monkeypatch, state, rt, tag):
    flat, cam = handle_state(renderer, state, monkeypatch)
    got, st = renderer.render_aov(cam, seed=SEED, real_type=rt)
    want, _ = G.model(oracles[rt], Described(flat, cam), SEED, tree=renderer.export_bvh(rt))
    G.same(got, want, f"{state} {tag}")
    assert st["samples"] == cam.image_width * cam.image_height * cam.samples == st["segments"]
    if state == "far" and rt == A.CR_REAL_F64:
        assert np.isfinite(got["depth"]).any() and 0 < got["coverage"].mean() < 1


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("state", STATES)
def test_adaptive(renderer, oracles, monkeypatch, state, rt, tag):
    """8 samples in passes of 2, judged from 4 on, blocks of 8 pixels, the median tolerance: counts and frame are those of
    tests/adaptive_model.py fed with the oracle's per-pass words on the exported tree."""
    flat, cam = handle_state(renderer, state, monkeypatch)
    cam.set_samples(8)
    P, min_samples, block = 2, 4, 8
    words = pass_words(oracles[rt], Described(flat, cam), SEED, P, flat=flat, tree=renderer.export_bvh(rt))
    want = Want(words, P, min_samples, block, np.float64 if rt == A.CR_REAL_F64 else np.float32)
    assert len(np.unique(want.counts)) >= 2                                  # blocks that stop early and blocks that do not
    img, counts, st = device_adaptive(renderer, cam, **adaptive_kw(rt, SEED, want.tol, P, min_samples, block))
    assert np.array_equal(counts, want.counts), f"{int((counts != want.counts).sum())} counts differ"
    same_image(img, want.frame, f"{state} {tag}")
    assert st["blocks"] == want.blocks and st["blocks_stopped"] == want.stopped and st["render"]["samples"] == want.samples


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
def test_frame_batch(renderer, oracles, monkeypatch, rt, tag):
    """Frames 0, 1, 2 of "keyed" in one launch, construction-time boxes: each frame is its single render and the oracle's,
    and the counters add up."""
    import torch
    sc = F.keyed_scene(0, refit=False)
    cam = sc.scene_cam
    flat = upload(renderer, sc, A.CR_BVH_SAH, monkeypatch)
    tree = renderer.export_bvh(rt)
    frames = list(F.KEYED_FRAMES)
    d = torch.full((len(frames), cam.image_height, cam.image_width, 3), -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    bst = renderer.render_frames_device(cam, frames, d.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX, want_stats=True)
    renderer.synchronize()
    batch = d.cpu().numpy()
    tot = dict.fromkeys(COUNTERS, 0)
    for k, f in enumerate(frames):
        cam.frame = f
        img, st = against_oracle(oracles, rt, flat, cam, renderer, RELAX, tree=tree, what=f"frame {f} {tag}")
        same_image(batch[k], img, f"batch entry {k} {tag}")
        for c in COUNTERS:
            tot[c] += st[c]
    for c in COUNTERS:
        assert bst[c] == tot[c], (c, bst[c], tot[c])
