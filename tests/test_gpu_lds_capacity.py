"""Scenes that fill the LDS to the byte, rendered on every path that stages a scene there.

How much of a scene a launch stages is settled by byte comparisons against 160 KB: render.hip render_typed (scene +
fx_lds_bytes(1024, 4) <= lds_limit), aov.hip aov_typed (scene + aov_lds_bytes(1024)), launch_plan.hpp plan_tile (the tile
falls back to 4 x 4 once fx_off + slots > 160 KB), residency.hpp choose_residency (the window, the side tables' 16 KB, the
6-waves entry point's third of a CU) and alt_pipelines.hip (the wavefront's geometry-only layout, the queue's state).
tests/lds_capacity.py restates the arithmetic and builds, per comparison, the largest scene that passes it ("at") and the
smallest that does not ("over"); tests/test_lds_capacity_host.py holds that arithmetic to the headers.  Here every case

  * uploads its scene and renders 32 x 20 pixels,
  * compares the output and segments, node_tests, prim_tests, texel_fetches bit for bit with the oracle in the same sum
    order (the relaxed oracle of tests/test_gpu_relaxed.py, the guide model of tests/test_gpu_aov.py),
  * asserts bvh_entries == tree_size(n) on the reference tree, and
  * asserts that scene_in_lds is the helper's prediction: 1 (RES_LDS) at, 2 (RES_TOP) over.

What a case would catch is named in its test's docstring.  An "at" scene's last material, last texture and last primitive
are all read by camera rays (tests/test_lds_capacity_host.py proves it on the CPU), so a table whose last 16 bytes are not
staged, or a link rewritten wrongly beyond 64 KB, changes the frame; a launch that asks one record too much is refused
(CR_ERR_HIP); a threshold off by one slot size flips scene_in_lds of the "at" or the "over" scene.

Each case prints one "LDSCAP" line: row, threshold, (n, wrappers, materials, textures), layout bytes, the launch's dynamic
LDS at a 1024-thread block, scene_in_lds, seconds."""
import copy
import os
import time

import numpy as np
import pytest

import lds_capacity as K
import test_gpu_aov as G
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from test_gpu_relaxed import COUNTERS, relaxed_oracle

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
RELAX, REFERENCE = A.CR_SUM_RELAXED, A.CR_SUM_REFERENCE_ORDER
ORDERED = A.CR_BVH_SAH_ORDERED
TINY_WINDOW = {"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "1"}
LATENCY = {"CRUCIBLE_LATENCY_ENTRIES": "1", "CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LATENCY_TOP_KB": "32"}


# ---------------------------------------------------------------------------------------------------- handles and references
@pytest.fixture(scope="module")
def handle(hiplib):
    """handle(env) -> the Renderer created under that environment (the knobs are read in cr_create), one per environment,
    closed when the module is done"""
    made = {}

    def get(env=None):
        key = tuple(sorted((env or {}).items()))
        if key not in made:
            saved = {k: os.environ.get(k) for k, _ in key}
            os.environ.update(dict(key))
            try:
                made[key] = Renderer(0)
            finally:
                for k, v in saved.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[key]
    yield get
    for r in made.values():
        r.close()


_references = {}


def reference(key, make):
    """An oracle result, computed once per key and shared by the cases that need it"""
    if key not in _references:
        _references[key] = make()
    return _references[key]


def scene_key(sc):
    return (sc.shape, sc.bvh_mode, bool(sc.flatten().desc.n_keys))


def oracle_frame(oracle, sc, order, tree=None, **kw):
    cam = sc.scene_cam
    key = ("frame", scene_key(sc), oracle.real_type, order, cam.samples, cam.frame, tuple(sorted(kw.items())))
    if order == RELAX:
        return reference(key, lambda: relaxed_oracle(oracle, sc, seed=SEED, tree=tree, **kw))
    return reference(key, lambda: oracle.render_image(sc, seed=SEED, tree=tree, **kw))


def oracle_guide(oracle, sc, tree=None):
    """The guide model's planes, and the counters of the same primary rays: a depth-1 render's"""
    cam = sc.scene_cam

    def make():
        planes, _ = G.model(oracle, sc, SEED, tree=tree)
        depth = cam.max_depth
        cam.set_max_depth(1)
        try:
            _, st = oracle.render_image(sc, seed=SEED, tree=tree)
        finally:
            cam.set_max_depth(depth)
        return planes, st
    return reference(("guide", scene_key(sc), oracle.real_type, cam.samples), make)


def same_frame(img, st, ref, rst):
    assert img.dtype == ref.dtype and img.shape == ref.shape
    assert np.array_equal(img, ref, equal_nan=True), f"differing px = {(img != ref).any(axis=-1).sum()}"
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])


def launch_bytes(row, shape, wrappers, kind, spp, res):
    """The dynamic LDS the launch asks for at a block of 1024 threads (a smaller block has fewer waves' slots): the staged
    scene, or the window with the side tables that ride along, and the slots behind it."""
    row = K.ROWS[row]
    n, m, t = shape
    s = K.SIZES[row.rt]
    if res == 1:
        scene = K.layout_of(row, n, wrappers, m, t)
    else:
        rec = s["screen_o"] if row.ordered and row.rt == K.F64 else (s["entry_o"] if row.ordered else 32)
        scene = min(wrappers, K.WINDOW // rec) * rec
        side = K.side_table_bytes(row.rt, m, t)
        if not row.ordered and side <= K.SIDE_LIMIT:
            scene = K.r16(scene) + side
    if kind == "guide":
        return K.r16(scene) + K.aov_lds_bytes(K.MAX_BLOCK)
    if kind == "reference":
        return scene
    tile = 6 if spp == 1 else (5 if spp < 4 else 4)
    if K.r16(scene) + K.fx_lds_bytes(K.MAX_BLOCK, tile) > K.LDS:
        tile = 4
    return K.r16(scene) + K.fx_lds_bytes(K.MAX_BLOCK, tile)


def run_case(r, oracles, row, sc, kind, want_res, label, threshold, wrappers=None):
    """Upload, render (kind: "reference", "relaxed", "guide"), compare with the oracle, check bvh_entries and scene_in_lds."""
    row_ = K.ROWS[row]
    rt, o, cam = row_.rt, oracles[row_.rt], sc.scene_cam
    t0 = time.time()
    r.upload_scene(sc.flatten())
    tree = r.export_bvh(rt) if row_.ordered else None
    if kind == "guide":
        got, st = r.render_aov(cam, seed=SEED, real_type=rt)
        want, rst = oracle_guide(o, sc, tree)
        assert sorted(got) == sorted(G.NAMES)
        G.same(got, want, label)
        for k in COUNTERS:
            assert st[k] == rst[k], (k, st[k], rst[k])
    else:
        order = RELAX if kind == "relaxed" else REFERENCE
        img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=order)
        same_frame(img, st, *oracle_frame(o, sc, order, tree))
    n = sc.shape[0]
    if wrappers is None:
        wrappers = K.tree_size(n)
    assert st["bvh_entries"] == wrappers
    assert st["samples"] == cam.image_width * cam.image_height * cam.samples and st["nan_pixels"] == 0
    log(label, row, threshold, sc, wrappers, kind, cam.samples, st["scene_in_lds"], t0)
    assert st["scene_in_lds"] == want_res, (st["scene_in_lds"], want_res)
    return st


def log(label, row, threshold, sc, wrappers, kind, spp, res, t0):
    n, m, t = sc.shape
    print(f"LDSCAP {label} row={row} threshold={threshold} scene=({n}, {wrappers}, {m}, {t}) layout={K.layout_of(row, n, wrappers, m, t)} "
          f"launch={launch_bytes(row, sc.shape, wrappers, kind, spp, res)} scene_in_lds={res} seconds={time.time() - t0:.2f}")


# ---------------------------------------------------------------------------------------------------- scenes per row
_ordered = {}


def ordered_found(r, row, threshold, over):
    """An ordered tree's wrapper count is the builder's: upload, read it, and pick the sphere count and the fillers from it.
    The layout lands within one side record's bytes of the threshold (the fillers' step)."""
    key = (row, threshold, over)
    if key in _ordered:
        return _ordered[key]
    row_ = K.ROWS[row]
    s = K.SIZES[row_.rt]
    n = K.find("f32" if row_.rt == K.F32 else "f64", threshold)[0].n
    found = None
    for _ in range(6):
        sc = K.capacity_scene(n, K.MIN_MATS, K.MIN_TEXS, bvh_mode=ORDERED)
        r.upload_scene(sc.flatten())
        w = r.build_info(row_.rt)["n_wrappers"]
        found = K.fit_fillers(row, n, w, threshold, over)
        if found and abs(found.bytes - threshold) <= s["tex"]:
            break
        found = None
        base = K.layout_of(row, n, w, K.MIN_MATS, K.MIN_TEXS)
        n += int(round((threshold - 32 * s["tex"] - base) / (s["prim"] + s[row_.record] * w / n)))
    assert found, "no ordered scene near the threshold"
    gap = found.bytes - threshold
    assert (0 < gap <= s["tex"]) if over else (-s["tex"] < gap <= 0)
    _ordered[key] = found
    return found


def pair_scene(r, row, name, which, **kw):
    """(scene, its Found, the threshold) of row at the named threshold; which: "at" or "over" """
    threshold = K.THRESHOLDS[name]
    if K.ROWS[row].ordered:
        f = ordered_found(r, row, threshold, which == "over")
        return K.scene_of(f, bvh_mode=ORDERED, **kw), f, threshold
    f = K.find(row, threshold)[which == "over"]
    return K.scene_of(f, **kw), f, threshold


# ---------------------------------------------------------------------------------------------------- A. the three thresholds
@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("kind", ["reference", "relaxed", "guide"])
@pytest.mark.parametrize("row", list(K.ROWS))
def test_threshold(handle, oracles, row, kind, which):
    """render.hip:240-242 (reference order: the scene alone against 163840; relaxed: + 12288) and aov.hip:123-125 (+ 16384):
    `<=` written `<`, or a slot size off by one record, turns the "at" scene's 1 into 2; the other way round the "over"
    scene's launch asks more than a CU has and is refused.  stage_scene (megakernel.hpp) copying a table short by its last
    16 bytes, or a link rewritten to a wrong LDS address past 64 KB, changes the "at" frame: its last material and texture
    are the ground's, its last primitive the marker."""
    r = handle(K.ROWS[row].env)
    sc, f, threshold = pair_scene(r, row, kind, which, samples=4 if kind == "guide" else 3)
    run_case(r, oracles, row, sc, kind, 2 if which == "over" else 1, f"A-{kind}-{which}", threshold, f.wrappers)


@pytest.mark.parametrize("kind,name,which,want", [("guide", "relaxed", "at", 2), ("relaxed", "guide", "over", 1)],
                         ids=["guide-of-the-relaxed-at-scene", "render-of-the-guide-over-scene"])
def test_one_scene_two_residencies(handle, oracles, kind, name, which, want):
    """A guide pass and a render that disagree about the same scene: the scene that just fits beside the relaxed sums' slots
    does not fit beside the guide slots, and the one 16 bytes too large for the guide pass fits the render.  Both exact."""
    r = handle()
    sc, f, threshold = pair_scene(r, "f64", name, which, samples=4 if kind == "guide" else 3)
    run_case(r, oracles, "f64", sc, kind, want, f"A-cross-{kind}", K.THRESHOLDS[kind], f.wrappers)


# ---------------------------------------------------------------------------------------------------- B. the other doors
def door_frames(r, o, rt, sc):
    cam = sc.scene_cam
    got, st = r.render_frames(cam, [0, 1], seed=SEED, real_type=rt, sum_order=RELAX)
    total = dict.fromkeys(COUNTERS, 0)
    for k in (0, 1):
        cam.frame = k
        try:
            ref, rst = oracle_frame(o, sc, RELAX)
        finally:
            cam.frame = 0
        assert np.array_equal(got[k], ref), k
        for c in COUNTERS:
            total[c] += rst[c]
    return st, total


def door_views(r, o, rt, sc):
    cam = sc.scene_cam
    other = copy.deepcopy(cam)
    other.look_from((1.5, 3.0, 8.5))
    got, st = r.render_views([cam, other], seed=SEED, real_type=rt, sum_order=RELAX)
    total = dict.fromkeys(COUNTERS, 0)
    for k, c in enumerate((cam, other)):
        sc.scene_cam = c
        try:
            ref, rst = reference(("view", scene_key(sc), rt, k, cam.samples), lambda: relaxed_oracle(o, sc, seed=SEED))
        finally:
            sc.scene_cam = cam
        assert np.array_equal(got[k], ref), k
        for name in COUNTERS:
            total[name] += rst[name]
    return st, total


REGION = (5, 3, 9, 7)   # no side on a multiple of the 4-, 8-pixel tiles


def door_region(r, o, rt, sc):
    cam = sc.scene_cam
    x0, y0, w, h = REGION
    got, st = r.render_region(cam, REGION, seed=SEED, real_type=rt, sum_order=RELAX)

    def make():
        rows, total = [], dict.fromkeys(COUNTERS, 0)
        hs = o.scene_create(sc.flatten())
        try:
            for j in range(y0, y0 + h):
                px, rst = o.render(hs, cam, seed=SEED, pix_begin=j * cam.image_width + x0, pix_end=j * cam.image_width + x0 + w, sum_order=RELAX)
                rows.append(px)
                for c in COUNTERS:
                    total[c] += rst[c]
        finally:
            o.scene_destroy(hs)
        return np.stack(rows), total
    ref, total = reference(("region", scene_key(sc), rt, cam.samples), make)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    return st, total


def door_adaptive(r, o, rt, sc):
    """min_samples = samples: no block stops, two passes of two samples, the plain frame (tests/test_gpu_adaptive.py)"""
    cam = sc.scene_cam
    img, counts, st = r.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=0.5, min_samples=4, pass_samples=2, block=8, sum_order=RELAX)
    ref, rst = oracle_frame(o, sc, RELAX)
    assert st["passes"] == 2 and (counts == 4).all() and np.array_equal(img, ref)
    return st["render"], rst


def door_anim(r, o, rt, sc):
    cam = sc.scene_cam
    img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    ref, rst = oracle_frame(o, sc, RELAX)
    assert np.array_equal(img, ref)
    return st, rst


def door_quiet(r, o, rt, sc):
    """pathtrace_kernel_quiet at the limit: the frame without stats is the oracle's; scene_in_lds from the counted twin"""
    cam = sc.scene_cam
    quiet, none = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, want_stats=False)
    assert not any(none[k] for k in COUNTERS)
    ref, rst = oracle_frame(o, sc, RELAX)
    assert np.array_equal(quiet, ref)
    counted, st = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, want_stats=True)
    assert np.array_equal(counted, ref)
    return st, rst


DOORS = {"frames": door_frames, "views": door_views, "region": door_region, "adaptive": door_adaptive, "anim": door_anim, "quiet": door_quiet}
DOOR_CASES = [(row, door) for row in ("f64", "f32") for door in DOORS if not (door == "quiet" and row == "f32")]


@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("row,door", DOOR_CASES, ids=[f"{row}-{door}" for row, door in DOOR_CASES])
def test_other_doors(handle, oracles, row, door, which):
    """Frames, views, regions and adaptive passes share launch() and render_typed's comparison with the plain render, but run
    other kernels (CAMK, the views' kernels, the listed kernel, ANIM for a keyed sphere, the quiet twin): each stages the
    scene through its own instantiation of stage_scene, at the relaxed threshold of 151552 bytes."""
    r = handle()
    rt = K.ROWS[row].rt
    samples = 4 if door == "adaptive" else 3
    sc, f, threshold = pair_scene(r, row, "relaxed", which, samples=samples, keyed=door == "anim")
    t0 = time.time()
    r.upload_scene(sc.flatten())
    st, want = DOORS[door](r, oracles[rt], rt, sc)
    for k in COUNTERS:
        assert st[k] == want[k], (k, st[k], want[k])
    assert st["bvh_entries"] == K.tree_size(f.n) == f.wrappers
    log(f"B-{door}-{which}", row, threshold, sc, f.wrappers, "relaxed", samples, st["scene_in_lds"], t0)
    assert st["scene_in_lds"] == (2 if which == "over" else 1)


# ---------------------------------------------------------------------------------------------------- C. the tile fallback
TILE_CASES = [("tile8x8", "at", 1), ("tile8x8", "over", 1), ("tile8x4", "at", 2), ("tile8x4", "over", 2), ("tile8x4", "at", 3), ("tile8x4", "over", 3),
              ("relaxed", "at", 1)]


@pytest.mark.parametrize("name,which,spp", TILE_CASES, ids=[f"{n}-{w}-{s}spp" for n, w, s in TILE_CASES])
@pytest.mark.parametrize("row", ["f64", "f32"])
def test_tile_fallback(handle, oracles, row, name, which, spp):
    """launch_plan.hpp plan_tile: fx_off + the slots of the 8 x 8 (1 spp) or 8 x 4 (2-3 spp) tile against 160 KB.  The scene
    "at" keeps the wide tile and its launch is 163840 bytes; the scene "over" falls back to 4 x 4.  The chosen tile is not
    observable and the frame does not depend on it, so a wrong threshold shows as a refused launch (one slot too many) or,
    where fx_lds_off and the launch's bytes disagree, as a wrong frame; the relaxed "at" scene at 1 spp has the least room."""
    r = handle()
    sc, f, threshold = pair_scene(r, row, name, which, samples=spp)
    run_case(r, oracles, row, sc, "relaxed", 1, f"C-{name}-{which}-{spp}spp", threshold, f.wrappers)


# ---------------------------------------------------------------------------------------------------- D. the default window
@pytest.mark.parametrize("kind,spp", [("reference", 1), ("relaxed", 1), ("relaxed", 4)], ids=["reference-1spp", "relaxed-1spp", "relaxed-4spp"])
@pytest.mark.parametrize("n", [4096, 4097])
@pytest.mark.parametrize("row", ["f64", "f32"])
def test_default_window(handle, oracles, row, n, kind, spp):
    """RES_TOP without knobs: a 128 KB window of 4096 32-byte records.  4096 spheres make 4095 wrappers, the whole tree in
    the window with the primitives in global memory; 4097 make 4097, one record outside it (residency.hpp:89-90: a window
    one record short or long reads a neighbour's bytes as a box).  Wrapper counts are odd, so no reference tree equals the
    window exactly.  Relaxed at 1 spp: window + side tables leave no room for the 8 x 8 tile's slots (the fallback tile)."""
    sc = K.capacity_scene(n, K.MIN_MATS, K.MIN_TEXS, samples=spp)
    assert K.tree_size(4096) == 4095 and K.tree_size(4097) == 4097
    run_case(handle(), oracles, row, sc, kind, 2, f"D-window-{n}-{kind}-{spp}spp", K.WINDOW)


@pytest.mark.parametrize("n_texs,side", [(256, 16384), (257, 16416)], ids=["side-16384", "side-16416"])
def test_default_window_full_side_tables(handle, oracles, n_texs, side):
    """residency.hpp:103: side tables of exactly lds_side_limit ride behind the window, and the guide pass's launch is
    131072 + 16384 + 16384 = 163840 bytes; 32 bytes more and they stay in global memory."""
    assert K.side_table_bytes(K.F32, 256, n_texs) == side
    sc = K.capacity_scene(4097, 256, n_texs, samples=4)
    run_case(handle(), oracles, "f32", sc, "guide", 2, f"D-side-{side}", K.SIDE_LIMIT)


@pytest.mark.parametrize("kind", ["reference", "relaxed"])
@pytest.mark.parametrize("env,n", [({}, 32), ({}, 33), ({}, 34), ({"CRUCIBLE_SCREEN": "0"}, 16), ({"CRUCIBLE_SCREEN": "0"}, 17), ({"CRUCIBLE_SCREEN": "0"}, 18)],
                         ids=["screen-32", "screen-33", "screen-34", "wrappers-16", "wrappers-17", "wrappers-18"])
def test_tiny_window(handle, oracles, env, n, kind):
    """A 1 KB window: 32 screening records or 16 wrappers of 64 bytes.  31, 33, 35 (15, 17, 19) wrappers: the tree inside the
    window, one record and three records outside it."""
    sc = K.capacity_scene(n, K.MIN_MATS, K.MIN_TEXS, samples=3)
    run_case(handle({**TINY_WINDOW, **env}), oracles, "f64" if not env else "f64-wrappers", sc, kind, 2, f"D-tiny-{n}-{kind}", 1024)


# ---------------------------------------------------------------------------------------------------- E. the 6-waves entry point
@pytest.mark.parametrize("kind", ["reference", "relaxed"])
@pytest.mark.parametrize("n_texs,side", [(245, 15680), (246, 15712)], ids=["side-15680", "side-15712"])
def test_latency_entry_side_tables(handle, oracles, n_texs, side, kind):
    """residency.hpp:100-103: three 512-thread groups share a CU, so the side tables ride along up to
    163840 / 3 - 16 - 32768 - 6144 = 15685 bytes: 15680 do (three groups of 54592 bytes fill a CU to 163776), 15712 do not."""
    cap = K.LDS // 3 - 16 - 32768 - K.fx_lds_bytes(512, 4)
    assert cap == 15685 and K.side_table_bytes(K.F32, 245, n_texs) == side and (side <= cap) == (n_texs == 245)
    sc = K.capacity_scene(4097, 245, n_texs, samples=3)
    run_case(handle(LATENCY), oracles, "f32", sc, kind, 2, f"E-latency-{side}-{kind}", cap)


# ---------------------------------------------------------------------------------------------------- F. the cross-check pipelines
@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("pipeline", ["wavefront", "queue"])
@pytest.mark.parametrize("row", ["f64-wrappers", "f32"], ids=["f64", "f32"])
def test_cross_check_pipelines(handle, oracles, row, pipeline, which):
    """alt_pipelines.hip:166-199: the wavefront's extend kernel stages wrappers | primitives when they fit 163840 bytes; the
    queue kernel the whole scene when scene + 16 + queue_state_bytes fit.  Reference order (the pipelines have no other)."""
    rt = K.ROWS[row].rt
    if pipeline == "wavefront":
        threshold = K.LDS
        f = K.find(row, threshold, False)[which == "over"]
    else:
        threshold = K.queue_threshold(rt)
        f = K.find(row, threshold)[which == "over"]
    sc = K.scene_of(f, samples=3)
    r = handle({"CRUCIBLE_PIPELINE": pipeline})
    t0 = time.time()
    r.upload_scene(sc.flatten())
    img, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=REFERENCE)
    same_frame(img, st, *oracle_frame(oracles[rt], sc, REFERENCE))
    assert st["bvh_entries"] == K.tree_size(f.n)
    print(f"LDSCAP F-{pipeline}-{which} row={row} threshold={threshold} scene={tuple(f)[:4]} layout={f.bytes} "
          f"launch={f.bytes + (K.queue_state_bytes(rt) if pipeline == 'queue' else 0) if which == 'at' else 0} scene_in_lds={st['scene_in_lds']} seconds={time.time() - t0:.2f}")
    assert st["scene_in_lds"] == (2 if which == "over" else 1)
