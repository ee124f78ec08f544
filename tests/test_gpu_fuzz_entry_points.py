"""The fuzz corpora of tests/test_gpu_fuzz.py through the entry points that came after them: the guide layers
(cr_render_aov_*), the frame batches (cr_render_frames_*, cr_render_aov_frames_*), the device-built SAH tree when it is
rendered, and CR_REFIT_REBUILD (the region and adaptive calls, cr_render_region_*, cr_render_aov_region_*, cr_render_adaptive_*
and cr_render_adaptive_frames_*: tests/test_gpu_fuzz_regions_adaptive.py).  No tolerance anywhere: every plane against tests/test_gpu_aov.py's model over the oracle's
probes (bytes, and the positions of the NaNs on their own), every beauty frame against the oracle's, every batch against
its single calls, work counters against the oracle's depth-1 render of the same scene and tree.

What the corpus has to contain is checked on the CPU, from the model's words alone (test_corpus_contains_the_edges): a
corpus without a flagged channel, a negative word or a pixel whose samples differ in depth would leave aov_word's refusal,
the flag word, the sign in the finalize and the depth minimum to luck.  DIRECTED names seeds of hostile_scene beyond the
committed list, found by a scan with the model, for the properties that only one committed scene shows; the same scan
found none for a flagged channel on a covered pixel or an encoded normal above 1.

The rota of tests/test_gpu_fuzz.py by seed % 3 stays: 0 the reference tree, 1 refit_boxes, 2 an opt-in tree exported and
handed to the model -- here cycling through CR_BVH_SAH, CR_BVH_SAH_ORDERED, CR_BVH_LBVH and the two SAH modes built on
the device."""
import numpy as np
import pytest

import lbvh_model as L
from crucible_amd import _abi as A
from crucible_amd.scene import NERP, WORLD, Lambertian, Metal, Scene, Sphere
from test_gpu_aov import NAMES, fx_log2, model, same
from test_gpu_fuzz import BIG_SEEDS, COUNTERS, HOSTILE_SEEDS, RANDOM_SEEDS, big_scene, hostile_scene, random_scene

gpu = pytest.mark.gpu

F64, F32 = A.CR_REAL_F64, A.CR_REAL_F32
REALS = [(F64, "f64"), (F32, "f32")]
REAL_IDS = [t for _, t in REALS]
DEVICE = A.CR_BVH_BUILD_DEVICE
TREES = [A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH, A.CR_BVH_SAH | DEVICE, A.CR_BVH_SAH_ORDERED | DEVICE]
SUMMED = ("samples",) + COUNTERS
ORACLE_THREADS = 4        # the images are at most 73 pixels wide

# What the corpus has to contain, property -> (hostile seed, precision) cases that show it, found with the model on the CPU:
# (a) a flagged channel on a pixel without coverage, (b) a negative normal word, (e) a pixel whose samples hit at different
# depths, (f) a finite depth beside a +inf one, (t) a hit between t = 0 and t = 0.001 (the planes change when the interval
# opens at 0).  The committed hostile seeds have one scene for (b), 300031 in f32, and one for (t), 300031 in f64; the
# seeds of DIRECTED were added for these two.  A scan of 24 000 further seeds (300045..320044, and 1200008..1204007 with
# the degenerate cameras) in both precisions found no scene for (c) a flagged channel on a covered pixel or (d) an
# encoded-normal word above samples * 2^S: see DESIGN.md 2.
EDGES = {"a": [(1200000, "f64"), (1200005, "f32")],
         "b": [(300031, "f32"), (300166, "f32"), (300227, "f32")],
         "e": [(300012, "f32"), (300036, "f64")],
         "f": [(300020, "f64"), (300005, "f32")],
         "t": [(300031, "f64"), (300108, "f64"), (300108, "f32"), (300114, "f64"), (300114, "f32")]}
DIRECTED = [300166, 300227, 300108, 300114]   # hostile seeds beyond tests/test_gpu_fuzz.py's list (switches as for every hostile seed, hostile_case)
# the random seeds whose scenes carry keys (primitive or camera keys) and run with variant 0 or 2, and for which the
# oracle alone reports nan_pixels == 0 at the frames f, f + 1, f + 2 in both precisions and both sum orders
BATCH_SEEDS = [3, 5, 9, 11, 14, 15, 104, 107, 108, 203, 206, 207]
# random seeds below 100 (no list or wrapper elements: a frame tree is built over single primitives) with a visible keyed
# primitive, nan_pixels == 0 in the oracle's refit render in both precisions; 24 has two visible primitives (one leaf,
# written on the host whatever the builder)
REBUILD_SEEDS = [3, 5, 6, 15, 18, 24, 33]


def hostile_case(seed):
    """test_hostile_scene_bit_exact's scene for this seed.  ValueError: the mirror's own argument checks reject it."""
    return hostile_scene(seed, lists=seed >= 400000 or (seed < 300045 and seed % 2 == 1), wrappers=seed >= 1200000, degenerate_camera=seed >= 1200000)


def make_scene(kind, seed):
    """(scene, render seed) as the beauty tests of tests/test_gpu_fuzz.py make them"""
    if kind == "hostile":
        return hostile_case(seed), seed
    if kind == "random":
        return random_scene(1000 + seed, lists=seed >= 100, wrappers=seed >= 200), 4000 + seed
    return big_scene(seed, lists=seed % 2 == 1), seed


def set_variant(sc, seed):
    variant = seed % 3
    sc.scene_cam.refit_boxes = variant == 1
    if variant == 2:
        sc.bvh_mode = TREES[(seed // 3) % len(TREES)]
    return variant


def guide_cases():
    return ([("hostile", s) for s in HOSTILE_SEEDS] + [("hostile", s) for s in DIRECTED]
            + [("random", s) for s in RANDOM_SEEDS[::2]] + [("big", s) for s in BIG_SEEDS])


def edges(words, samples):
    """Which of the properties (a), (b), (c), (d), (f) of test_corpus_contains_the_edges the words of one image show."""
    sums, flags, depth = words
    top = samples << fx_log2(samples)
    out = set()
    for s, f in zip(sums, flags):
        if f:
            out.add("c" if s[6] > 0 else "a")
        if min(s[3:6]) < 0:
            out.add("b")
        if max(s[3:6]) > top:
            out.add("d")
    if np.isfinite(depth).any() and np.isposinf(depth).any():
        out.add("f")
    return out


def depths_differ(oracle, sc, seed, tree=None, linear_list=False):
    """(e): the samples of the frame one by one -- a pixel at which two of them hit, at different depths."""
    cam = sc.scene_cam
    per_sample = [model(oracle, sc, seed, tree=tree, linear_list=linear_list, sample_begin=s, sample_count=1)[1][2] for s in range(cam.samples)]
    for a in range(len(per_sample)):
        for b in range(a):
            both = np.isfinite(per_sample[a]) & np.isfinite(per_sample[b])
            if (per_sample[a][both] != per_sample[b][both]).any():
                return True
    return False


def interval_matters(oracle, sc, seed, planes, tree=None, linear_list=False):
    """The model's planes differ when the hit interval opens at 0 instead of 0.001: some primary ray has a hit in between."""
    open_at_0, _ = model(oracle, sc, seed, tree=tree, linear_list=linear_list, tmin=0.0)
    return any(open_at_0[n].tobytes() != planes[n].tobytes() for n in NAMES)


def shows(p, oracle, sc, seed, planes, words, tree=None, linear_list=False):
    """Whether the model's words of one image (on the tree they were formed with) show the property p of EDGES."""
    if p == "e":
        return depths_differ(oracle, sc, seed, tree, linear_list)
    if p == "t":
        return interval_matters(oracle, sc, seed, planes, tree, linear_list)
    return p in edges(words, sc.scene_cam.samples)


def same_planes(got, want, what):
    """same(), after the positions of the NaNs on their own"""
    assert sorted(got) == sorted(want) == sorted(NAMES), what
    for n in NAMES:
        assert np.array_equal(np.isnan(got[n]), np.isnan(want[n])), f"{what} {n}: NaN at {np.argwhere(np.isnan(got[n]) != np.isnan(want[n]))[:4].tolist()}"
    same(got, want, what)


# ------------------------------------------------------------------ 2. what the corpus contains (CPU)
def test_corpus_contains_the_edges(oracles):
    """From the model's words alone, every case of EDGES shows its property: the corpus that
    test_guide_layers_against_the_model runs reaches aov_word's refusal and the flag words (a), the sign of a word (b), the
    depth minimum over different depths (e), both kinds of depth in one image (f) and the start of the interval (t).  The
    scenes are formed as that test forms them -- the reference tree, refit by the rota; an opt-in tree needs the device and
    is replaced by the reference tree here, and that test asserts the property again on the tree it walked.  At most 2
    hostile seeds are scenes the Python mirror rejects, and no case of EDGES is among them."""
    rejected = set()
    for kind, seed in guide_cases():
        if kind == "hostile":
            try:
                make_scene(kind, seed)
            except ValueError:
                rejected.add(seed)
    assert len(rejected) <= 2, rejected
    by_tag = {tag: rt for rt, tag in REALS}
    assert sorted(EDGES) == ["a", "b", "e", "f", "t"] and all(EDGES.values())
    assert set(DIRECTED) <= {seed for cases in EDGES.values() for seed, _ in cases}
    for p, cases in EDGES.items():
        for seed, tag in cases:
            assert ("hostile", seed) in guide_cases() and seed not in rejected
            sc, rseed = make_scene("hostile", seed)
            sc.scene_cam.refit_boxes = seed % 3 == 1
            planes, words = model(oracles[by_tag[tag]], sc, rseed)
            assert shows(p, oracles[by_tag[tag]], sc, rseed, planes, words), (p, seed, tag)
            assert not {"c", "d"} & edges(words, sc.scene_cam.samples)   # none known: a scene that shows one gets a name in EDGES


def test_batch_and_rebuild_seeds_are_keyed_and_free_of_nan(oracles):
    """What BATCH_SEEDS and REBUILD_SEEDS claim, from the oracle alone: no case below runs into CR_ERR_NAN."""
    for seed in sorted(set(BATCH_SEEDS + REBUILD_SEEDS)):
        sc, rseed = make_scene("random", seed)
        cam = sc.scene_cam
        recs = L.prim_records(sc.flatten())
        vis = L.visible_prims(recs)
        if seed in BATCH_SEEDS:
            assert seed % 3 != 1 and ((recs["key_count"] > 0).any() or cam.look_from_tl.keyframes() or cam.look_at_tl.keyframes()), seed
        if seed in REBUILD_SEEDS:
            assert seed < 100 and (recs["key_count"][vis] > 0).any(), seed
        f = cam.frame
        for rt, _ in REALS:
            for frame, refit, order in ([(g, False, A.CR_SUM_RELAXED) for g in (f, f + 1, f + 2)] if seed in BATCH_SEEDS else []) + (
                    [(f, True, A.CR_SUM_REFERENCE_ORDER)] if seed in REBUILD_SEEDS else []):
                cam.frame, cam.refit_boxes = frame, refit
                _, st = oracles[rt].render_image(sc, seed=rseed, n_threads=ORACLE_THREADS, sum_order=order)
                assert st["nan_pixels"] == 0, (seed, frame, refit)


# ------------------------------------------------------------------ 1. guide layers of the corpora against the model
def oracle_depth_1(oracle, sc, seed, tree, linear_list):
    """The oracle's work counters for the primary rays: its depth-1 render of the same scene and tree"""
    cam = sc.scene_cam
    depth = cam.max_depth
    cam.set_max_depth(1)
    try:
        _, rst = oracle.render_image(sc, seed=seed, tree=tree, linear_list=linear_list, n_threads=ORACLE_THREADS, sum_order=A.CR_SUM_REFERENCE_ORDER)
    finally:
        cam.set_max_depth(depth)
    return rst


def check_guide_stats(st, rst, cam, frames=1):
    assert st["samples"] == frames * cam.image_width * cam.image_height * cam.samples and st["segments"] == st["samples"]
    assert st["nan_pixels"] == 0          # the stat is 0 for this pass even when planes hold NaN (include/crucible_hip.h)
    if rst is not None:
        for k in COUNTERS:
            assert st[k] == rst[k], (k, st[k], rst[k])


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("kind,seed", guide_cases(), ids=[f"{k}-{s}" for k, s in guide_cases()])
def test_guide_layers_against_the_model(renderer, oracles, kind, seed, rt, tag):
    """All four layers of one corpus scene, by the rota of its seed: planes and NaN positions against the model, work
    counters against the oracle's depth-1 render on the same tree; a device-built tree is reported as such."""
    try:
        sc, rseed = make_scene(kind, seed)
    except ValueError:
        assert kind == "hostile"
        pytest.skip("the mirror's own argument checks reject this scene")
    variant = set_variant(sc, seed)
    cam = sc.scene_cam
    flat = sc.flatten()
    renderer.upload_scene(flat)
    got, st = renderer.render_aov(cam, seed=rseed, real_type=rt)
    tree, empty = None, False
    if variant == 2:
        tree = renderer.export_bvh(rt)
        empty = len(tree[1]) == 0
        if sc.bvh_mode & DEVICE and len(L.visible_prims(L.prim_records(flat))) >= 3:
            assert renderer.build_info(rt)["built_on_device"] == 1
        if empty:
            tree = None
    want, words = model(oracles[rt], sc, rseed, tree=tree, linear_list=empty)
    same_planes(got, want, f"{kind} {seed}")
    check_guide_stats(st, oracle_depth_1(oracles[rt], sc, rseed, tree, empty), cam)
    for p, cases in EDGES.items():   # a named case shows its property on the tree it walked
        if kind == "hostile" and (seed, tag) in cases:
            assert shows(p, oracles[rt], sc, rseed, want, words, tree, empty), (p, seed)


# ------------------------------------------------------------------ 3. frame batches on the random corpus
def batch_scene(seed):
    sc, rseed = make_scene("random", seed)
    assert set_variant(sc, seed) != 1          # a batch refuses refit
    f = sc.scene_cam.frame
    return sc, rseed, [f, f + 2, f, f + 1]


def at_frames(cam, frames, call):
    keep, out = cam.frame, {}
    try:
        for f in sorted(set(frames)):
            cam.frame = f
            out[f] = call()
    finally:
        cam.frame = keep
    return out


def guide_batch_equals_singles(renderer, cam, frames, rseed, rt, what):
    singles = at_frames(cam, frames, lambda: renderer.render_aov(cam, seed=rseed, real_type=rt))
    got, st = renderer.render_aov_frames(cam, frames, seed=rseed, real_type=rt)
    assert len(got) == len(frames)
    for k, f in enumerate(frames):
        same_planes(got[k], singles[f][0], f"{what} frame {f} (entry {k})")
    for key in SUMMED:
        assert st[key] == sum(singles[f][1][key] for f in frames), (what, key)
    check_guide_stats(st, None, cam, len(frames))
    return got, singles


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("seed", BATCH_SEEDS)
def test_guide_batch_equals_single_calls(renderer, seed, rt, tag):
    sc, rseed, frames = batch_scene(seed)
    renderer.upload_scene(sc.flatten())
    guide_batch_equals_singles(renderer, sc.scene_cam, frames, rseed, rt, f"random {seed}")


def blinking_camera_scene():
    """1 fps, a 180 degree shutter: frame f draws ray times in [f, f + 0.5).  look_at jumps onto look_from at t = 1 and
    back at t = 2 (NERP keys), so the camera has no basis during frame 1 and only then: every ray of that frame is NaN,
    misses, and its sky colour flags the three albedo channels of every pixel."""
    sc = Scene.new_image(1.0, 9, 1.0, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(3)
    cam.set_max_depth(4)
    cam.look_from((0.5, 1.5, 6.0))
    cam.look_at((0.0, 0.5, 0.0))
    cam.set_vfov(40.0)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, Lambertian.new_from_color((0.4, 0.6, 0.3), 1.0)), "ground")
    sc.add_element(Sphere.new((0.0, 0.7, 0.0), 0.7, Metal.new((0.8, 0.7, 0.6), 0.1)), "ball")
    sc.cam_translate_point((0.5, 1.5, 6.0), 1.0, NERP, WORLD, "at")
    sc.cam_translate_point((0.0, 0.5, 0.0), 2.0, NERP, WORLD, "at")
    return sc


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
def test_guide_batch_flags_stay_in_their_frame(renderer, oracles, rt, tag):
    """A frame whose every pixel is flagged between two frames without a flag: the flag words are per frame."""
    sc = blinking_camera_scene()
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    for frames in ([0, 1, 2], [1, 0, 1, 2]):
        got, _ = guide_batch_equals_singles(renderer, cam, frames, 77, rt, str(frames))
        for k, f in enumerate(frames):
            want, words = at_frames(cam, [f], lambda: model(oracles[rt], sc, 77))[f]
            same_planes(got[k], want, f"{frames} frame {f} against the model")
            assert np.isnan(got[k]["albedo"]).all() == (f == 1) and np.isnan(got[k]["albedo"]).any() == (f == 1)
            assert not np.isnan(got[k]["normal"]).any() and not np.isnan(got[k]["coverage"]).any()
            assert (got[k]["coverage"] > 0).any() == (f != 1)


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("seed", BATCH_SEEDS)
def test_beauty_batch_equals_single_renders_and_the_oracle(renderer, oracles, seed, rt, tag):
    sc, rseed, frames = batch_scene(seed)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    RELAX = A.CR_SUM_RELAXED
    singles = at_frames(cam, frames, lambda: renderer.render(cam, seed=rseed, real_type=rt, sum_order=RELAX))
    got, st = renderer.render_frames(cam, frames, seed=rseed, real_type=rt, sum_order=RELAX)
    assert got.shape == (len(frames), cam.image_height, cam.image_width, 3)
    for k, f in enumerate(frames):
        assert got[k].dtype == singles[f][0].dtype and got[k].tobytes() == singles[f][0].tobytes(), f"random {seed}: frame {f} (entry {k}) differs"
    for key in SUMMED:
        assert st[key] == sum(singles[f][1][key] for f in frames), key
    assert st["nan_pixels"] == 0
    tree = renderer.export_bvh(rt) if seed % 3 == 2 else None
    ref, rst = oracles[rt].render_image(sc, seed=rseed, tree=tree, n_threads=ORACLE_THREADS, sum_order=RELAX)
    assert rst["nan_pixels"] == 0
    assert got[0].tobytes() == ref.tobytes(), f"random {seed}: {(got[0] != ref).any(axis=2).sum()} pixels differ from the relaxed oracle"
    for key in COUNTERS:
        assert singles[frames[0]][1][key] == rst[key], (key, singles[frames[0]][1][key], rst[key])


# ------------------------------------------------------------------ CR_REFIT_REBUILD on the random corpus
@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("builder", [0, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("seed", REBUILD_SEEDS)
def test_refit_rebuild_on_random_scenes(renderer, oracles, seed, builder, rt, tag):
    """Beauty image and guide layers of a frame whose SAH tree is rebuilt over the keyed primitives' motion boxes, against
    the oracle and the model walking cr_export_render_bvh's tree."""
    sc, rseed = make_scene("random", seed)
    cam = sc.scene_cam
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED | builder
    cam.refit_boxes = "rebuild"
    flat = sc.flatten()
    renderer.upload_scene(flat)
    img, st = renderer.render(cam, seed=rseed, real_type=rt, sum_order=A.CR_SUM_REFERENCE_ORDER)
    tree = renderer.export_render_bvh(rt)
    info = renderer.frame_build_info(rt)
    assert info["n_wrappers"] == len(tree[1]) > 0 and info["bvh_mode"] == A.CR_BVH_SAH_ORDERED
    if len(L.visible_prims(L.prim_records(flat))) >= 3:
        assert info["built_on_device"] == (1 if builder else 0)
    got, gst = renderer.render_aov(cam, seed=rseed, real_type=rt)
    again = renderer.export_render_bvh(rt)
    assert all(np.array_equal(x, y) for x, y in zip(tree, again))           # the guide pass walked the frame's tree too
    cam.refit_boxes = True                                                   # the oracle refits the tree it is handed
    ref, rst = oracles[rt].render_image(sc, seed=rseed, tree=tree, n_threads=ORACLE_THREADS, sum_order=A.CR_SUM_REFERENCE_ORDER)
    assert rst["nan_pixels"] == 0
    assert np.array_equal(img, ref), f"random {seed}: {(img != ref).any(axis=2).sum()} pixels differ"
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    want, _ = model(oracles[rt], sc, rseed, tree=tree)
    same_planes(got, want, f"random {seed} rebuilt")
    check_guide_stats(gst, oracle_depth_1(oracles[rt], sc, rseed, tree, False), cam)
