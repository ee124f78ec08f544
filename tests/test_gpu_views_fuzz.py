"""The keyed seeded scenes of tests/test_gpu_fuzz_entry_points.py (BATCH_SEEDS) through a three-view call: the scene's own
camera, a narrower and tilted copy of it, and a copy without camera keys whose defocus switch is flipped, at the frames
f, f + 2, f + 1.  No tolerance: every view against its single call, beauty and guide layers, counters summed; view 0 and
view 1 of the beauty call against the relaxed oracle.

VIEW_SEEDS is chosen on the CPU (test_view_seeds_are_free_of_nan): the seeds of BATCH_SEEDS for which the oracle alone reports
nan_pixels == 0 for all three views in both precisions, so that no case below runs into CR_ERR_NAN.  A seed may be left out
for NaN frames only, and at most a quarter of the corpus is."""
import copy

import pytest

from crucible_amd import _abi as A
from test_gpu_fuzz_entry_points import BATCH_SEEDS, COUNTERS, NAMES, ORACLE_THREADS, REAL_IDS, REALS, SUMMED, make_scene, same_planes, set_variant

gpu = pytest.mark.gpu
RELAX = A.CR_SUM_RELAXED

# BATCH_SEEDS without the seeds whose second or third view has a NaN frame in the oracle (none of them has)
LEFT_OUT = []
VIEW_SEEDS = [s for s in BATCH_SEEDS if s not in LEFT_OUT]


def views_of(seed):
    """(scene, render seed, the three cameras, their frames)"""
    sc, rseed = make_scene("random", seed)
    assert set_variant(sc, seed) != 1          # a call of several views refuses refit
    cam = sc.scene_cam
    narrow = copy.deepcopy(cam)
    narrow.set_vfov(0.8 * cam.vfov_degrees)
    narrow.set_vup((0.25, 1.0, 0.1))
    still = copy.deepcopy(cam)
    still.look_from(cam.look_from_tl.start_pos)
    still.look_at(cam.look_at_tl.start_pos)
    still.set_defocus_angle(0.0 if cam.defocus_angle_degrees > 0 else 1.5)
    f = cam.frame
    return sc, rseed, [cam, narrow, still], [f, f + 2, f + 1]


def at_frame(cam, frame):
    c = copy.copy(cam)
    c.frame = frame
    return c


def oracle_view(oracle, sc, cam, rseed, tree=None):
    keep = sc.scene_cam
    sc.scene_cam = cam
    try:
        return oracle.render_image(sc, seed=rseed, tree=tree, n_threads=ORACLE_THREADS, sum_order=RELAX)
    finally:
        sc.scene_cam = keep


def test_view_seeds_are_free_of_nan(oracles):
    """What VIEW_SEEDS claims, from the oracle alone; a left-out seed really has a NaN frame, and few are left out."""
    assert set(LEFT_OUT) <= set(BATCH_SEEDS) and 4 * len(LEFT_OUT) <= len(BATCH_SEEDS)
    for seed in BATCH_SEEDS:
        sc, rseed, cams, frames = views_of(seed)
        nan = 0
        for rt, _ in REALS:
            for c, f in zip(cams, frames):
                nan += oracle_view(oracles[rt], sc, at_frame(c, f), rseed)[1]["nan_pixels"]
        assert (nan > 0) == (seed in LEFT_OUT), (seed, nan)


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("seed", VIEW_SEEDS)
def test_beauty_views_equal_single_renders_and_the_oracle(renderer, oracles, seed, rt, tag):
    sc, rseed, cams, frames = views_of(seed)
    renderer.upload_scene(sc.flatten())
    singles = [renderer.render(at_frame(c, f), seed=rseed, real_type=rt, sum_order=RELAX) for c, f in zip(cams, frames)]
    got, st = renderer.render_views(cams, frames, seed=rseed, real_type=rt, sum_order=RELAX)
    cam = sc.scene_cam
    assert got.shape == (3, cam.image_height, cam.image_width, 3)
    for k, (img, _) in enumerate(singles):
        assert got[k].dtype == img.dtype and got[k].tobytes() == img.tobytes(), f"random {seed}: view {k} differs from its single render"
    for key in SUMMED:
        assert st[key] == sum(x[key] for _, x in singles), key
    assert st["nan_pixels"] == 0
    tree = renderer.export_bvh(rt) if seed % 3 == 2 else None
    for k in (0, 1):
        ref, rst = oracle_view(oracles[rt], sc, at_frame(cams[k], frames[k]), rseed, tree)
        assert rst["nan_pixels"] == 0
        assert got[k].tobytes() == ref.tobytes(), f"random {seed}: view {k}: {(got[k] != ref).any(axis=2).sum()} pixels differ from the relaxed oracle"
        for key in COUNTERS:
            assert singles[k][1][key] == rst[key], (k, key, singles[k][1][key], rst[key])


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("seed", VIEW_SEEDS)
def test_guide_views_equal_single_calls(renderer, seed, rt, tag):
    sc, rseed, cams, frames = views_of(seed)
    renderer.upload_scene(sc.flatten())
    singles = [renderer.render_aov(at_frame(c, f), seed=rseed, real_type=rt) for c, f in zip(cams, frames)]
    got, st = renderer.render_aov_views(cams, frames, seed=rseed, real_type=rt)
    assert len(got) == 3
    for k, (planes, _) in enumerate(singles):
        same_planes(got[k], planes, f"random {seed} view {k}")
        assert all(got[k][n].tobytes() == planes[n].tobytes() for n in NAMES)
    for key in SUMMED:
        assert st[key] == sum(x[key] for _, x in singles), key
