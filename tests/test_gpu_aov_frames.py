"""cr_render_aov_frames_*: the guide layers of a batch of frames in one launch.

The yardstick is the single-frame Renderer.render_aov, which tests/test_gpu_aov.py pins bit for bit against the oracle
model: frame k of a batch has the bytes of render_aov at frame frames[k], plane by plane, and the call's stats are the sums
of the single calls' (samples, segments, node_tests, prim_tests, texel_fetches).  One case compares a batch with the
Python-over-oracle model directly, so that the batch has a check that does not pass through the library's single-frame
path.  The shapes are the smallest at which the batch arithmetic can go wrong: 37 x 23 is no multiple of the 4 x 4 tile,
1, 3 and 5 samples are no multiple of the sample group of 4, and the frame lists are single, consecutive, descending with
a repeat, and strided."""
import ctypes as C

import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer
from scenes import few_spheres, mixed_scene, moving_scene
from test_gpu_aov import model, resize, same

pytestmark = pytest.mark.gpu

SEED = 0xA0B1
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
NAMES = [n for n, _, _ in A.AOV_LAYERS]
SUMMED = ("samples", "segments", "node_tests", "prim_tests", "texel_fetches")
LISTS = ([0], [0, 1, 2], [2, 0, 2], [1, 4, 7])


def keyed_camera_scene():
    """test_mixed_scene_default_sky_keyed_camera's scene.  Its keys end after 0.02 s, within frame 0 at its 24 frames per
    second; at 600 per second the frames 0..7 all start inside them, so every frame of a list has its own camera."""
    sc = mixed_scene(sky=False, animate=True)
    sc.scene_cam.frame_rate = 600.0
    return sc


def singles(r, cam, frames, rt, layers=A.CR_AOV_ALL, **kw):
    """frame -> (planes, stats) of one render_aov call per distinct frame"""
    keep, out = cam.frame, {}
    try:
        for f in sorted(set(frames)):
            cam.frame = f
            out[f] = r.render_aov(cam, layers, seed=SEED, real_type=rt, **kw)
    finally:
        cam.frame = keep
    return out


def batch_equals_singles(r, cam, frames, rt, layers=A.CR_AOV_ALL, batch_renderer=None, what="", **kw):
    want = singles(r, cam, frames, rt, layers, **kw)
    keep = cam.frame
    cam.frame = 12345   # params->frame is ignored
    try:
        got, st = (batch_renderer or r).render_aov_frames(cam, frames, layers, seed=SEED, real_type=rt, **kw)
    finally:
        cam.frame = keep
    assert len(got) == len(frames)
    for k, f in enumerate(frames):
        assert sorted(got[k]) == sorted(want[f][0])
        same(got[k], want[f][0], f"{what} frame {f} (entry {k})")
    for key in SUMMED:
        assert st[key] == sum(want[f][1][key] for f in frames), (what, key)
    assert st["segments"] == st["samples"] and st["nan_pixels"] == 0
    first = want[frames[0]][1]
    assert st["bvh_entries"] == first["bvh_entries"] and st["scene_in_lds"] == first["scene_in_lds"]
    return got, st, want


def differ(a, b):
    return any(a[n].tobytes() != b[n].tobytes() for n in a)


# ---- 1. padding and frame lists
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("samples", [1, 3, 5])
@pytest.mark.parametrize("maker", [lambda: moving_scene(frame=0), keyed_camera_scene], ids=["moving", "keyed_camera"])
def test_padding_and_frame_lists(renderer, rt, tag, samples, maker):
    sc = resize(maker(), 37, 23, samples)
    cam = sc.scene_cam
    assert not cam.refit_boxes   # keyed primitives are clipped by the construction-time boxes, as the beauty frame clips them
    renderer.upload_scene(sc.flatten())
    for frames in LISTS:
        got, st, _ = batch_equals_singles(renderer, cam, frames, rt, what=str(frames))
        assert st["samples"] == len(frames) * 37 * 23 * samples
        if len(frames) > 1:   # not one frame rendered N times
            assert any(differ(got[a], got[b]) for a in range(len(frames)) for b in range(a)), frames
    # the keyed camera moves the ray origin between any two frames of these lists
    if maker is keyed_camera_scene:
        got, _ = renderer.render_aov_frames(cam, [1, 4, 7], seed=SEED, real_type=rt)
        assert differ(got[0], got[1]) and differ(got[1], got[2]) and differ(got[0], got[2])


# ---- 2. against the oracle directly
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_a_batch_against_the_oracle_model(renderer, oracles, rt, tag):
    sc = resize(moving_scene(frame=0), 13, 9, 3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    frames = [2, 0, 1]
    got, st = renderer.render_aov_frames(cam, frames, seed=SEED, real_type=rt)
    assert st["samples"] == 3 * 13 * 9 * 3
    for k, f in enumerate(frames):
        cam.frame = f
        want, _ = model(oracles[rt], sc, SEED)
        assert sorted(got[k]) == sorted(NAMES)
        same(got[k], want, f"frame {f}")
    assert differ(got[0], got[1]) and differ(got[1], got[2])


# ---- 3. a static scene: every frame is the same frame
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_static_scene(renderer, rt, tag):
    sc = resize(few_spheres(20), 37, 23, 3)
    renderer.upload_scene(sc.flatten())
    got, _, want = batch_equals_singles(renderer, sc.scene_cam, [0, 3], rt)
    same(got[1], got[0])
    same(want[3][0], want[0][0])


# ---- 4. partial masks: stride and plane offsets of the raw buffer
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_partial_masks_in_the_device_buffer(renderer, rt, tag):
    import torch
    sc = resize(moving_scene(frame=0), 37, 23, 3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    frames = [2, 0, 1]
    full = singles(renderer, cam, frames, rt)
    n = 37 * 23
    dtype = torch.float64 if rt == A.CR_REAL_F64 else torch.float32
    for mask in (A.CR_AOV_DEPTH, A.CR_AOV_ALBEDO | A.CR_AOV_COVERAGE, A.CR_AOV_ALL):
        planes = [(name, c) for name, bit, c in A.AOV_LAYERS if mask & bit]
        stride = n * sum(c for _, c in planes)
        buf = torch.full((stride * len(frames) + 5,), -7.0, dtype=dtype, device="cuda:0")
        assert renderer.render_aov_frames_device(cam, frames, buf.data_ptr(), mask, seed=SEED, real_type=rt) is None
        renderer.synchronize()
        flat = buf.cpu().numpy()
        want = np.concatenate([full[f][0][name].reshape(-1) for f in frames for name, _ in planes])
        assert want.size == stride * len(frames)
        assert flat[:want.size].tobytes() == want.tobytes(), mask
        assert (flat[want.size:] == -7.0).all()   # nothing behind the last frame
        for k, f in enumerate(frames):   # frame k at k * R, its planes in ascending bit order
            o = k * stride
            for name, c in planes:
                assert flat[o:o + n * c].tobytes() == full[f][0][name].tobytes(), (mask, k, name)
                o += n * c
    st = renderer.render_aov_frames_device(cam, frames, buf.data_ptr(), A.CR_AOV_ALL, seed=SEED, real_type=rt, want_stats=True)
    assert st["samples"] == 3 * n * 3 and st["kernel_ms"] > 0


# ---- 5. shards
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_shards(renderer, rt, tag):
    sc = resize(moving_scene(frame=0), 37, 23, 5)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    for output_sum in (0, 1):
        _, st, _ = batch_equals_singles(renderer, cam, [0, 2, 1], rt, sample_begin=1, sample_count=2, output_sum=output_sum)
        assert st["samples"] == 3 * 37 * 23 * 2
    got, st, _ = batch_equals_singles(renderer, cam, [0, 2], rt, sample_begin=2, sample_count=0)   # an empty shard
    assert st["samples"] == 0
    for frame in got:
        assert not frame["albedo"].any() and not frame["normal"].any() and not frame["coverage"].any()
        assert np.isposinf(frame["depth"]).all()


# ---- 6. residency and trees
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_teapot_top_window(renderer, rt, tag):
    from crucible_amd.demo_builder import procedural_sky, teapot_orbit_movie
    sc = teapot_orbit_movie(1, image_width=48, samples=3, sky=procedural_sky(64, 32))
    renderer.upload_scene(sc.flatten())
    _, st, _ = batch_equals_singles(renderer, sc.scene_cam, [0, 5], rt)
    assert st["scene_in_lds"] == 2


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_global_memory_handle(hiplib, rt, tag, monkeypatch):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        sc = resize(keyed_camera_scene(), 24, 16, 3)
        r.upload_scene(sc.flatten())
        _, st, _ = batch_equals_singles(r, sc.scene_cam, [3, 1], rt)
        assert st["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH], ids=["sah_ordered", "lbvh"])
def test_opt_in_trees(renderer, rt, tag, mode):
    sc = resize(keyed_camera_scene(), 24, 16, 3)
    sc.bvh_mode = mode
    renderer.upload_scene(sc.flatten())
    batch_equals_singles(renderer, sc.scene_cam, [0, 2], rt)


# ---- 7. a batch with more units than the work counter hands out: several launches of whole frames
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("limit", [250, 64], ids=["two_then_one", "one_by_one"])
def test_work_counter_split(hiplib, renderer, monkeypatch, rt, tag, limit):
    """37 x 23 @ 5 samples: 60 tiles of 2 sample groups, 120 units a frame with one group per unit.  A limit of 250 units
    leaves room for two frames per launch; one of 64 for one frame at a time, with both groups in one unit."""
    sc = resize(moving_scene(frame=0), 37, 23, 5)
    renderer.upload_scene(sc.flatten())
    monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", str(limit))   # read by cr_create
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        batch_equals_singles(renderer, sc.scene_cam, [0, 1, 2], rt, batch_renderer=r)
    finally:
        r.close()


# ---- 8. refusals
def test_refusals_leave_the_handle_alone(hiplib, renderer):
    sc = resize(moving_scene(frame=0), 24, 16, 3)
    sc.bvh_mode = A.CR_BVH_SAH
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    rt = A.CR_REAL_F32
    before, _ = renderer.render_aov(cam, seed=SEED, real_type=rt)

    def unchanged():
        after, _ = renderer.render_aov(cam, seed=SEED, real_type=rt)
        same(after, before)
        assert sorted(after) == sorted(before)

    def refused(code, frames=(0, 1), layers=A.CR_AOV_ALL, **kw):
        with pytest.raises(CrucibleError) as e:
            renderer.render_aov_frames(cam, frames, layers, seed=SEED, real_type=rt, **kw)
        assert e.value.code == code
        unchanged()
        return str(e.value)

    refused(A.CR_ERR_INVALID_ARG, frames=None)
    # n_frames = 0 with a list that is there, and the device form alike
    cd, p = cam.desc(), cam.params(SEED, rt, 0, None, 0, A.CR_SUM_DEFAULT)
    fr = (C.c_int32 * 2)(0, 1)
    out = np.zeros(24 * 16 * 8 * 2, dtype=np.float32)
    lib, h = renderer.lib, renderer.h
    for n_frames in (0, -1):
        assert lib.cr_render_aov_frames_host(h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, fr, n_frames, out.ctypes.data_as(C.c_void_p), None) == A.CR_ERR_INVALID_ARG
        assert lib.cr_render_aov_frames_device(h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, fr, n_frames, out.ctypes.data_as(C.c_void_p), None) == A.CR_ERR_INVALID_ARG
    assert lib.cr_render_aov_frames_device(h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, None, 2, out.ctypes.data_as(C.c_void_p), None) == A.CR_ERR_INVALID_ARG
    unchanged()
    for layers in (0, 16, -1):
        refused(A.CR_ERR_INVALID_ARG, layers=layers)
    refused(A.CR_ERR_UNSUPPORTED, output_sum=A.CR_OUTPUT_FIXED_SUM)
    refused(A.CR_ERR_INVALID_ARG, sample_begin=2, sample_count=5)   # what cr_render_aov_device rejects
    # boxes are per frame: a refit or a rebuild is the caller's to make frame by frame, with cr_render_frames_*'s message
    for refit in (True, "rebuild"):
        cam.refit_boxes = refit
        try:
            with pytest.raises(CrucibleError) as e:
                renderer.render_aov_frames(cam, [0, 1], seed=SEED, real_type=rt)
        finally:
            cam.refit_boxes = False
        assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_frames cannot refit boxes" in str(e.value)
        unchanged()
    got, _ = renderer.render_aov_frames(cam, [0], seed=SEED, real_type=rt)   # and the handle still renders batches
    same(got[0], before)
    # a refit that changes nothing is no refit
    still = resize(few_spheres(5), 24, 16, 3)
    still.scene_cam.refit_boxes = True
    renderer.upload_scene(still.flatten())
    batch_equals_singles(renderer, still.scene_cam, [0, 3], rt)


# ---- 9. the other pipeline settings
@pytest.mark.parametrize("pipeline", ["wavefront", "queue"])
def test_every_pipeline_setting(hiplib, renderer, monkeypatch, pipeline):
    sc = resize(keyed_camera_scene(), 24, 16, 3)
    renderer.upload_scene(sc.flatten())
    monkeypatch.setenv("CRUCIBLE_PIPELINE", pipeline)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        batch_equals_singles(renderer, sc.scene_cam, [0, 2], A.CR_REAL_F64, batch_renderer=r, what=pipeline)
    finally:
        r.close()
