"""cr_render_frames_device / cr_render_frames_host: a batch of movie frames in one launch.  The contract is bit-exact:
frame k of a batch is, byte for byte, the frame a single render writes with frame = frames[k] and the relaxed oracle's
frame of frames[k], and the batch's work counters are the sum of those single renders' counters (and of the oracle's) --
in f32 and in f64, for any frame list, every output_sum mode, a sample shard, a batch the 32-bit work counter splits into
several launches, and every scene residency.  Batches need CR_SUM_RELAXED (tests/conftest.py makes the reference order the suite default, so every render
here names its sum order)."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.demo_builder import procedural_sky, teapot_orbit_movie
from crucible_amd.renderer import CrucibleError, Renderer

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
RELAX = A.CR_SUM_RELAXED


def singles(r, sc, frames, rt, **kw):
    """Each frame of the list as its own cr_render_host call: (images, stats)."""
    out, sts = [], []
    cam = sc.scene_cam
    keep = cam.frame
    try:
        for f in frames:
            cam.frame = f
            img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
            out.append(img)
            sts.append(st)
    finally:
        cam.frame = keep
    return out, sts


_ORACLES = {}


def oracle_frames(sc, frames, rt, **kw):
    """The relaxed oracle's frame for each entry of the list: (frames, summed counters)."""
    from oracle.oracle import Oracle
    o = _ORACLES.setdefault(rt, Oracle(rt))
    cam = sc.scene_cam
    keep = cam.frame
    out, tot = [], {c: 0 for c in COUNTERS}
    try:
        for f in frames:
            cam.frame = f
            img, st = o.render_image(sc, seed=SEED, sum_order=RELAX, **kw)
            out.append(img)
            for c in COUNTERS:
                tot[c] += st[c]
    finally:
        cam.frame = keep
    return out, tot


def check_batch(r, sc, frames, rt, **kw):
    """The batch equals the single renders bit for bit, and its counters are theirs summed; each frame is also the
    relaxed oracle's frame of frames[k], bit for bit.  Returns the batch stats."""
    r.upload_scene(sc.flatten())
    got, st = r.render_frames(sc.scene_cam, frames, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
    refs, rsts = singles(r, sc, frames, rt, **kw)
    cam = sc.scene_cam
    assert got.shape == (len(frames), cam.image_height, cam.image_width, 3)
    for k, ref in enumerate(refs):
        assert got[k].dtype == ref.dtype
        assert got[k].tobytes() == ref.tobytes(), f"frame {frames[k]} (entry {k}) differs"
    for c in COUNTERS + ("samples",):
        assert st[c] == sum(s[c] for s in rsts), (c, st[c], [s[c] for s in rsts])
    assert st["kernel_ms"] > 0
    want, wst = oracle_frames(sc, frames, rt, **kw)
    for k, ref in enumerate(want):
        assert got[k].dtype == ref.dtype
        assert got[k].tobytes() == ref.tobytes(), f"frame {frames[k]} (entry {k}) differs from the relaxed oracle"
    for c in COUNTERS:
        assert st[c] == wst[c], (c, st[c], wst[c])
    return st


def moved_frames_differ(r, sc, frames, rt):
    """The test is only meaningful if the frames of the list really differ (keys cross the frames)."""
    r.upload_scene(sc.flatten())
    got, _ = r.render_frames(sc.scene_cam, frames, seed=SEED, real_type=rt, sum_order=RELAX)
    return any(got[0].tobytes() != got[k].tobytes() for k in range(1, len(frames)) if frames[k] != frames[0])


@pytest.mark.parametrize("rt,name", REALS)
def test_teapot_orbit_camera_keys(renderer, rt, name):
    """The orbit movie: keyed camera (CAMK kernels), an image sky, the tree's top levels in LDS (RES_TOP)."""
    sc = teapot_orbit_movie(1, image_width=64, samples=4, sky=procedural_sky(64, 32))
    frames = [0, 7, 30, 61, 119, 200]
    st = check_batch(renderer, sc, frames, rt)
    assert st["scene_in_lds"] == 2
    assert moved_frames_differ(renderer, sc, frames, rt)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("build", [scenes.moving_scene, scenes.scaled_scene], ids=["moving", "scaled"])
def test_keyed_primitives(renderer, rt, name, build):
    """Keyed primitives (ANIM kernels) at 1 fps with a 360 degree shutter: the keys change inside and across the frames."""
    sc = build(width=48, samples=4)
    frames = [0, 1, 2, 3]
    check_batch(renderer, sc, frames, rt)
    assert moved_frames_differ(renderer, sc, frames, rt)


@pytest.mark.parametrize("rt,name", REALS)
def test_scene_without_keys(renderer, rt, name):
    """No keys at all: the batch runs on the CAMK kernel, a single render on the static one -- the same bytes."""
    sc = scenes.few_spheres(20, width=40, samples=3)
    check_batch(renderer, sc, [0, 5, 2], rt)


@pytest.mark.parametrize("rt,name", REALS)
def test_scene_in_global_memory(monkeypatch, rt, name):
    """A handle that keeps the whole scene in global memory (RES_GLOBAL)."""
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        st = check_batch(r, scenes.moving_scene(width=40, samples=3), [0, 2, 1], rt)
        assert st["scene_in_lds"] == 0
    finally:
        r.close()


def odd_size(sc, w=37, h=23):
    """An image whose sides are multiples of no tile side (the tile is 4x4, 8x4 or 8x8 pixels)."""
    sc.scene_cam.image_width, sc.scene_cam.image_height = w, h
    return sc


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("spp", [1, 2, 3, 4, 5])
def test_odd_image_size_every_tile_shape(renderer, rt, name, spp):
    """37x23: no tile straddles two frames although H is not a multiple of the tile height; below 4 samples the tile
    shape changes (8x8 pixels at 1 sample, 8x4 at 2 and 3)."""
    check_batch(renderer, odd_size(scenes.moving_scene(samples=spp)), [0, 1, 2], rt)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("frames", [[0, 1, 2, 3], [1, 4, 7], [3, 2, 1, 0], [2, 2, 5, 2], [3]],
                         ids=["consecutive", "strided", "descending", "repeated", "single"])
def test_frame_lists(renderer, rt, name, frames):
    check_batch(renderer, odd_size(scenes.moving_scene(samples=3)), frames, rt)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("output_sum", [0, 1, A.CR_OUTPUT_FIXED_SUM], ids=["mean", "sum", "fixed"])
@pytest.mark.parametrize("shard", [None, (1, 3)], ids=["whole", "shard"])
def test_output_modes_and_shards(renderer, rt, name, output_sum, shard):
    """The mean, sums in reals and fixed-point words at the whole frame's scale; a sample shard [1, 4) of 5 samples."""
    kw = {"output_sum": output_sum}
    if shard:
        kw.update(sample_begin=shard[0], sample_count=shard[1])
    check_batch(renderer, odd_size(scenes.moving_scene(samples=5)), [0, 2, 1], rt, **kw)


def test_device_form(renderer):
    """cr_render_frames_device writes the same frames, one after the other, into a device buffer."""
    import torch
    sc = odd_size(scenes.moving_scene(samples=3))
    renderer.upload_scene(sc.flatten())
    frames = [1, 0, 3]
    want, _ = renderer.render_frames(sc.scene_cam, frames, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    d = torch.full((len(frames), 23, 37, 3), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = renderer.render_frames_device(sc.scene_cam, frames, d.data_ptr(), seed=SEED, real_type=A.CR_REAL_F64,
                                       sum_order=RELAX, want_stats=True)
    assert st["samples"] == 37 * 23 * 3 * len(frames)
    assert d.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("limit,spp", [(8000, 4), (3840, 8)], ids=["whole-frames", "sample-batches"])
def test_work_counter_split(monkeypatch, rt, name, limit, spp):
    """A small CRUCIBLE_WORK_COUNTER_MAX: 37x23 at 4 samples is 60 tiles x 64 = 3840 work items a frame, so 8000 holds two
    frames per launch (five frames: three launches); at 8 samples a frame alone needs two sample batches of 3840 items
    and the batch runs frame by frame."""
    sc = odd_size(scenes.moving_scene(samples=spp))
    frames = [0, 1, 2, 3, 4]
    monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", str(limit))
    small = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_WORK_COUNTER_MAX")
    try:
        check_batch(small, sc, frames, rt)   # single renders on the small counter too
        got, st = small.render_frames(sc.scene_cam, frames, seed=SEED, real_type=rt, sum_order=RELAX)
    finally:
        small.close()
    r = Renderer(0)   # the single renders of an unrestricted handle
    try:
        r.upload_scene(sc.flatten())
        refs, rsts = singles(r, sc, frames, rt)
    finally:
        r.close()
    for k, ref in enumerate(refs):
        assert got[k].tobytes() == ref.tobytes(), k
    for c in COUNTERS:
        assert st[c] == sum(s[c] for s in rsts), c


def test_refusals_leave_the_handle_usable(renderer):
    lib = renderer.lib
    sc = scenes.moving_scene(width=32, samples=2)
    renderer.upload_scene(sc.flatten())
    cam = sc.scene_cam
    ok = lambda: renderer.render_frames(cam, [0, 1], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)  # noqa: E731
    good, _ = ok()

    # reference order: sequential over samples, a per-sample buffer per frame
    with pytest.raises(CrucibleError) as e:
        renderer.render_frames(cam, [0, 1], seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_REFERENCE_ORDER)
    assert e.value.code == A.CR_ERR_UNSUPPORTED and "CR_SUM_RELAXED" in str(e.value)
    assert ok()[0].tobytes() == good.tobytes()
    # the handle default resolves to the reference order here (CRUCIBLE_SUM_ORDER=reference, tests/conftest.py)
    with pytest.raises(CrucibleError) as e:
        renderer.render_frames(cam, [0, 1], seed=SEED, real_type=A.CR_REAL_F32, sum_order=A.CR_SUM_DEFAULT)
    assert e.value.code == A.CR_ERR_UNSUPPORTED

    # refit boxes with keyed primitives: the boxes are per frame
    cam.refit_boxes = True
    with pytest.raises(CrucibleError) as e:
        renderer.render_frames(cam, [0, 1], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    assert e.value.code == A.CR_ERR_UNSUPPORTED and "refit" in str(e.value)
    cam.refit_boxes = False
    assert ok()[0].tobytes() == good.tobytes()

    # n_frames < 1, null frames
    cd, p = cam.desc(), cam.params(SEED, A.CR_REAL_F64, sum_order=RELAX)
    out = np.empty((2, cam.image_height, cam.image_width, 3), dtype=np.float64)
    fr = (C.c_int32 * 2)(0, 1)
    outp = out.ctypes.data_as(C.c_void_p)
    for frames, n in ((fr, 0), (fr, -3), (None, 2)):
        for fn in (lib.cr_render_frames_host, lib.cr_render_frames_device):
            assert fn(renderer.h, C.byref(cd), C.byref(p), frames, n, outp, None) == A.CR_ERR_INVALID_ARG
    # what validate() rejects for a single render it rejects for a batch
    bad = cam.params(SEED, A.CR_REAL_F64, sample_begin=1, sample_count=2, sum_order=RELAX)   # 2 samples: [1, 3) is outside
    assert lib.cr_render_frames_host(renderer.h, C.byref(cd), C.byref(bad), fr, 2, outp, None) == A.CR_ERR_INVALID_ARG
    assert lib.cr_render_frames_host(renderer.h, C.byref(cd), C.byref(p), fr, 2, None, None) == A.CR_ERR_INVALID_ARG
    assert ok()[0].tobytes() == good.tobytes()


def test_empty_shard(renderer):
    """sample_count = 0 (more ranks than samples): zero frames, no kernel, as for a single render."""
    sc = odd_size(scenes.moving_scene(samples=3))
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render_frames(sc.scene_cam, [0, 1], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX,
                                     sample_begin=3, sample_count=0, output_sum=A.CR_OUTPUT_FIXED_SUM)
    assert got.shape == (2, 23, 37, 3) and not got.any() and st["samples"] == 0


@pytest.mark.parametrize("order", ["relaxed", "reference"])
def test_scene_render_movie_frames_per_launch(tmp_path, monkeypatch, order):
    """Scene.render_movie with frames_per_launch = 4 writes the files frames_per_launch = 1 writes: batched under relaxed
    sums, one frame per call after the library refuses the batch under the reference order."""
    monkeypatch.setenv("CRUCIBLE_SUM_ORDER", order)
    stems = []
    for n in (1, 4):
        sc = teapot_orbit_movie(1, image_width=32, samples=2, frame_rate=4, duration=1.5, sky=procedural_sky(64, 32))
        sc.real_type = A.CR_REAL_F64
        sc.frames_per_launch = n
        stem = str(tmp_path / f"movie{n}")
        sc.render_movie(stem)
        stems.append(stem)
    names = sorted(os.listdir(os.path.join(stems[0], "artifacts")))
    assert len(names) == 6 and names == sorted(os.listdir(os.path.join(stems[1], "artifacts")))
    for nm in names:
        assert filecmp.cmp(os.path.join(stems[0], "artifacts", nm), os.path.join(stems[1], "artifacts", nm), shallow=False), nm
