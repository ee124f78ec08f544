"""Renders at the ends of the integer ranges the C ABI accepts, each held to the oracle bit for bit in the same sum order
(np.array_equal on the frame or the fixed-point words, equal segments / node_tests / prim_tests / texel_fetches):

A. image extents past 16 bits (65537 x 1 and 1 x 65537; 257 x 255 as the control through the same code),
B. paths of more than 32767 and more than 65535 bounces (scenes.mirror_box_scene),
C. sample indices up to INT32_MAX - 1 in a frame of INT32_MAX samples, and the sample ranges that must be refused,
D. 512 camera keyframes, the documented ceiling, and the refusal of 513.

What each pins in the library: the LDS-queue pipeline packs a slot's pixel into 16 + 16 bits and its depth counters into
16 + 15 bits, so render_queue hands larger renders to the plain megakernel (A, B); the wavefront pipeline keeps
depth_left and stack_n in a word each (B); validate_render adds sample_begin + sample_count in 64 bits (C); the regeneration
step compares a work item's offset in the shard with the shard's length, because begin + offset wraps in the padding of a
shard's last sample group when the shard ends at INT32_MAX (C), and the host's loops over sample batches count in 64 bits (C)."""
import functools
import os

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer
from test_gpu_aov import finalize as aov_finalize, model as aov_model, model_words as aov_model_words, same as aov_same

pytestmark = pytest.mark.gpu

SEED = 0xD1CE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
REF, RELAX = A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_RELAXED
INT32_MAX = 2 ** 31 - 1

# how a render is made: (environment of the handle, sum order)
WAYS = {
    "relaxed": ({}, RELAX),
    "reference": ({}, REF),
    "lane-per-pixel": ({"CRUCIBLE_SAMPLE_GRANULAR": "0"}, REF),
    "wavefront": ({"CRUCIBLE_PIPELINE": "wavefront"}, REF),
    "queue": ({"CRUCIBLE_PIPELINE": "queue"}, REF),
}


@pytest.fixture(scope="module")
def handles(renderer):
    """Renderers by environment (cr_create reads the CRUCIBLE_* knobs once): the session's for the empty one, the others
    created on first use and closed with the module."""
    made = {}

    def get(env):
        if not env:
            return renderer
        key = tuple(sorted(env.items()))
        if key not in made:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[key] = Renderer(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[key]

    yield get
    for r in made.values():
        r.close()


def same_frame(got, st, want, wst, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at (row, column) {tuple(bad[0])}, last at {tuple(bad[-1])}")
    for k in COUNTERS:
        assert st[k] == wst[k], (what, k, st[k], wst[k])


# ---------------------------------------------------------------- A. image extents past 16 bits
SHAPES = [(65537, 1), (1, 65537), (257, 255)]
SHAPE_IDS = ["65537x1", "1x65537", "257x255"]


@functools.lru_cache(maxsize=None)
def extent_oracle(oracle, shape, samples, order, keyed=False, frame=0):
    sc = scenes.extent_scene(*shape, samples, keyed=keyed)
    sc.scene_cam.frame = frame
    return oracle.render_image(sc, seed=SEED, sum_order=order)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_extents_past_16_bits(handles, oracles, shape, samples, rt, tag, way):
    """Every pipeline at a width, then a height, that no 16-bit coordinate holds.  (The queue pipeline cannot: it must hand
    these to the plain megakernel, where the parent commit rendered the last column or row as column or row 0.)"""
    env, order = WAYS[way]
    r = handles(env)
    sc = scenes.extent_scene(*shape, samples)
    r.upload_scene(sc.flatten())
    got, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=order)
    want, wst = extent_oracle(oracles[rt], shape, samples, order)
    assert st["samples"] == shape[0] * shape[1] * samples
    same_frame(got, st, want, wst, f"{way} {shape}")


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_extents_frame_batch(renderer, oracles, shape, rt, tag):
    """Two frames of a moving camera in one launch (the batch's rows run on below each other), frame by frame."""
    sc = scenes.extent_scene(*shape, 3, keyed=True)
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render_frames(sc.scene_cam, [0, 2], seed=SEED, real_type=rt, sum_order=RELAX)
    assert st["samples"] == 2 * shape[0] * shape[1] * 3
    total = dict.fromkeys(COUNTERS, 0)
    for k, frame in enumerate((0, 2)):
        want, wst = extent_oracle(oracles[rt], shape, 3, RELAX, True, frame)
        assert np.array_equal(got[k], want), (shape, frame, int((got[k] != want).any(axis=-1).sum()))
        for c in COUNTERS:
            total[c] += wst[c]
    assert not np.array_equal(got[0], got[1])
    for c in COUNTERS:
        assert st[c] == total[c], (c, st[c], total[c])


@pytest.mark.parametrize("shape,rt", [((65537, 1), A.CR_REAL_F64), ((65537, 1), A.CR_REAL_F32), ((1, 65537), A.CR_REAL_F64),
                                      ((1, 65537), A.CR_REAL_F32), ((257, 255), A.CR_REAL_F64)],
                         ids=["65537x1-f64", "65537x1-f32", "1x65537-f64", "1x65537-f32", "257x255-f64"])
def test_extents_guide_layers(renderer, oracles, shape, rt):
    """All four guide layers against the model of tests/test_gpu_aov.py.  The model loops over the pixels in Python, about
    2.2 s for 65537 of them at one sample (measured on the CPU oracle), so: one sample per pixel, and the control shape in
    f64 only."""
    sc = scenes.extent_scene(*shape, 1)
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render_aov(sc.scene_cam, seed=SEED, real_type=rt)
    want, _ = aov_model(oracles[rt], sc, SEED)
    assert sorted(got) == sorted(n for n, _, _ in A.AOV_LAYERS) and st["samples"] == shape[0] * shape[1]
    aov_same(got, want, str(shape))
    assert 0 < got["coverage"].mean() < 1


# ---------------------------------------------------------------- B. deep paths
DEEP_REF, DEEP_RELAX = 40000, 70000


@functools.lru_cache(maxsize=None)
def deep_paths(oracle):
    """(segments, lit) of each of the 32 paths of mirror_box_scene at max_depth 70000: one-pixel, one-sample renders."""
    sc = scenes.mirror_box_scene(depth=DEEP_RELAX)
    cam = sc.scene_cam
    h = oracle.scene_create(sc.flatten())
    out = []
    try:
        for pix in range(cam.image_width * cam.image_height):
            for s in range(cam.samples):
                rgb, st = oracle.render(h, cam, seed=SEED, sample_begin=s, sample_count=1, output_sum=True, pix_begin=pix, pix_end=pix + 1,
                                        n_threads=1, sum_order=RELAX)
                out.append((st["segments"], bool(rgb.any())))
    finally:
        oracle.scene_destroy(h)
    return out


@functools.lru_cache(maxsize=None)
def deep_oracle(oracle, depth, order):
    return oracle.render_image(scenes.mirror_box_scene(depth=depth), seed=SEED, sum_order=order)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_deep_scene_has_every_class_of_path(oracles, rt, tag):
    """A condition on the inputs, checked on the oracle: of the 32 paths (4 x 4 pixels, 2 samples) some reach the sky after
    fewer than 32768 bounces, some after 32768 .. 65535 (a stack index, then a depth, that 15 / 16 bits do not hold), some
    use up max_depth = 70000; and some reach the sky after 32768 .. 39998 bounces, so that at max_depth = 40000 a stack of
    more than 32767 records is also unwound into a colour.  Observed with seed 0xD1CE (early / 32768..65535 / exhausted /
    32768..39998): f64 15 / 6 / 10 / 2, f32 11 / 11 / 9 / 5."""
    paths = deep_paths(oracles[rt])
    bounces = np.array([s - 1 for s, _ in paths])
    lit = np.array([l for _, l in paths])
    seg = bounces + 1
    early = int((lit & (bounces < 32768)).sum())
    mid = int((lit & (bounces >= 32768) & (bounces < 65536)).sum())
    spent = int((~lit & (seg == DEEP_RELAX)).sum())
    unwound = int((lit & (bounces >= 32768) & (bounces < DEEP_REF - 1)).sum())
    print(f"deep paths {tag}: early {early}, 32768..65535 {mid}, exhausted {spent}, 32768..{DEEP_REF - 2} {unwound}; bounces {sorted(bounces.tolist())}")
    assert early > 0 and mid > 0 and spent > 0 and unwound > 0
    assert early + mid + spent <= len(paths)


@pytest.mark.parametrize("way", ["reference", "wavefront", "queue"])
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_deep_paths_reference_order(handles, oracles, rt, tag, way):
    """max_depth = 40000 with an attenuation stack: stack_n passes 32767.  One workgroup's worth of threads: the stack is
    3 * 40000 * 1024 * 8 bytes at most.  Under a second in the megakernel (which the queue setting falls back to at this
    depth); 7 to 10 s in the wavefront pipeline on an MI355X, whose every bounce is one round of two kernel launches and the
    longest path sets the number of rounds -- 40000 here, whatever the image or the sample count."""
    env, order = WAYS[way]
    r = handles(env)
    sc = scenes.mirror_box_scene(depth=DEEP_REF)
    r.upload_scene(sc.flatten())
    got, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=order)
    want, wst = deep_oracle(oracles[rt], DEEP_REF, REF)
    assert wst["segments"] > 32 * 20000 and (want > 0).any()
    same_frame(got, st, want, wst, way)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_deep_paths_at_the_queue_pipeline_limit(handles, oracles, rt, tag):
    """max_depth = 32767, the deepest render the LDS-queue kernel itself takes: depth_left | stack_n << 16 with both at
    their largest."""
    r = handles(WAYS["queue"][0])
    sc = scenes.mirror_box_scene(depth=32767)
    r.upload_scene(sc.flatten())
    got, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=REF)
    want, wst = deep_oracle(oracles[rt], 32767, REF)
    same_frame(got, st, want, wst, "queue at 32767")


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_deep_paths_relaxed(renderer, oracles, rt, tag):
    """max_depth = 70000 without a stack: depth_left starts beyond 65535."""
    sc = scenes.mirror_box_scene(depth=DEEP_RELAX)
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=RELAX)
    want, wst = deep_oracle(oracles[rt], DEEP_RELAX, RELAX)
    assert wst["segments"] == sum(s for s, _ in deep_paths(oracles[rt]))
    same_frame(got, st, want, wst, "relaxed")


# ---------------------------------------------------------------- C. sample indices at the top of int32
SHARDS = [(INT32_MAX - 1, 1), (INT32_MAX - 5, 5), (INT32_MAX - 4, 3)]
SHARD_IDS = ["last-sample", "last-five", "three-before-the-last"]


def top_scene():
    sc = scenes.few_spheres(3, samples=INT32_MAX)
    cam = sc.scene_cam
    cam.image_width, cam.image_height = 5, 3
    cam.set_max_depth(3)
    return sc


@functools.lru_cache(maxsize=None)
def top_oracle(oracle, begin, count, order, output_sum):
    return oracle.render_image(top_scene(), seed=SEED, sum_order=order, sample_begin=begin, sample_count=count, output_sum=output_sum)


def check_top_shard(r, oracle, rt, begin, count):
    sc = top_scene()
    r.upload_scene(sc.flatten())
    for order, output_sum in ((RELAX, 1), (RELAX, A.CR_OUTPUT_FIXED_SUM), (REF, 1)):   # (fixed-point words exist in the relaxed order only)
        got, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=order, sample_begin=begin, sample_count=count, output_sum=output_sum)
        want, wst = top_oracle(oracle, begin, count, order, output_sum)
        assert st["samples"] == 5 * 3 * count
        assert got.tobytes() == want.tobytes() and got.dtype == want.dtype, (order, output_sum, got.reshape(-1)[:3], want.reshape(-1)[:3])
        for k in COUNTERS:
            assert st[k] == wst[k], (order, output_sum, k, st[k], wst[k])   # surplus samples would show here first


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("begin,count", SHARDS, ids=SHARD_IDS)
def test_shards_that_end_at_int32_max(renderer, oracles, begin, count, rt, tag):
    """Shards cr_group_shard hands out for samples = INT32_MAX.  The five-sample shard's second group of four has two
    padding lanes whose index begin + offset passes INT32_MAX."""
    check_top_shard(renderer, oracles[rt], rt, begin, count)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_shard_at_int32_max_in_several_launches(handles, oracles, rt, tag):
    """A work counter of 128 items cuts the five-sample shard into launches of 4 + 1 samples: the host's batch loop steps past
    INT32_MAX."""
    check_top_shard(handles({"CRUCIBLE_WORK_COUNTER_MAX": "128"}), oracles[rt], rt, INT32_MAX - 5, 5)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_guide_layers_of_a_shard_that_ends_at_int32_max(renderer, oracles, rt, tag):
    sc = top_scene()
    renderer.upload_scene(sc.flatten())
    o = oracles[rt]
    flat = sc.flatten()
    h = o.scene_create(flat)   # test_gpu_aov.model, primed by one sample of the frame's 2^31 - 1 instead of a whole pixel
    try:
        o.render(h, sc.scene_cam, seed=SEED, sample_count=1, pix_begin=0, pix_end=1, n_threads=1)
        words = aov_model_words(o, h, flat, sc.scene_cam, SEED, INT32_MAX - 5, 5)
    finally:
        o.scene_destroy(h)
    for output_sum in (0, 1):
        got, st = renderer.render_aov(sc.scene_cam, seed=SEED, real_type=rt, sample_begin=INT32_MAX - 5, sample_count=5, output_sum=output_sum)
        want = aov_finalize(words, sc.scene_cam, o.np_real, output_sum)
        aov_same(got, want, f"output_sum {output_sum}")
        assert st["samples"] == 5 * 3 * 5 and st["segments"] == st["samples"]


def test_sample_ranges_past_int32_max_are_refused(renderer, o32):
    """begin + count wraps in 32 bits: (1, INT32_MAX) would pass as a range that ends at INT32_MIN and start 2^31 samples
    per pixel.  Every entry point refuses, and the handle renders on."""
    sc = top_scene()
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    want, wst = top_oracle(o32, INT32_MAX - 1, 1, RELAX, 1)
    for begin, count in ((1, INT32_MAX), (INT32_MAX, INT32_MAX)):
        for call in (lambda **kw: renderer.render(cam, seed=SEED, sum_order=RELAX, **kw),
                     lambda **kw: renderer.render(cam, seed=SEED, sum_order=REF, **kw),
                     lambda **kw: renderer.render_aov(cam, seed=SEED, **kw),
                     lambda **kw: renderer.render_frames(cam, [0, 1], seed=SEED, sum_order=RELAX, **kw)):
            with pytest.raises(CrucibleError) as e:
                call(sample_begin=begin, sample_count=count)
            assert e.value.code == A.CR_ERR_INVALID_ARG
            got, st = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F32, sum_order=RELAX, sample_begin=INT32_MAX - 1, sample_count=1, output_sum=1)
            same_frame(got, st, want, wst, "after a refusal")


# ---------------------------------------------------------------- D. camera keyframe ceiling
@functools.lru_cache(maxsize=None)
def keyed_oracle(oracle, amp, order):
    return oracle.render_image(scenes.keyed_camera_scene(amp=amp), seed=SEED, sum_order=order)


@pytest.mark.parametrize("rt,tag,order", scenes.REAL_ORDERS, ids=scenes.REAL_ORDER_IDS)
def test_512_camera_keyframes(renderer, oracles, rt, tag, order):
    sc = scenes.keyed_camera_scene()
    d = sc.scene_cam.desc()
    assert (d.from_key_count, d.at_key_count) == (300, 212)
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=order)
    same_frame(got, st, *keyed_oracle(oracles[rt], 0.3, order), "512 keys")


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_512_keyframes_through_the_key_ring(renderer, oracles, rt, tag):
    """Five asynchronous renders back to back, each with its own 512 keys, through the ring of four key slots: what the same
    renders give one at a time -- the oracle's frames."""
    import torch
    amps = (0.3, 0.25, 0.2, 0.15, 0.1)
    scs = [scenes.keyed_camera_scene(amp=a) for a in amps]
    renderer.upload_scene(scs[0].flatten())   # the scenes differ in their cameras only
    bufs = [torch.full((8, 8, 3), -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0") for _ in amps]
    for sc, buf in zip(scs, bufs):
        assert renderer.render_device(sc.scene_cam, buf.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX) is None
    renderer.synchronize()
    frames = [b.cpu().numpy() for b in bufs]
    for a, sc, frame in zip(amps, scs, frames):
        alone, st = renderer.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=RELAX)
        want, wst = keyed_oracle(oracles[rt], a, RELAX)
        same_frame(alone, st, want, wst, f"amp {a} alone")
        assert np.array_equal(frame, want), a
    assert not np.array_equal(frames[0], frames[4])


def test_513_camera_keyframes_are_refused(renderer, o64):
    sc = scenes.keyed_camera_scene()
    renderer.upload_scene(sc.flatten())
    for n_from, n_at in ((301, 212), (300, 213)):
        over = scenes.keyed_camera_scene(n_from, n_at)
        d = over.scene_cam.desc()
        assert d.from_key_count + d.at_key_count == 513
        with pytest.raises(CrucibleError) as e:
            renderer.render(over.scene_cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
        assert e.value.code == A.CR_ERR_UNSUPPORTED
        with pytest.raises(CrucibleError) as e:
            renderer.render_aov(over.scene_cam, seed=SEED, real_type=A.CR_REAL_F64)
        assert e.value.code == A.CR_ERR_UNSUPPORTED
        got, st = renderer.render(sc.scene_cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
        same_frame(got, st, *keyed_oracle(o64, 0.3, RELAX), "512 keys after a refusal")
