"""Exact group renders: in CR_SUM_RELAXED the members of a group export their fixed-point sums at the whole frame's
scale (CrRenderParams.output_sum = CR_OUTPUT_FIXED_SUM), the group adds the integers and the root finalizes them like
cr_render_device -- so a group of any member count returns the one-device relaxed frame BIT FOR BIT, with the same
counters.  Several members share the one GPU of the box (CRUCIBLE_GROUP_SAME_DEVICE=1: the u64 combine kernel stands in
for RCCL); one-member groups with the collective forced on run the ncclUint64 / ncclUint8 reduces on real RCCL.

tests/conftest.py makes the suite's default order the reference order, so every render here asks for CR_SUM_RELAXED."""
import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.group import RenderGroup
from crucible_amd.renderer import CrucibleError, np_real

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
RELAX = A.CR_SUM_RELAXED
FIXED = A.CR_OUTPUT_FIXED_SUM
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
F = np.uint64(1 << 63)
M = np.uint64((1 << 63) - 1)


def combine(a, b):
    """include/crucible_hip.h: c = ((a & M) + (b & M)) | ((a | b) & F)."""
    return ((a & M) + (b & M)) | ((a | b) & F)


def torch_real(rt):
    import torch
    return torch.float64 if rt == A.CR_REAL_F64 else torch.float32


def device_frame(renderer, cam, rt):
    """cr_render_device's relaxed frame (a NaN frame too, which cr_render_host refuses)."""
    import torch
    t = torch.full((cam.image_height, cam.image_width, 3), -1.0, dtype=torch_real(rt), device="cuda:0")
    torch.cuda.synchronize()
    renderer.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX)
    renderer.synchronize()
    return t.cpu().numpy()


def group_device_frame(g, cam, rt):
    import torch
    t = torch.full((cam.image_height, cam.image_width, 3), -1.0, dtype=torch_real(rt), device="cuda:0")
    torch.cuda.synchronize()
    st = g.render_device(cam, t.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX)
    return t.cpu().numpy(), st


def finalize(renderer, words, cam, rt, samples):
    """cr_fixed_sums_to_rgb on host words (H, W, 3) uint64."""
    import torch
    d_words = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to("cuda:0")
    out = torch.full(words.shape, -1.0, dtype=torch_real(rt), device="cuda:0")
    torch.cuda.synchronize()
    renderer.fixed_sums_to_rgb(d_words.data_ptr(), out.data_ptr(), width=cam.image_width, height=cam.image_height,
                               samples=samples, real_type=rt)
    renderer.synchronize()
    return out.cpu().numpy()


# words where the finalize can go wrong: the 32-bit halves of the conversion, the first words that do not fit a double
# (2^53 + 1 ties to even downwards, 2^53 + 3 upwards), the largest magnitude and flagged words
CRAFTED = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 53) - 1, (1 << 53) + 1, (1 << 53) + 3, (1 << 63) - 1,
           1 << 63, (1 << 63) | 5, (1 << 63) | ((1 << 63) - 1), (1 << 63) | (1 << 53) + 1]


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("samples", [1, 3, 2047, 2048, 4095, 4096, 1 << 20, (1 << 31) - 1])
def test_finalize_of_crafted_words_is_plain_arithmetic(renderer, rt, tag, samples):
    """cr_fixed_sums_to_rgb against the header's finalize in plain Python (tests/test_oracle_relaxed.py: float(int),
    ldexp, the divide, np.float32), bit for bit, at every scale the sample count selects."""
    from types import SimpleNamespace

    from test_oracle_relaxed import bits, finalize as plain_finalize
    words = np.array(CRAFTED, dtype=np.uint64).reshape(1, len(CRAFTED) // 3, 3)
    cam = SimpleNamespace(image_width=words.shape[1], image_height=1)
    got = finalize(renderer, words, cam, rt, samples)
    want = plain_finalize(words, samples, rt)
    assert got.dtype == want.dtype
    assert np.array_equal(bits(got), bits(want)), (got.reshape(-1), want.reshape(-1))


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("members,spp", [(2, 6), (3, 10), (4, 10), (8, 5)])
def test_same_device_group_equals_the_single_relaxed_frame(renderer, oracles, monkeypatch, rt, tag, members, spp):
    """(8, 5): three members have empty shards and contribute zero words.  The group's frame and counters are also the
    relaxed oracle's, bit for bit."""
    monkeypatch.setenv("CRUCIBLE_GROUP_SAME_DEVICE", "1")
    sc = book1_end_scene(1, scene_seed=1, image_width=80, samples=spp)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    single, sst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    g = RenderGroup.local([0] * members)
    try:
        g.upload_scene(sc.flatten())
        img, st = g.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
        assert st["members"] == members and st["used_rccl"] == 0 and st["nan_pixels"] == 0
        assert img.dtype == single.dtype and np.array_equal(img, single)
        for k in COUNTERS:
            assert st[k] == sst[k], k
        assert st["samples"] == 80 * 45 * spp
        dev, _ = group_device_frame(g, cam, rt)
        assert np.array_equal(dev, single)
        want, wst = oracles[rt].render_image(sc, seed=SEED, sum_order=RELAX)
        assert np.array_equal(img, want)
        for k in COUNTERS:
            assert st[k] == wst[k], k
    finally:
        g.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
def test_many_samples_per_shard_share_the_frame_scale(renderer, monkeypatch, rt, tag):
    """5000 spp over 3 members: each shard alone would take the scale 2^52 (<= 2047 samples), the frame takes 2^50."""
    monkeypatch.setenv("CRUCIBLE_GROUP_SAME_DEVICE", "1")
    sc = book1_end_scene(1, scene_seed=1, image_width=16, samples=5000)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    single, sst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    g = RenderGroup.local([0] * 3)
    try:
        g.upload_scene(sc.flatten())
        img, st = g.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
        assert np.array_equal(img, single)
        for k in COUNTERS:
            assert st[k] == sst[k], k
    finally:
        g.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["local", "rank"])
def test_one_member_group_through_rccl_is_exact(renderer, monkeypatch, rt, tag, mode):
    """The collective forced on with one rank: the split kernel, ncclReduce(sum, uint64) of the magnitudes,
    ncclReduce(max, uint8) of the flag plane, the merge and the finalize on real RCCL.  A float reduce would round the
    shard's sum once more before the divide (f32: visibly)."""
    monkeypatch.setenv("CRUCIBLE_GROUP_FORCE_RCCL", "1")
    sc = book1_end_scene(1, scene_seed=1, image_width=96, samples=5)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    single = device_frame(renderer, cam, rt)
    _, sst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    g = RenderGroup.local([0]) if mode == "local" else RenderGroup.rank(0, 0, 1, RenderGroup.unique_id())
    try:
        g.upload_scene(sc.flatten())
        img, st = group_device_frame(g, cam, rt)
        assert st["used_rccl"] == 1 and st["members"] == 1 and st["reduce_ms"] > 0
        assert np.array_equal(img, single)
        for k in COUNTERS:
            assert st[k] == sst[k], k
        host, hst = g.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
        assert np.array_equal(host, single) and hst["nan_pixels"] == 0
    finally:
        g.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("spp,splits", [(12, [(0, 5), (5, 0), (5, 4), (9, 3)]), (3000, [(0, 1000), (1000, 0), (1000, 2000)])],
                         ids=["12spp", "3000spp"])
def test_fixed_sum_words_of_shards_add_to_the_frame(renderer, oracles, rt, tag, spp, splits):
    """Shard words combined with the header's rule equal the whole frame's words, and cr_fixed_sums_to_rgb of them is the
    relaxed frame bit for bit.  3000 spp: the frame's scale 2^51 is not the one a 1000- or 2000-sample shard would take.
    Every shard's words are the relaxed oracle's."""
    sc = book1_end_scene(1, scene_seed=1, image_width=80 if spp < 100 else 16, samples=spp)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    whole, wst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED)
    assert whole.dtype == np.uint64 and whole.shape == (cam.image_height, cam.image_width, 3)
    assert not (whole & F).any() and (whole & M).any()
    acc = np.zeros_like(whole)
    for b, n in splits:
        part, pst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED, sample_begin=b, sample_count=n)
        if n == 0:
            assert not part.any()
        want, _ = oracles[rt].render_image(sc, seed=SEED, sum_order=RELAX, output_sum=FIXED, sample_begin=b, sample_count=n)
        assert np.array_equal(part, want), (b, n)
        acc = combine(acc, part)
    assert np.array_equal(acc, whole)
    frame, fst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    for k in COUNTERS:
        assert wst[k] == fst[k], k
    got = finalize(renderer, acc, cam, rt, spp)
    assert got.dtype == np_real(rt) and np.array_equal(got, frame)


@pytest.mark.parametrize("members", [2, 8])
def test_nan_flags_survive_the_group(renderer, monkeypatch, members):
    """Every sample of this camera is NaN (look_from == look_at).  8 members at 2 spp: six shards are empty and carry
    no flags, the merge keeps the others'.  The group's frame is NaN wherever the single frame is, and the host entry
    points report CR_ERR_NAN alike."""
    monkeypatch.setenv("CRUCIBLE_GROUP_SAME_DEVICE", "1")
    sc = scenes.few_spheres(2, width=24, samples=2)
    sc.scene_cam.look_from((1.0, 2.0, 3.0))
    sc.scene_cam.look_at((1.0, 2.0, 3.0))
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    g = RenderGroup.local([0] * members)
    try:
        g.upload_scene(sc.flatten())
        for rt, _ in REALS:
            single = device_frame(renderer, cam, rt)
            assert np.isnan(single).any()
            img, _ = group_device_frame(g, cam, rt)
            assert np.array_equal(np.isnan(img), np.isnan(single))
            assert np.array_equal(img, single, equal_nan=True)
            with pytest.raises(CrucibleError) as e1:
                renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
            with pytest.raises(CrucibleError) as e2:
                g.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
            assert e1.value.code == e2.value.code == A.CR_ERR_NAN
    finally:
        g.close()


def test_nan_flags_survive_the_rccl_flag_plane(renderer, monkeypatch):
    """The same NaN frame through the one-member collective: the flags leave the words as a byte plane
    (ncclReduce(max, uint8)) and are merged back on the root."""
    monkeypatch.setenv("CRUCIBLE_GROUP_FORCE_RCCL", "1")
    sc = scenes.few_spheres(2, width=24, samples=2)
    sc.scene_cam.look_from((1.0, 2.0, 3.0))
    sc.scene_cam.look_at((1.0, 2.0, 3.0))
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    g = RenderGroup.local([0])
    try:
        g.upload_scene(sc.flatten())
        for rt, _ in REALS:
            single = device_frame(renderer, cam, rt)
            img, st = group_device_frame(g, cam, rt)
            assert st["used_rccl"] == 1
            assert np.array_equal(img, single, equal_nan=True) and np.isnan(img).any()
            with pytest.raises(CrucibleError) as e:
                g.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
            assert e.value.code == A.CR_ERR_NAN
    finally:
        g.close()


def test_fixed_sum_refusals_leave_the_handle_usable(renderer):
    import torch
    sc = book1_end_scene(1, scene_seed=1, image_width=32, samples=3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    before, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    for order in (A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_DEFAULT):   # CR_SUM_DEFAULT resolves to the reference order here
        with pytest.raises(CrucibleError) as e:
            renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=order, output_sum=FIXED)
        assert e.value.code == A.CR_ERR_UNSUPPORTED and "CR_OUTPUT_FIXED_SUM" in str(e.value)
    for bad in (3, -1):
        with pytest.raises(CrucibleError) as e:
            renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX, output_sum=bad)
        assert e.value.code == A.CR_ERR_INVALID_ARG and "output_sum" in str(e.value)
    words = torch.zeros(cam.image_height * cam.image_width * 3, dtype=torch.int64, device="cuda:0")
    out = torch.zeros(words.shape, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for kw in (dict(samples=0), dict(width=0), dict(real_type=7)):
        args = dict(width=cam.image_width, height=cam.image_height, samples=3, real_type=A.CR_REAL_F64)
        args.update(kw)
        with pytest.raises(CrucibleError) as e:
            renderer.fixed_sums_to_rgb(words.data_ptr(), out.data_ptr(), **args)
        assert e.value.code == A.CR_ERR_INVALID_ARG
    after, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    assert np.array_equal(after, before)
