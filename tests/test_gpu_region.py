"""cr_render_region_device / cr_render_region_host: a region of a frame.  The contract is bit-exact: output pixel (i, j)
of a region (x0, y0, w, h) is, byte for byte, pixel (x0 + i, y0 + j) of the whole-frame render with the same camera and
params, and of the relaxed oracle's rows of those pixels; the region's work counters are the oracle's for its pixels, and
the counters of a partition add up to the frame's -- in f32 and f64, every tile shape, every output_sum, shards, every
residency, the opt-in trees, refits, sample batches inside a region and frames beyond 2^26 pixels.  Region renders need
CR_SUM_RELAXED (tests/conftest.py makes the reference order the suite default, so every render here names its order)."""
import ctypes as C

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
FIXED = A.CR_OUTPUT_FIXED_SUM
W, H = 37, 23
# a partition of the 37 x 23 frame, none of it aligned to a work tile (4x4, 8x4 or 8x8 pixels)
P = [(0, 0, 5, 3), (5, 0, 32, 3), (0, 3, 5, 20), (5, 3, 13, 9), (18, 3, 19, 9), (5, 12, 32, 11)]
EXTRA = [(36, 22, 1, 1), (0, 0, 37, 23)]
F = np.uint64(1 << 63)
M = np.uint64((1 << 63) - 1)


def odd_size(sc, w=W, h=H):
    sc.scene_cam.image_width, sc.scene_cam.image_height = w, h
    return sc


def scaled(regions, w, h):
    """The regions of the 37 x 23 frame with their edges moved into a w x h frame (a partition stays one)."""
    bx, by = (lambda x: x * w // W), (lambda y: y * h // H)
    out = []
    for x0, y0, rw, rh in regions:
        if (rw, rh) == (1, 1):
            out.append((w - 1, h - 1, 1, 1))
        else:
            out.append((bx(x0), by(y0), bx(x0 + rw) - bx(x0), by(y0 + rh) - by(y0)))
    return out


def crop(img, region):
    x0, y0, w, h = region
    return np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])


def combine(a, b):
    """include/crucible_hip.h: c = ((a & M) + (b & M)) | ((a | b) & F)."""
    return ((a & M) + (b & M)) | ((a | b) & F)


def oracle_rows(oracle, scene_h, cam, region, **kw):
    """The relaxed oracle over the region's pixels, row by row (pix_begin / pix_end): (h, w, 3) array, summed counters."""
    x0, y0, w, h = region
    rows, tot = [], {c: 0 for c in COUNTERS}
    for j in range(h):
        b = (y0 + j) * cam.image_width + x0
        out, st = oracle.render(scene_h, cam, seed=SEED, pix_begin=b, pix_end=b + w, n_threads=1, sum_order=RELAX, **kw)
        rows.append(out)
        for c in COUNTERS:
            tot[c] += st[c]
    return np.stack(rows), tot


def check_regions(r, oracle, sc, rt, regions, partition, check_oracle=True, **kw):
    """Every region equals the crop of render()'s frame (and the oracle's rows, with its counters); the counters over the
    partition add up to the frame's.  Returns the full render's stats."""
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    full, fst = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
    oh = oracle.scene_create(sc.flatten()) if check_oracle else None
    try:
        tot = {c: 0 for c in COUNTERS + ("samples",)}
        for reg in regions:
            got, st = r.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
            assert got.shape == (reg[3], reg[2], 3) and got.dtype == full.dtype
            assert got.tobytes() == crop(full, reg).tobytes(), f"region {reg} differs from the crop"
            n_samples = cam.samples if kw.get("sample_count") is None else kw["sample_count"]
            assert st["samples"] == reg[2] * reg[3] * n_samples
            if check_oracle:
                want, wst = oracle_rows(oracle, oh, cam, reg, **kw)
                assert got.tobytes() == want.tobytes(), f"region {reg} differs from the relaxed oracle"
                for c in COUNTERS:
                    assert st[c] == wst[c], (reg, c, st[c], wst[c])
            if reg in partition:
                for c in tot:
                    tot[c] += st[c]
        if partition:
            for c in tot:
                assert tot[c] == fst[c], (c, tot[c], fst[c])
    finally:
        if oh:
            oracle.scene_destroy(oh)
    return fst


SCENES = {
    "static": lambda: odd_size(scenes.mixed_scene(samples=5)),                # CAMK kernel, defocus, image sky
    "animated": lambda: odd_size(scenes.mixed_scene(samples=5, animate=True)),   # ANIM and a keyed camera
    "moving": lambda: odd_size(scenes.moving_scene(samples=5, frame=1)),
    "teapot": lambda: teapot_orbit_movie(1, image_width=64, samples=4, sky=procedural_sky(64, 32)),
}


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("which", list(SCENES))
def test_crops_and_oracle(renderer, oracles, rt, name, which):
    sc = SCENES[which]()
    cam = sc.scene_cam
    part = scaled(P, cam.image_width, cam.image_height)
    extra = scaled(EXTRA, cam.image_width, cam.image_height)
    assert sum(w * h for _, _, w, h in part) == cam.image_width * cam.image_height
    fst = check_regions(renderer, oracles[rt], sc, rt, part + extra, part)
    if which == "teapot":
        assert fst["scene_in_lds"] == 2
    # the whole frame as a region: render()'s bytes and counters
    full, fst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    got, st = renderer.render_region(cam, (0, 0, cam.image_width, cam.image_height), seed=SEED, real_type=rt, sum_order=RELAX)
    assert got.tobytes() == full.tobytes()
    for c in COUNTERS + ("samples", "bvh_entries", "scene_in_lds"):
        assert st[c] == fst[c], c
    assert st["nan_pixels"] == 0


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("spp", [1, 2, 3, 4, 5])
def test_every_tile_shape(renderer, oracles, rt, name, spp):
    """Below 4 samples the work tile changes shape (8x8 pixels at 1 sample, 8x4 at 2 and 3)."""
    sc = odd_size(scenes.moving_scene(samples=spp, frame=1))
    check_regions(renderer, oracles[rt], sc, rt, [(5, 3, 13, 9), (3, 1, 9, 10)], [], check_oracle=(spp in (1, 5)))


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("output_sum", [0, 1, FIXED], ids=["mean", "sum", "fixed"])
@pytest.mark.parametrize("shard", [None, (1, 3)], ids=["whole", "shard"])
def test_output_modes_and_shards(renderer, oracles, rt, name, output_sum, shard):
    kw = {"output_sum": output_sum}
    if shard:
        kw.update(sample_begin=shard[0], sample_count=shard[1])
    sc = odd_size(scenes.mixed_scene(samples=5, animate=True))
    check_regions(renderer, oracles[rt], sc, rt, [(5, 3, 13, 9), (36, 22, 1, 1)], [], **kw)


@pytest.mark.parametrize("rt,name", REALS)
def test_fixed_sum_shards_combine(renderer, rt, name):
    """The words of two shards of a region, added as the header prescribes and finalised with the region's dimensions,
    are the mean region."""
    import torch
    sc = odd_size(scenes.mixed_scene(samples=5))
    cam = sc.scene_cam
    reg = (5, 3, 13, 9)
    renderer.upload_scene(sc.flatten())
    mean, _ = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX)
    a, _ = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED, sample_begin=0, sample_count=2)
    b, _ = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED, sample_begin=2, sample_count=3)
    words = combine(a, b)
    d_words = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to("cuda:0")
    out = torch.full(words.shape, -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    renderer.fixed_sums_to_rgb(d_words.data_ptr(), out.data_ptr(), width=reg[2], height=reg[3], samples=5, real_type=rt)
    renderer.synchronize()
    assert out.cpu().numpy().tobytes() == mean.tobytes()


@pytest.mark.parametrize("rt,name", REALS)
def test_scene_in_global_memory(monkeypatch, oracles, rt, name):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        sc = odd_size(scenes.moving_scene(samples=5, frame=1))
        fst = check_regions(r, oracles[rt], sc, rt, P, P, check_oracle=False)
        assert fst["scene_in_lds"] == 0
        _, st = r.render_region(sc.scene_cam, P[3], seed=SEED, real_type=rt, sum_order=RELAX)
        assert st["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH], ids=["ordered", "lbvh"])
def test_trees(renderer, oracles, rt, name, mode):
    sc = odd_size(scenes.mixed_scene(samples=5, animate=True))
    sc.bvh_mode = mode
    check_regions(renderer, oracles[rt], sc, rt, P, P, check_oracle=False)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("refit", [True, "rebuild"], ids=["boxes", "rebuild"])
def test_refits(renderer, oracles, rt, name, refit):
    """One frame per call, so boxes may be refitted and the tree rebuilt: the region is the crop of the full render made
    with the same setting."""
    sc = odd_size(scenes.moving_scene(samples=5, frame=1))
    sc.bvh_mode = A.CR_BVH_SAH
    sc.scene_cam.refit_boxes = refit
    check_regions(renderer, oracles[rt], sc, rt, [P[3], P[5], EXTRA[0]], [], check_oracle=False)


@pytest.mark.parametrize("rt,name", REALS)
def test_work_counter_forces_sample_batches(monkeypatch, rt, name):
    """(5,3,13,9) at 8 samples is 12 tiles x 64 = 768 work items per group of 4 samples: a counter of 1000 holds one group,
    so the region renders as two sample batches -- the same bytes."""
    sc = odd_size(scenes.moving_scene(samples=8, frame=1))
    reg = (5, 3, 13, 9)
    monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", "1000")
    small = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_WORK_COUNTER_MAX")
    try:
        small.upload_scene(sc.flatten())
        got, st = small.render_region(sc.scene_cam, reg, seed=SEED, real_type=rt, sum_order=RELAX)
    finally:
        small.close()
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        full, _ = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=RELAX)
        one, ost = r.render_region(sc.scene_cam, reg, seed=SEED, real_type=rt, sum_order=RELAX)
    finally:
        r.close()
    assert got.tobytes() == crop(full, reg).tobytes() and one.tobytes() == got.tobytes()
    for c in COUNTERS + ("samples",):
        assert st[c] == ost[c], c


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("w,h,reg", [(16384, 4100, (8190, 2047, 11, 6)), (40000, 50000, (39990, 49995, 10, 5))],
                         ids=["past-2^26", "2e9"])
def test_frames_beyond_2_26_pixels(renderer, oracles, rt, name, w, h, reg):
    sc = odd_size(scenes.mixed_scene(samples=5), w, h)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX)
    oracle = oracles[rt]
    oh = oracle.scene_create(sc.flatten())
    try:
        want, wst = oracle_rows(oracle, oh, cam, reg)
    finally:
        oracle.scene_destroy(oh)
    assert got.tobytes() == want.tobytes()
    for c in COUNTERS:
        assert st[c] == wst[c], c
    assert st["samples"] == reg[2] * reg[3] * 5 and st["nan_pixels"] == 0
    # the whole-frame call keeps its limit and its message
    cd, p = cam.desc(), cam.params(SEED, rt, sum_order=RELAX)
    dummy = np.zeros(8, dtype=np.float64)
    rc = renderer.lib.cr_render_device(renderer.h, C.byref(cd), C.byref(p), dummy.ctypes.data_as(C.c_void_p), None)
    assert rc == A.CR_ERR_INVALID_ARG and renderer.lib.cr_last_error(renderer.h) == b"image too large"


def test_device_form(renderer):
    import torch
    sc = odd_size(scenes.moving_scene(samples=3, frame=1))
    cam = sc.scene_cam
    reg = (5, 3, 13, 9)
    renderer.upload_scene(sc.flatten())
    want, _ = renderer.render_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    d = torch.full((reg[3], reg[2], 3), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert renderer.render_region_device(cam, reg, d.data_ptr(), seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX) is None
    renderer.synchronize()
    assert d.cpu().numpy().tobytes() == want.tobytes()
    assert renderer.last_kernel_ms() > 0
    st = renderer.render_region_device(cam, reg, d.data_ptr(), seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX, want_stats=True)
    assert st["samples"] == reg[2] * reg[3] * 3
    # an empty shard: zeros of the region's size
    for output_sum, dtype in ((0, torch.float64), (FIXED, torch.int64)):
        e = torch.full((reg[3], reg[2], 3), 7, dtype=dtype, device="cuda:0")
        guard = torch.full((64,), 7, dtype=dtype, device="cuda:0")
        torch.cuda.synchronize()
        st = renderer.render_region_device(cam, reg, e.data_ptr(), seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX,
                                           sample_begin=3, sample_count=0, output_sum=output_sum, want_stats=True)
        assert st["samples"] == 0 and not e.cpu().numpy().any() and (guard.cpu().numpy() == 7).all()
    got, st = renderer.render_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F32, sum_order=RELAX, sample_begin=3, sample_count=0)
    assert got.shape == (9, 13, 3) and not got.any() and st["samples"] == 0


def test_refusals_leave_the_handle_usable(renderer, monkeypatch):
    lib = renderer.lib
    sc = odd_size(scenes.moving_scene(samples=2, frame=1))
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    reg = (5, 3, 13, 9)
    ok = lambda: renderer.render_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)[0]  # noqa: E731
    good = ok()
    cd, p = cam.desc(), cam.params(SEED, A.CR_REAL_F64, sum_order=RELAX)
    out = np.empty((H, W, 3), dtype=np.float64)
    outp = out.ctypes.data_as(C.c_void_p)
    int_max = 2 ** 31 - 1

    def rc_of(region, fn=lib.cr_render_region_host, cdesc=cd, params=p, dst=outp):
        r = None if region is None else C.byref(A.CrRegion(*region))
        return fn(renderer.h, C.byref(cdesc) if cdesc is not None else None, C.byref(params) if params is not None else None, r, dst, None)

    bad_regions = [None, (0, 0, 0, 3), (0, 0, 3, 0), (0, 0, -2, 3), (0, 0, 3, -1), (-1, 0, 3, 3), (0, -1, 3, 3), (int_max, 0, 2, 1),
                   (0, int_max, 1, 2), (30, 0, 8, 3), (0, 20, 3, 4), (W, 0, 1, 1), (0, H, 1, 1)]
    for fn in (lib.cr_render_region_host, lib.cr_render_region_device):
        for region in bad_regions:
            assert rc_of(region, fn) == A.CR_ERR_INVALID_ARG, region
            assert ok().tobytes() == good.tobytes(), region   # after every refusal the render made before it
        assert rc_of(reg, fn, cdesc=None) == A.CR_ERR_INVALID_ARG
        assert ok().tobytes() == good.tobytes()
        assert rc_of(reg, fn, params=None) == A.CR_ERR_INVALID_ARG
        assert ok().tobytes() == good.tobytes()
        assert rc_of(reg, fn, dst=None) == A.CR_ERR_INVALID_ARG
        assert ok().tobytes() == good.tobytes()
        # what a whole-frame call rejects: a sample range outside [0, samples)
        bad = cam.params(SEED, A.CR_REAL_F64, sample_begin=1, sample_count=2, sum_order=RELAX)
        assert rc_of(reg, fn, params=bad) == A.CR_ERR_INVALID_ARG
        assert ok().tobytes() == good.tobytes()
        # a region above 2^26 pixels: the whole 16384 x 4100 frame
        big = odd_size(scenes.moving_scene(samples=2, frame=1), 16384, 4100).scene_cam.desc()
        assert rc_of((0, 0, 16384, 4100), fn, cdesc=big) == A.CR_ERR_INVALID_ARG
        assert b"2^26" in lib.cr_last_error(renderer.h)
        assert ok().tobytes() == good.tobytes()
        # a frame above 2^31 - 1 pixels: the key's pixel index has 32 bits
        huge = odd_size(scenes.moving_scene(samples=2, frame=1), 50000, 50000).scene_cam.desc()
        assert rc_of(reg, fn, cdesc=huge) == A.CR_ERR_INVALID_ARG
        assert b"2^31" in lib.cr_last_error(renderer.h)
        assert ok().tobytes() == good.tobytes()
    # the reference order (named, and as what CR_SUM_DEFAULT resolves to in this suite)
    for order in (A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_DEFAULT):
        with pytest.raises(CrucibleError) as e:
            renderer.render_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64, sum_order=order)
        assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_region" in str(e.value)
        assert ok().tobytes() == good.tobytes()
    # the cross-check pipelines
    for pipe in ("queue", "wavefront"):
        monkeypatch.setenv("CRUCIBLE_PIPELINE", pipe)
        other = Renderer(0)
        monkeypatch.delenv("CRUCIBLE_PIPELINE")
        try:
            other.upload_scene(sc.flatten())
            with pytest.raises(CrucibleError) as e:
                other.render_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
            assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_region" in str(e.value)
            # guide regions work there, before and after the refusal
            planes, _ = other.render_aov_region(cam, reg, ("depth",), seed=SEED, real_type=A.CR_REAL_F64)
            assert planes["depth"].shape == (reg[3], reg[2])
        finally:
            other.close()
        assert ok().tobytes() == good.tobytes()


@pytest.mark.parametrize("rt,name", REALS)
def test_render_tiled(renderer, rt, name):
    sc = odd_size(scenes.mixed_scene(samples=5, animate=True))
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    full, fst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    got, st = renderer.render_tiled(cam, tile=(16, 8), seed=SEED, real_type=rt, sum_order=RELAX)
    assert got.shape == full.shape and got.tobytes() == full.tobytes()
    for c in COUNTERS + ("samples", "nan_pixels"):
        assert st[c] == fst[c], c


def test_latency_entry_point_handle(monkeypatch):
    """A handle whose f32 whole-frame renders run on the 6-waves-per-SIMD entry point (CRUCIBLE_LATENCY_ENTRIES): those
    kernels do not carry a region's offsets, so a region runs on the regular kernel -- the same bytes and counters."""
    monkeypatch.setenv("CRUCIBLE_LATENCY_ENTRIES", "1")
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    r = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_LATENCY_ENTRIES")
    monkeypatch.delenv("CRUCIBLE_LDS_LIMIT")
    try:
        for sc in (odd_size(scenes.moving_scene(samples=5, frame=1)), odd_size(scenes.mixed_scene(samples=5))):
            fst = check_regions(r, None, sc, A.CR_REAL_F32, P + EXTRA, P, check_oracle=False)
            assert fst["scene_in_lds"] == 2
    finally:
        r.close()
