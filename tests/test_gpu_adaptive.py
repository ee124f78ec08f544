"""cr_render_adaptive_device / cr_render_adaptive_host: a frame whose blocks stop taking samples once their two half-frame
sums agree.  The rule is exact integer arithmetic, so everything here is bit for bit and without a tolerance: the counts
and the frame equal those of tests/adaptive_model.py, an independent model fed with the per-pass CR_OUTPUT_FIXED_SUM words
that the EXISTING Renderer.render(sample_begin=pP, sample_count=P) returns (never with the new call's output); every pixel
equals the plain relaxed render at samples = counts[pixel]; the work counters are those of the region-and-shard renders the
blocks took.  Adaptive renders need CR_SUM_RELAXED (tests/conftest.py makes the reference order the suite default, so
every render here names its order)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as M
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


def sized(sc, w, h, samples):
    """Odd sizes: edge tiles and edge blocks are partial."""
    sc.scene_cam.image_width, sc.scene_cam.image_height = w, h
    sc.scene_cam.set_samples(samples)
    return sc


def np_real(rt):
    return np.float64 if rt == A.CR_REAL_F64 else np.float32


def pass_words(r, cam, rt, P):
    """The per-pass fixed-point words of the frame, from the existing sample-shard renders: (passes, H, W, 3) uint64."""
    return np.stack([r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, sample_begin=p * P, sample_count=P, output_sum=FIXED)[0]
                     for p in range(cam.samples // P)])


def plain(r, cam, rt, samples):
    """The plain relaxed render of the frame with `samples` samples per pixel: (image, stats)."""
    keep = cam.samples
    cam.set_samples(samples)
    try:
        return r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    finally:
        cam.set_samples(keep)


def median_tolerance(words, P, min_samples, samples, block):
    """The median over blocks of D_b / (2^(S-12) qP 3 N_b) at the first judgement: about half the blocks stop there."""
    return float(np.median(np.array(M.first_judgement_ratios(words, P, min_samples, samples, block), dtype=np.float64)))


def check_mixed(r, sc, rt, P, min_samples, block, distinct=3):
    """Mixed decisions on the uploaded scene `sc`: counts and bytes against the model, every pixel against the plain render at
    its own count, the samples and the work counters against the region-and-shard renders of every block.  Returns the
    adaptive call's (image, counts, stats)."""
    cam = sc.scene_cam
    S, W, H = cam.samples, cam.image_width, cam.image_height
    words = pass_words(r, cam, rt, P)
    tol = median_tolerance(words, P, min_samples, S, block)
    want_counts, want, _ = M.adaptive(words, P, min_samples, S, block, tol, np_real(rt))
    # a condition on the inputs, before the library is asked: the decisions are mixed
    assert len(np.unique(want_counts)) >= distinct and (want_counts == S).any() and (want_counts == min_samples).any(), np.unique(want_counts)
    img, counts, st = r.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=tol, min_samples=min_samples, pass_samples=P, block=block,
                                        sum_order=RELAX)
    assert counts.dtype == np.int32 and counts.shape == (H, W) and img.shape == (H, W, 3) and img.dtype == np_real(rt)
    assert np.array_equal(counts, want_counts)
    assert img.tobytes() == want.tobytes()
    for n in np.unique(counts):   # S = 52: a pixel that stopped at n is the pixel of the plain render with n samples
        ref, _ = plain(r, cam, rt, int(n))
        assert np.array_equal(img[counts == n], ref[counts == n]), n
    rects = M.blocks_of(W, H, block)
    assert st["blocks"] == len(rects) and st["blocks_stopped"] == sum(1 for x0, y0, _, _ in rects if want_counts[y0, x0] < S)
    assert st["passes"] == int(want_counts.max()) // P
    assert st["render"]["samples"] == int(counts.sum(dtype=np.int64)) and st["render"]["nan_pixels"] == 0
    tot = {c: 0 for c in COUNTERS}
    for x0, y0, w, h in rects:   # what each block took: its pixels, the samples [0, n_b)
        _, rst = r.render_region(cam, (x0, y0, w, h), seed=SEED, real_type=rt, sum_order=RELAX, sample_begin=0,
                                 sample_count=int(want_counts[y0, x0]))
        for c in COUNTERS:
            tot[c] += rst[c]
    for c in COUNTERS:
        assert st["render"][c] == tot[c], (c, st["render"][c], tot[c])
    return img, counts, st


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("P,block", [(2, 8), (4, 16)])
def test_min_samples_equal_to_samples_is_the_plain_render(renderer, rt, name, P, block):
    sc = sized(scenes.mixed_scene(), 37, 29, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    ref, rst = plain(renderer, cam, rt, 16)
    img, counts, st = renderer.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=0.5, min_samples=16, pass_samples=P, block=block,
                                               sum_order=RELAX)
    assert img.tobytes() == ref.tobytes() and (counts == 16).all()
    for c in COUNTERS + ("samples", "bvh_entries", "scene_in_lds", "nan_pixels"):
        assert st["render"][c] == rst[c], c
    assert st["passes"] == 16 // P and st["blocks_stopped"] == 0 and st["blocks"] == -(-37 // block) * -(-29 // block)
    assert st["render"]["kernel_ms"] > 0 and st["judge_ms"] > 0


@pytest.mark.parametrize("rt,name", REALS)
def test_huge_tolerance_stops_every_block_at_min_samples(renderer, rt, name):
    sc = sized(scenes.mixed_scene(animate=True), 41, 31, 24)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    ref, rst = plain(renderer, cam, rt, 8)
    for tol in (1e300, 1.0):   # a product beyond 2^63; and means lie in [0, 1], so no difference exceeds 1
        img, counts, st = renderer.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=tol, min_samples=8, pass_samples=2, block=16,
                                                   sum_order=RELAX)
        assert (counts == 8).all() and img.tobytes() == ref.tobytes()
        assert st["render"]["samples"] == 41 * 31 * 8 and st["passes"] == 4 and st["blocks_stopped"] == st["blocks"] == 3 * 2
        for c in COUNTERS:
            assert st["render"][c] == rst[c], c


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("which", ["mixed-P2-block8", "moving-P3-block16"])
def test_mixed_decisions(renderer, rt, name, which):
    """(scene, samples, P, min_samples, block) chosen on the CPU with the relaxed oracle's words and the model, so that the
    model's counts take at least three values, min_samples and samples among them."""
    if which == "mixed-P2-block8":
        sc, P, min_samples, block = sized(scenes.mixed_scene(), 47, 37, 16), 2, 8, 8
    else:
        sc, P, min_samples, block = sized(scenes.moving_scene(frame=1), 37, 29, 24), 3, 6, 16
    renderer.upload_scene(sc.flatten())
    check_mixed(renderer, sc, rt, P, min_samples, block)


def ordered(sc):
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED
    return sc


def refitting(sc, refit):
    sc.bvh_mode = A.CR_BVH_SAH
    sc.scene_cam.refit_boxes = refit
    return sc


# the kernels that carry the active-tile list, one tiny frame each (scene, pass_samples, min_samples, block)
KERNELS = {
    "keyed-primitives": lambda: (sized(scenes.moving_scene(frame=1), 37, 29, 16), 2, 4, 8),
    "keyed-camera": lambda: (sized(scenes.keyed_camera_scene(n_from=6, n_at=4, width=8), 37, 29, 24), 2, 4, 8),
    "list": lambda: (sized(scenes.list_scene(frame=1), 37, 29, 24), 4, 8, 16),
    "wrapper": lambda: (sized(scenes.wrapped_scene(frame=1), 37, 29, 24), 4, 8, 16),
    "teapot-top-levels": lambda: (sized(teapot_orbit_movie(1, image_width=64, samples=4, sky=procedural_sky(64, 32)), 37, 29, 32), 4, 16, 8),
    "sah-ordered": lambda: (ordered(sized(scenes.mixed_scene(animate=True), 37, 29, 16)), 2, 8, 8),
    "refit-boxes": lambda: (refitting(sized(scenes.moving_scene(frame=1), 37, 29, 16), True), 2, 8, 8),
    "refit-rebuild": lambda: (refitting(sized(scenes.moving_scene(frame=1), 37, 29, 16), "rebuild"), 2, 8, 8),
}


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("which", list(KERNELS))
def test_every_carrying_kernel(renderer, rt, name, which):
    sc, P, min_samples, block = KERNELS[which]()
    renderer.upload_scene(sc.flatten())
    _, _, st = check_mixed(renderer, sc, rt, P, min_samples, block)
    if which == "teapot-top-levels":
        assert st["render"]["scene_in_lds"] == 2


@pytest.mark.parametrize("rt,name", REALS)
def test_global_memory_handle(monkeypatch, rt, name):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        sc = sized(scenes.moving_scene(frame=1), 37, 29, 16)
        r.upload_scene(sc.flatten())
        _, _, st = check_mixed(r, sc, rt, 2, 4, 8)
        assert st["render"]["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("tile", ["16x4", "8x8", "2x2", "1x8"])
def test_work_tile_override(monkeypatch, tile):
    """CRUCIBLE_SG_TILE names the work tile.  One that fits the block of 8 is used (8x8: one sample per group; 2x2; 1x8); one
    wider than the block (16x4) gives way to the default shape, since tiles must partition blocks.  The same counts and bytes."""
    monkeypatch.setenv("CRUCIBLE_SG_TILE", tile)
    r = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_SG_TILE")
    try:
        sc = sized(scenes.moving_scene(frame=1), 37, 29, 16)
        r.upload_scene(sc.flatten())
        check_mixed(r, sc, A.CR_REAL_F64, 2, 4, 8)
    finally:
        r.close()


@pytest.mark.parametrize("rt,name", REALS)
def test_scale_below_2_52(renderer, rt, name):
    """samples = 4096: S = 50.  Counts and bytes equal the model's.  The comparison with plain renders at samples = counts does
    not apply: a plain render of fewer than 2048 samples forms its sums at 2^52, four times finer than the 2^50 of this
    frame's sums, so its rounded per-sample terms differ from the ones added here."""
    sc = sized(scenes.mixed_scene(), 8, 8, 4096)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    P, min_samples = 256, 512
    words = pass_words(renderer, cam, rt, P)
    assert M.fx_log2(4096) == 50
    # the one block's ratio at n = 512 and at n = 2048: a tolerance between them stops it after the first judgement and before the end
    first = M.first_judgement_ratios(words, P, 512, 4096, 8)[0]
    later = M.first_judgement_ratios(words, P, 2048, 4096, 8)[0]
    assert later < first
    tol = (first + later) / 2
    want_counts, want, _ = M.adaptive(words, P, min_samples, 4096, 8, tol, np_real(rt))
    assert min_samples < want_counts[0, 0] <= 2048
    img, counts, st = renderer.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=tol, min_samples=min_samples, pass_samples=P, block=8,
                                               sum_order=RELAX)
    assert np.array_equal(counts, want_counts) and img.tobytes() == want.tobytes()
    assert st["render"]["samples"] == 64 * int(want_counts[0, 0]) and st["blocks"] == 1 and st["blocks_stopped"] == 1


def test_repeatable_without_counts_and_device_form(renderer):
    import torch
    sc = sized(scenes.moving_scene(frame=1), 41, 31, 24)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    for rt, tdt in ((A.CR_REAL_F64, torch.float64), (A.CR_REAL_F32, torch.float32)):
        tol = median_tolerance(pass_words(renderer, cam, rt, 2), 2, 8, 24, 8)
        kw = dict(seed=SEED, real_type=rt, tolerance=tol, min_samples=8, pass_samples=2, block=8, sum_order=RELAX)
        a, ca, sta = renderer.render_adaptive(cam, **kw)
        b, cb, stb = renderer.render_adaptive(cam, **kw)
        assert len(np.unique(ca)) >= 2
        assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb)
        for c in COUNTERS + ("samples",):
            assert sta["render"][c] == stb["render"][c], c
        c, none, _ = renderer.render_adaptive(cam, want_counts=False, **kw)
        assert none is None and c.tobytes() == a.tobytes()
        d, _, _ = renderer.render_adaptive(cam, want_counts=False, want_stats=False, **kw)
        assert d.tobytes() == a.tobytes()
        d_img = torch.full((31, 41, 3), -1.0, dtype=tdt, device="cuda:0")
        d_cnt = torch.full((31, 41), -1, dtype=torch.int32, device="cuda:0")
        guard = torch.full((64,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        std = renderer.render_adaptive_device(cam, d_img.data_ptr(), d_cnt.data_ptr(), **kw)
        renderer.synchronize()
        assert d_img.cpu().numpy().tobytes() == a.tobytes() and np.array_equal(d_cnt.cpu().numpy(), ca) and (guard.cpu().numpy() == -1).all()
        assert std["render"]["samples"] == sta["render"]["samples"] and std["passes"] == sta["passes"]
        d_img.fill_(-1.0)
        torch.cuda.synchronize()
        renderer.render_adaptive_device(cam, d_img.data_ptr(), None, want_stats=False, **kw)
        renderer.synchronize()
        assert d_img.cpu().numpy().tobytes() == a.tobytes()
        assert renderer.last_kernel_ms() > 0


def test_refusals_leave_the_handle_usable(renderer, monkeypatch):
    lib = renderer.lib
    sc = sized(scenes.moving_scene(frame=1), 37, 29, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    rt = A.CR_REAL_F64

    def others():
        """A plain render, a frame batch and a region render on the handle."""
        return (renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)[0].tobytes(),
                renderer.render_frames(cam, [1, 0], seed=SEED, real_type=rt, sum_order=RELAX)[0].tobytes(),
                renderer.render_region(cam, (5, 3, 13, 9), seed=SEED, real_type=rt, sum_order=RELAX)[0].tobytes())

    before = others()
    cd, p = cam.desc(), cam.params(SEED, rt, sum_order=RELAX)
    out = np.empty((29, 37, 3), dtype=np.float64)
    cnt = np.empty((29, 37), dtype=np.int32)
    good = dict(min_samples=8, pass_samples=2, block_log2=4, _reserved=0, tolerance=0.01)

    def rc_of(fn, cdesc=cd, params=p, dst=out, null_adaptive=False, **change):
        ap = A.CrAdaptiveParams(**{**good, **change})
        return fn(renderer.h, C.byref(cdesc) if cdesc is not None else None, C.byref(params) if params is not None else None,
                  None if null_adaptive else C.byref(ap), dst.ctypes.data_as(C.c_void_p) if dst is not None else None,
                  cnt.ctypes.data_as(C.c_void_p), None)

    def params(**kw):
        q = cam.params(SEED, rt, sum_order=RELAX)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    invalid = [dict(null_adaptive=True), dict(block_log2=1), dict(block_log2=2), dict(block_log2=6), dict(block_log2=-1), dict(_reserved=1),
               dict(pass_samples=0), dict(pass_samples=-2), dict(pass_samples=3),            # 16 is no multiple of 6
               dict(min_samples=0), dict(min_samples=-4), dict(min_samples=6), dict(min_samples=2),   # 2 is no multiple of 2P = 4
               dict(min_samples=20), dict(tolerance=-1e-9), dict(tolerance=float("inf")), dict(tolerance=float("nan")),
               dict(cdesc=None), dict(params=None), dict(dst=None),
               dict(params=params(samples=0, sample_count=0)), dict(params=params(samples=18, sample_count=18)),   # 18 is no multiple of 4
               dict(params=params(sample_begin=14, sample_count=4)),                          # what cr_render_device rejects
               dict(params=params(max_depth=-1)), dict(params=params(real_type=7))]
    unsupported = [dict(params=params(sum_order=A.CR_SUM_REFERENCE_ORDER)), dict(params=params(sum_order=A.CR_SUM_DEFAULT)),
                   dict(params=params(sample_begin=4, sample_count=12)), dict(params=params(sample_count=12)),
                   dict(params=params(output_sum=1)), dict(params=params(output_sum=FIXED))]
    for fn in (lib.cr_render_adaptive_host, lib.cr_render_adaptive_device):
        for case in invalid:
            assert rc_of(fn, **case) == A.CR_ERR_INVALID_ARG, case
            assert others() == before, case
        for case in unsupported:
            assert rc_of(fn, **case) == A.CR_ERR_UNSUPPORTED, case
            assert others() == before, case
    for bad_block in (4, 12, 64):   # the mirror hands a side that is not 8, 16 or 32 on as a block_log2 the library refuses
        with pytest.raises(CrucibleError) as e:
            renderer.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=0.01, min_samples=8, pass_samples=2, block=bad_block, sum_order=RELAX)
        assert e.value.code == A.CR_ERR_INVALID_ARG
    # the cross-check pipelines
    for pipe in ("queue", "wavefront"):
        monkeypatch.setenv("CRUCIBLE_PIPELINE", pipe)
        other = Renderer(0)
        monkeypatch.delenv("CRUCIBLE_PIPELINE")
        try:
            other.upload_scene(sc.flatten())
            with pytest.raises(CrucibleError) as e:
                other.render_adaptive(cam, seed=SEED, real_type=rt, tolerance=0.01, min_samples=8, pass_samples=2, sum_order=RELAX)
            assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_adaptive" in str(e.value)
        finally:
            other.close()
    # a handle without a scene
    empty = Renderer(0)
    try:
        assert lib.cr_render_adaptive_host(empty.h, C.byref(cd), C.byref(p), C.byref(A.CrAdaptiveParams(**good)), out.ctypes.data_as(C.c_void_p),
                                           None, None) == A.CR_ERR_NO_SCENE
    finally:
        empty.close()
    # and after a successful call (block_log2 0 is the default, 16 pixels)
    st = A.CrAdaptiveStats()
    assert lib.cr_render_adaptive_host(renderer.h, C.byref(cd), C.byref(p), C.byref(A.CrAdaptiveParams(**{**good, "block_log2": 0})),
                                       out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(st)) == A.CR_OK
    assert st.blocks == 3 * 2 and set(np.unique(cnt)) <= {8, 12, 16}
    assert others() == before
