"""cr_render_adaptive_region_device / _host: a region of a frame to a noise target, judged as if the region were the frame
(blocks anchored at the region's origin).  Everything is bit for bit and without a tolerance.  The model is the existing
tests/adaptive_model.py, fed with the region's per-pass CR_OUTPUT_FIXED_SUM words from the EXISTING
Renderer.render_region(sample_begin=pP, sample_count=P) -- the region's words are its "frame" -- and never with the new
call's output.  The seed, the regions and the sizes were chosen on the CPU with the relaxed oracle so that the decisions are
mixed; each test checks that condition on its inputs before it asks the library.  Adaptive renders need CR_SUM_RELAXED
(tests/conftest.py makes the reference order the suite default, so every render here names its order)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as M
import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer

pytestmark = pytest.mark.gpu

SEED = 7
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
RELAX = A.CR_SUM_RELAXED
FIXED = A.CR_OUTPUT_FIXED_SUM
W, H = 61, 45                     # no multiple of a tile's or a block's side
UNALIGNED = (5, 3, 43, 37)        # partial tiles and blocks at the region's own right and bottom edge
QUADRANTS = [(0, 0, 32, 32), (32, 0, 29, 32), (0, 32, 32, 13), (32, 32, 29, 13)]   # a 2 x 2 partition at multiples of 8, 16 and 32


def sized(sc, w, h, samples):
    sc.scene_cam.image_width, sc.scene_cam.image_height = w, h
    sc.scene_cam.set_samples(samples)
    return sc


def np_real(rt):
    return np.float64 if rt == A.CR_REAL_F64 else np.float32


def region_words(r, cam, rt, P, region):
    """The per-pass fixed-point words of the region, from the existing region-and-shard renders: (passes, h, w, 3) uint64."""
    return np.stack([r.render_region(cam, region, seed=SEED, real_type=rt, sum_order=RELAX, sample_begin=p * P, sample_count=P,
                                     output_sum=FIXED)[0] for p in range(cam.samples // P)])


def plain_region(r, cam, rt, region, samples):
    """The plain relaxed region render with `samples` samples per pixel: (image, stats)."""
    keep = cam.samples
    cam.set_samples(samples)
    try:
        return r.render_region(cam, region, seed=SEED, real_type=rt, sum_order=RELAX)
    finally:
        cam.set_samples(keep)


def median_tolerance(words, P, min_samples, samples, block):
    """The median over blocks of D_b / (2^(S-12) qP 3 N_b) at the first judgement: about half the blocks stop there."""
    return float(np.median(np.array(M.first_judgement_ratios(words, P, min_samples, samples, block), dtype=np.float64)))


def kw_of(rt, tol, P, min_samples, block):
    return dict(seed=SEED, real_type=rt, tolerance=tol, min_samples=min_samples, pass_samples=P, block=block, sum_order=RELAX)


def crop(a, region):
    x0, y0, w, h = region
    return a[y0:y0 + h, x0:x0 + w]


def check_region(r, sc, rt, P, min_samples, block, region, distinct=3):
    """Mixed decisions over `region` of the uploaded scene `sc`: counts and bytes against the model, every pixel against
    render_region at its own count, samples and work counters against render_region of every block with sample_count = n_b.
    Returns the call's (image, counts, stats)."""
    cam = sc.scene_cam
    S = cam.samples
    x0, y0, w, h = region
    words = region_words(r, cam, rt, P, region)
    tol = median_tolerance(words, P, min_samples, S, block)
    want_counts, want, _ = M.adaptive(words, P, min_samples, S, block, tol, np_real(rt))
    # a condition on the inputs, before the library is asked: the decisions are mixed
    assert len(np.unique(want_counts)) >= distinct and (want_counts == S).any() and (want_counts == min_samples).any(), np.unique(want_counts)
    img, counts, st = r.render_adaptive_region(cam, region, **kw_of(rt, tol, P, min_samples, block))
    assert counts.dtype == np.int32 and counts.shape == (h, w) and img.shape == (h, w, 3) and img.dtype == np_real(rt)
    assert np.array_equal(counts, want_counts)
    assert img.tobytes() == want.tobytes()
    for n in np.unique(counts):   # S = 52: a pixel that stopped at n is the pixel of the region render with n samples
        ref, _ = plain_region(r, cam, rt, region, int(n))
        assert np.array_equal(img[counts == n], ref[counts == n]), n
    rects = M.blocks_of(w, h, block)   # anchored at the region's origin
    assert st["blocks"] == len(rects) and st["blocks_stopped"] == sum(1 for bx, by, _, _ in rects if want_counts[by, bx] < S)
    assert st["passes"] == int(want_counts.max()) // P
    assert st["render"]["samples"] == int(counts.sum(dtype=np.int64)) and st["render"]["nan_pixels"] == 0
    tot = {c: 0 for c in COUNTERS}
    for bx, by, bw, bh in rects:   # what each block took: its pixels inside the region, the samples [0, n_b)
        _, rst = r.render_region(cam, (x0 + bx, y0 + by, bw, bh), seed=SEED, real_type=rt, sum_order=RELAX, sample_begin=0,
                                 sample_count=int(want_counts[by, bx]))
        for c in COUNTERS:
            tot[c] += rst[c]
    for c in COUNTERS:
        assert st["render"][c] == tot[c], (c, st["render"][c], tot[c])
    return img, counts, st


def frame_setup(r, rt, samples, P, min_samples, block):
    """mixed_scene at 61 x 45 on the handle, and a tolerance from the whole frame's words under which the model's whole-frame
    counts take at least three values: (scene, kw for the adaptive calls)."""
    sc = sized(scenes.mixed_scene(), W, H, samples)
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    words = region_words(r, cam, rt, P, (0, 0, W, H))
    tol = median_tolerance(words, P, min_samples, samples, block)
    want_counts, _, _ = M.adaptive(words, P, min_samples, samples, block, tol, np_real(rt))
    assert len(np.unique(want_counts)) >= 3, np.unique(want_counts)
    return sc, kw_of(rt, tol, P, min_samples, block)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("samples,min_samples,block", [(16, 8, 8), (24, 12, 16)])
def test_mixed_decisions_on_an_unaligned_region(renderer, rt, name, samples, min_samples, block):
    sc = sized(scenes.mixed_scene(), W, H, samples)
    renderer.upload_scene(sc.flatten())
    check_region(renderer, sc, rt, 2, min_samples, block, UNALIGNED)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("block", [8, 16])
def test_aligned_regions_are_the_frames_own_pixels(renderer, rt, name, block):
    """An aligned interior region, and one that reaches the frame's right and bottom edge with partial blocks."""
    sc, kw = frame_setup(renderer, rt, 24, 2, 12, block)
    cam = sc.scene_cam
    whole, whole_counts, _ = renderer.render_adaptive(cam, **kw)
    assert len(np.unique(whole_counts)) >= 3
    for region in ((16, 16, 32, 16), (48, 32, 13, 13)):
        img, counts, st = renderer.render_adaptive_region(cam, region, **kw)
        assert img.tobytes() == np.ascontiguousarray(crop(whole, region)).tobytes(), region
        assert np.array_equal(counts, crop(whole_counts, region)), region
        assert st["render"]["samples"] == int(crop(whole_counts, region).sum(dtype=np.int64))


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("block", [8, 16])
def test_a_partition_at_block_multiples_is_the_whole_frame(renderer, rt, name, block):
    sc, kw = frame_setup(renderer, rt, 24, 2, 12, block)
    cam = sc.scene_cam
    whole, whole_counts, wst = renderer.render_adaptive(cam, **kw)
    img = np.full_like(whole, -1)
    counts = np.full_like(whole_counts, -1)
    tot = {k: 0 for k in COUNTERS + ("samples", "blocks", "blocks_stopped")}
    passes = []
    for region in QUADRANTS:
        part, cnt, st = renderer.render_adaptive_region(cam, region, **kw)
        crop(img, region)[...] = part
        crop(counts, region)[...] = cnt
        for k in COUNTERS + ("samples",):
            tot[k] += st["render"][k]
        tot["blocks"] += st["blocks"]
        tot["blocks_stopped"] += st["blocks_stopped"]
        passes.append(st["passes"])
    assert img.tobytes() == whole.tobytes() and np.array_equal(counts, whole_counts)
    for k in COUNTERS + ("samples",):
        assert tot[k] == wst["render"][k], k
    assert tot["blocks"] == wst["blocks"] and tot["blocks_stopped"] == wst["blocks_stopped"]
    assert max(passes) == wst["passes"]   # passes does not add up: the frame runs as long as its slowest block
    timg, tcounts, tst = renderer.render_tiled(cam, (32, 32), seed=SEED, real_type=rt, sum_order=RELAX,
                                               adaptive={k: kw[k] for k in ("tolerance", "min_samples", "pass_samples", "block")})
    assert timg.tobytes() == whole.tobytes() and np.array_equal(tcounts, whole_counts) and tcounts.dtype == np.int32
    for k in COUNTERS + ("samples",):
        assert tst["render"][k] == wst["render"][k], k
    assert tst["blocks"] == wst["blocks"] and tst["blocks_stopped"] == wst["blocks_stopped"] and tst["passes"] == sum(passes)
    # without `adaptive` render_tiled is what it was
    plain, pst = renderer.render_tiled(cam, (32, 32), seed=SEED, real_type=rt, sum_order=RELAX)
    ref, rst = renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)
    assert plain.tobytes() == ref.tobytes() and pst["samples"] == rst["samples"] == W * H * 24


@pytest.mark.parametrize("rt,name", REALS)
def test_a_region_that_is_the_whole_frame(renderer, rt, name):
    sc, kw = frame_setup(renderer, rt, 24, 2, 12, 16)
    cam = sc.scene_cam
    whole, whole_counts, wst = renderer.render_adaptive(cam, **kw)
    img, counts, st = renderer.render_adaptive_region(cam, (0, 0, W, H), **kw)
    assert img.tobytes() == whole.tobytes() and np.array_equal(counts, whole_counts)
    for k in ("passes", "blocks", "blocks_stopped"):
        assert st[k] == wst[k], k
    for k in COUNTERS + ("samples", "nan_pixels", "bvh_entries", "scene_in_lds"):
        assert st["render"][k] == wst["render"][k], k
    assert st["render"]["kernel_ms"] > 0 and st["judge_ms"] > 0


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("P,block", [(2, 8), (4, 16)])
def test_min_samples_equal_to_samples_is_the_region_render(renderer, rt, name, P, block):
    sc = sized(scenes.mixed_scene(), W, H, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    ref, rst = plain_region(renderer, cam, rt, UNALIGNED, 16)
    img, counts, st = renderer.render_adaptive_region(cam, UNALIGNED, **kw_of(rt, 0.5, P, 16, block))
    assert img.tobytes() == ref.tobytes() and (counts == 16).all()
    for c in COUNTERS + ("samples", "bvh_entries", "scene_in_lds", "nan_pixels"):
        assert st["render"][c] == rst[c], c
    assert st["passes"] == 16 // P and st["blocks_stopped"] == 0 and st["blocks"] == -(-43 // block) * -(-37 // block)


@pytest.mark.parametrize("rt,name", REALS)
def test_huge_tolerance_stops_every_block_at_min_samples(renderer, rt, name):
    sc = sized(scenes.mixed_scene(animate=True), W, H, 24)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    ref, rst = plain_region(renderer, cam, rt, UNALIGNED, 8)
    for tol in (1e300, 1.0):   # a product beyond 2^63; and means lie in [0, 1], so no difference exceeds 1
        img, counts, st = renderer.render_adaptive_region(cam, UNALIGNED, **kw_of(rt, tol, 2, 8, 16))
        assert (counts == 8).all() and img.tobytes() == ref.tobytes()
        assert st["render"]["samples"] == 43 * 37 * 8 and st["passes"] == 4 and st["blocks_stopped"] == st["blocks"] == 3 * 3
        for c in COUNTERS:
            assert st["render"][c] == rst[c], c


def ordered(sc):
    sc.bvh_mode = A.CR_BVH_SAH_ORDERED
    return sc


def refitting(sc, refit):
    sc.bvh_mode = A.CR_BVH_SAH
    sc.scene_cam.refit_boxes = refit
    return sc


SMALL = (5, 3, 27, 21)   # of a 37 x 29 frame
# one tiny frame each: (scene, pass_samples, min_samples, block)
VARIANTS = {
    "keyed-primitives-refit": lambda: (refitting(sized(scenes.moving_scene(frame=1), 37, 29, 16), True), 2, 8, 8),
    "keyed-primitives-rebuild": lambda: (refitting(sized(scenes.moving_scene(frame=1), 37, 29, 16), "rebuild"), 2, 8, 8),
    "keyed-camera": lambda: (sized(scenes.keyed_camera_scene(n_from=6, n_at=4, width=8), 37, 29, 24), 2, 8, 8),
    "list": lambda: (sized(scenes.list_scene(frame=1), 37, 29, 24), 4, 8, 16),
    "sah-ordered": lambda: (ordered(sized(scenes.mixed_scene(animate=True), 37, 29, 12)), 2, 8, 8),
}


@pytest.mark.parametrize("which", list(VARIANTS))
def test_scene_variants(renderer, which):
    """The kernels that carry the region's offsets and the active-tile list, one case each: at least two distinct counts."""
    sc, P, min_samples, block = VARIANTS[which]()
    renderer.upload_scene(sc.flatten())
    check_region(renderer, sc, A.CR_REAL_F64 if which != "list" else A.CR_REAL_F32, P, min_samples, block, SMALL, distinct=2)
    if which == "keyed-primitives-rebuild":
        assert renderer.frame_build_info(A.CR_REAL_F64)["n_wrappers"] > 0
        assert len(renderer.export_render_bvh(A.CR_REAL_F64)[1]) > 0


def test_global_memory_handle(monkeypatch):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        sc = sized(scenes.moving_scene(frame=1), 37, 29, 16)
        r.upload_scene(sc.flatten())
        _, _, st = check_region(r, sc, A.CR_REAL_F64, 2, 8, 8, SMALL, distinct=2)
        assert st["render"]["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("rt,name", REALS)
def test_scale_below_2_52(renderer, rt, name):
    """samples = 4096: S = 50, on a region of one 8 x 8 block.  Counts and bytes equal the model's (a plain render of fewer than
    2048 samples forms its sums at 2^52, so the comparison with render_region at samples = counts does not apply)."""
    sc = sized(scenes.mixed_scene(), 21, 17, 4096)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    region, P, min_samples = (9, 5, 8, 8), 256, 512
    words = region_words(renderer, cam, rt, P, region)
    assert M.fx_log2(4096) == 50
    first = M.first_judgement_ratios(words, P, 512, 4096, 8)[0]
    later = M.first_judgement_ratios(words, P, 2048, 4096, 8)[0]
    assert later < first
    tol = (first + later) / 2   # stops the block after the first judgement and before the end
    want_counts, want, _ = M.adaptive(words, P, min_samples, 4096, 8, tol, np_real(rt))
    assert min_samples < want_counts[0, 0] <= 2048
    img, counts, st = renderer.render_adaptive_region(cam, region, **kw_of(rt, tol, P, min_samples, 8))
    assert np.array_equal(counts, want_counts) and img.tobytes() == want.tobytes()
    assert st["render"]["samples"] == 64 * int(want_counts[0, 0]) and st["blocks"] == 1 and st["blocks_stopped"] == 1


def test_repeatable_without_counts_and_device_form(renderer):
    import torch
    sc = sized(scenes.moving_scene(frame=1), 41, 31, 24)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    region = (3, 5, 29, 22)
    for rt, tdt in ((A.CR_REAL_F64, torch.float64), (A.CR_REAL_F32, torch.float32)):
        tol = median_tolerance(region_words(renderer, cam, rt, 2, region), 2, 8, 24, 8)
        kw = kw_of(rt, tol, 2, 8, 8)
        a, ca, sta = renderer.render_adaptive_region(cam, region, **kw)
        b, cb, stb = renderer.render_adaptive_region(cam, region, **kw)
        assert len(np.unique(ca)) >= 2
        assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb)
        for c in COUNTERS + ("samples",):
            assert sta["render"][c] == stb["render"][c], c
        c, none, _ = renderer.render_adaptive_region(cam, region, want_counts=False, **kw)
        assert none is None and c.tobytes() == a.tobytes()
        d, _, _ = renderer.render_adaptive_region(cam, region, want_counts=False, want_stats=False, **kw)
        assert d.tobytes() == a.tobytes()
        d_img = torch.full((22, 29, 3), -1.0, dtype=tdt, device="cuda:0")
        d_cnt = torch.full((22, 29), -1, dtype=torch.int32, device="cuda:0")
        guard = torch.full((64,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        std = renderer.render_adaptive_region_device(cam, region, d_img.data_ptr(), d_cnt.data_ptr(), **kw)
        renderer.synchronize()
        assert d_img.cpu().numpy().tobytes() == a.tobytes() and np.array_equal(d_cnt.cpu().numpy(), ca) and (guard.cpu().numpy() == -1).all()
        assert std["render"]["samples"] == sta["render"]["samples"] and std["passes"] == sta["passes"]
        d_img.fill_(-1.0)
        torch.cuda.synchronize()
        renderer.render_adaptive_region_device(cam, region, d_img.data_ptr(), None, want_stats=False, **kw)
        renderer.synchronize()
        assert d_img.cpu().numpy().tobytes() == a.tobytes()
        assert renderer.last_kernel_ms() > 0


def test_editor_loop(renderer):
    """An adaptive frame, an edit of one sphere through cr_update_primitives, the aligned region around it re-rendered
    adaptively and pasted in: on exactly those pixels the whole-frame adaptive render of the edited scene."""
    rt, block = A.CR_REAL_F64, 16
    sc, kw = frame_setup(renderer, rt, 24, 2, 12, block)
    cam = sc.scene_cam
    frame, counts, _ = renderer.render_adaptive(cam, **kw)
    flat = sc.flatten()
    k = next(i for i in range(flat.desc.n_prims) if flat.desc.prims[i].kind == A.CR_PRIM_SPHERE and flat.desc.prims[i].v[3] == 0.3)   # "mirror"
    row = np.array(list(flat.desc.prims[k].v), dtype=np.float64)
    row[1] += 0.25 * row[3]   # up by a quarter of its radius
    renderer.update_primitives([k], row.reshape(1, 9))
    edited, edited_counts, _ = renderer.render_adaptive(cam, **kw)
    change = np.abs(edited - frame).sum(axis=2)
    assert change.max() > 0
    # the aligned region around the edit: the block of the pixel that changed most and its neighbours, clipped to the frame
    cy, cx = np.unravel_index(int(np.argmax(change)), change.shape)
    x0, y0 = max(0, int(cx) // block * block - block), max(0, int(cy) // block * block - block)
    x1, y1 = min(W, int(cx) // block * block + 2 * block), min(H, int(cy) // block * block + 2 * block)
    region = (x0, y0, x1 - x0, y1 - y0)
    part, part_counts, _ = renderer.render_adaptive_region(cam, region, **kw)
    pasted, pasted_counts = frame.copy(), counts.copy()
    crop(pasted, region)[...] = part
    crop(pasted_counts, region)[...] = part_counts
    assert np.ascontiguousarray(crop(pasted, region)).tobytes() == np.ascontiguousarray(crop(edited, region)).tobytes()
    assert np.array_equal(crop(pasted_counts, region), crop(edited_counts, region))
    assert (crop(pasted, region) != crop(frame, region)).any()   # the patch shows the edit
    outside = np.ones((H, W), dtype=bool)
    crop(outside, region)[...] = False
    assert np.array_equal(pasted[outside], frame[outside]) and np.array_equal(pasted_counts[outside], counts[outside])


def handle_with(monkeypatch, name, value):
    monkeypatch.setenv(name, value)   # read by cr_create
    r = Renderer(0)
    monkeypatch.delenv(name)
    return r


@pytest.mark.parametrize("tile", ["8x8", "2x2", "1x8", "4x2"])
def test_work_tile_override_that_fits_the_block(renderer, monkeypatch, tile):
    sc = sized(scenes.mixed_scene(), W, H, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    kw = kw_of(A.CR_REAL_F64, median_tolerance(region_words(renderer, cam, A.CR_REAL_F64, 2, UNALIGNED), 2, 8, 16, 8), 2, 8, 8)
    want, want_counts, wst = renderer.render_adaptive_region(cam, UNALIGNED, **kw)
    assert len(np.unique(want_counts)) >= 3
    r = handle_with(monkeypatch, "CRUCIBLE_SG_TILE", tile)
    try:
        r.upload_scene(sc.flatten())
        img, counts, st = r.render_adaptive_region(cam, UNALIGNED, **kw)
        assert img.tobytes() == want.tobytes() and np.array_equal(counts, want_counts)
        for c in COUNTERS + ("samples",):
            assert st["render"][c] == wst["render"][c], c
    finally:
        r.close()


def test_work_tile_override_that_does_not_fit_the_block_is_refused(monkeypatch):
    sc = sized(scenes.mixed_scene(), W, H, 16)
    cam = sc.scene_cam
    r = handle_with(monkeypatch, "CRUCIBLE_SG_TILE", "16x4")
    try:
        r.upload_scene(sc.flatten())
        before = r.render_region(cam, UNALIGNED, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)[0].tobytes()
        with pytest.raises(CrucibleError) as e:
            r.render_adaptive_region(cam, UNALIGNED, **kw_of(A.CR_REAL_F64, 0.1, 2, 8, 8))
        assert e.value.code == A.CR_ERR_UNSUPPORTED and "CRUCIBLE_SG_TILE" in str(e.value)
        assert r.render_region(cam, UNALIGNED, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)[0].tobytes() == before
        _, counts, _ = r.render_adaptive_region(cam, UNALIGNED, **kw_of(A.CR_REAL_F64, 0.1, 2, 8, 16))   # a block it fits
        assert counts.shape == (37, 43)
    finally:
        r.close()




@pytest.mark.parametrize("samples,P,limit", [(32, 8, 8000), (48, 12, 7040)], ids=["two-launches", "three-launches"])
def test_a_pass_split_by_the_work_counter(renderer, monkeypatch, samples, P, limit):
    """43 x 37 pixels are 11 x 10 work tiles of 4 x 4 pixels: 7040 work items per group of four samples.  A work counter that
    holds one group cuts a pass of 8 samples into two launches and one of 12 into three.  The same bytes, counts and counters."""
    sc = sized(scenes.mixed_scene(), W, H, samples)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    rt = A.CR_REAL_F64
    kw = kw_of(rt, median_tolerance(region_words(renderer, cam, rt, P, UNALIGNED), P, 2 * P, samples, 8), P, 2 * P, 8)
    want, want_counts, wst = renderer.render_adaptive_region(cam, UNALIGNED, **kw)
    assert len(np.unique(want_counts)) >= 2
    r = handle_with(monkeypatch, "CRUCIBLE_WORK_COUNTER_MAX", str(limit))
    try:
        r.upload_scene(sc.flatten())
        img, counts, st = r.render_adaptive_region(cam, UNALIGNED, **kw)
        assert img.tobytes() == want.tobytes() and np.array_equal(counts, want_counts)
        for c in COUNTERS + ("samples",):
            assert st["render"][c] == wst["render"][c], c
        assert (st["passes"], st["blocks"], st["blocks_stopped"]) == (wst["passes"], wst["blocks"], wst["blocks_stopped"])
    finally:
        r.close()
    # a counter that does not hold one group of the region's tiles: refused, as a region render refuses it
    r = handle_with(monkeypatch, "CRUCIBLE_WORK_COUNTER_MAX", "7000")
    try:
        r.upload_scene(sc.flatten())
        with pytest.raises(CrucibleError) as e:
            r.render_adaptive_region(cam, UNALIGNED, **kw)
        assert e.value.code == A.CR_ERR_UNSUPPORTED
    finally:
        r.close()


def test_refusals_leave_the_handle_usable(renderer, monkeypatch):
    lib = renderer.lib
    sc = sized(scenes.moving_scene(frame=1), 37, 29, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    rt = A.CR_REAL_F64
    akw = kw_of(rt, 0.05, 2, 8, 8)

    def others():
        """A plain render, a region render and a whole-frame adaptive render on the handle."""
        img, counts, _ = renderer.render_adaptive(cam, **akw)
        return (renderer.render(cam, seed=SEED, real_type=rt, sum_order=RELAX)[0].tobytes(),
                renderer.render_region(cam, (5, 3, 13, 9), seed=SEED, real_type=rt, sum_order=RELAX)[0].tobytes(),
                img.tobytes(), counts.tobytes())

    before = others()
    cd, p = cam.desc(), cam.params(SEED, rt, sum_order=RELAX)
    out = np.empty((29, 37, 3), dtype=np.float64)
    cnt = np.empty((29, 37), dtype=np.int32)
    good = dict(min_samples=8, pass_samples=2, block_log2=4, _reserved=0, tolerance=0.01)
    good_region = (5, 3, 13, 9)

    def rc_of(fn, cdesc=cd, params=p, dst=out, null_adaptive=False, region=good_region, **change):
        ap = A.CrAdaptiveParams(**{**good, **change})
        reg = A.CrRegion(*region) if region is not None else None
        return fn(renderer.h, C.byref(cdesc) if cdesc is not None else None, C.byref(params) if params is not None else None,
                  None if null_adaptive else C.byref(ap), C.byref(reg) if reg is not None else None,
                  dst.ctypes.data_as(C.c_void_p) if dst is not None else None, cnt.ctypes.data_as(C.c_void_p), None)

    def params(**kw):
        q = cam.params(SEED, rt, sum_order=RELAX)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def frame(w, h):
        d = cam.desc()
        d.image_width, d.image_height = w, h
        return d

    i32 = 2 ** 31 - 1
    # everything cr_render_adaptive_device refuses ...
    invalid = [dict(null_adaptive=True), dict(block_log2=1), dict(block_log2=2), dict(block_log2=6), dict(block_log2=-1), dict(_reserved=1),
               dict(pass_samples=0), dict(pass_samples=-2), dict(pass_samples=3),            # 16 is no multiple of 6
               dict(min_samples=0), dict(min_samples=-4), dict(min_samples=6), dict(min_samples=2),   # 2 is no multiple of 2P = 4
               dict(min_samples=20), dict(tolerance=-1e-9), dict(tolerance=float("inf")), dict(tolerance=float("nan")),
               dict(cdesc=None), dict(params=None), dict(dst=None),
               dict(params=params(samples=0, sample_count=0)), dict(params=params(samples=18, sample_count=18)),   # 18 is no multiple of 4
               dict(params=params(sample_begin=14, sample_count=4)),                          # what cr_render_device rejects
               dict(params=params(max_depth=-1)), dict(params=params(real_type=7)),
               # ... and everything cr_render_region_device refuses about the region
               dict(region=None), dict(region=(5, 3, 0, 9)), dict(region=(5, 3, 13, 0)), dict(region=(5, 3, -1, 9)), dict(region=(5, 3, 13, -9)),
               dict(region=(-1, 3, 13, 9)), dict(region=(5, -1, 13, 9)),
               dict(region=(25, 3, 13, 9)), dict(region=(5, 21, 13, 9)), dict(region=(0, 0, 38, 29)), dict(region=(0, 0, 37, 30)),
               dict(region=(i32, 3, 1, 1)), dict(region=(1, 1, i32, 1)), dict(region=(5, i32, 1, 1)), dict(region=(1, 1, 1, i32)),   # sums in 64 bits
               dict(cdesc=frame(16384, 8192), region=(0, 0, 16384, 4097)),                    # more than 2^26 pixels in the region
               dict(cdesc=frame(65536, 32768)),                                               # a frame of 2^31 pixels
               dict(cdesc=frame(0, 29)), dict(cdesc=frame(37, -1))]
    unsupported = [dict(params=params(sum_order=A.CR_SUM_REFERENCE_ORDER)), dict(params=params(sum_order=A.CR_SUM_DEFAULT)),
                   dict(params=params(sample_begin=4, sample_count=12)), dict(params=params(sample_count=12)),
                   dict(params=params(output_sum=1)), dict(params=params(output_sum=FIXED))]
    for fn in (lib.cr_render_adaptive_region_host, lib.cr_render_adaptive_region_device):
        for case in invalid:
            assert rc_of(fn, **case) == A.CR_ERR_INVALID_ARG, case
            assert others() == before, case
        for case in unsupported:
            assert rc_of(fn, **case) == A.CR_ERR_UNSUPPORTED, case
            assert others() == before, case
    # the refusals carry the parents' words
    assert rc_of(lib.cr_render_adaptive_region_host, region=(25, 3, 13, 9)) == A.CR_ERR_INVALID_ARG
    assert b"outside the frame" in lib.cr_last_error(renderer.h)
    for bad_block in (4, 12, 64):   # the mirror hands a side that is not 8, 16 or 32 on as a block_log2 the library refuses
        with pytest.raises(CrucibleError) as e:
            renderer.render_adaptive_region(cam, good_region, **{**akw, "block": bad_block})
        assert e.value.code == A.CR_ERR_INVALID_ARG
    with pytest.raises(CrucibleError) as e:
        renderer.render_adaptive_region(cam, None, **akw)
    assert e.value.code == A.CR_ERR_INVALID_ARG
    # the cross-check pipelines
    for pipe in ("queue", "wavefront"):
        other = handle_with(monkeypatch, "CRUCIBLE_PIPELINE", pipe)
        try:
            other.upload_scene(sc.flatten())
            with pytest.raises(CrucibleError) as e:
                other.render_adaptive_region(cam, good_region, **akw)
            assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_adaptive" in str(e.value)
        finally:
            other.close()
    # a handle without a scene
    empty = Renderer(0)
    try:
        reg = A.CrRegion(*good_region)
        assert lib.cr_render_adaptive_region_host(empty.h, C.byref(cd), C.byref(p), C.byref(A.CrAdaptiveParams(**good)), C.byref(reg),
                                                  out.ctypes.data_as(C.c_void_p), None, None) == A.CR_ERR_NO_SCENE
    finally:
        empty.close()
    # a frame beyond 2^26 pixels is accepted, as for regions; and after all of this a good call is what the model says
    big = frame(16384, 8192)
    assert rc_of(lib.cr_render_adaptive_region_host, cdesc=big, region=(8000, 4000, 13, 9)) == A.CR_OK
    assert others() == before
    check_region(renderer, sc, rt, 2, 8, 8, SMALL, distinct=2)
