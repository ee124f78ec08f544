"""cr_render_aov_counts_*: the guide pass at a per-pixel count plane.  Pixel p casts the primary rays 0 .. n_p - 1, n_p its
clamped value of the plane, so every pixel with n_p >= 1 is pinned bit for bit against the sibling cr_render_aov_* call at
samples = n_p (itself pinned against the oracle's probes in tests/test_gpu_aov.py), pixels without samples against +0.0 and
+inf, the counters against the sibling region calls over rectangles of constant count, and a frame at a scale below 2^52
against the Python model of tests/test_gpu_aov.py.  Values are compared as bytes."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as M
import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer
from test_gpu_adaptive import SEED, median_tolerance, pass_words, sized   # (pass_words renders with that module's seed)
from test_gpu_aov import finalize, model

pytestmark = pytest.mark.gpu

REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
IDS = [t for _, t in REALS]
NAMES = [n for n, _, _ in A.AOV_LAYERS]
INT_STATS = ("samples", "segments", "node_tests", "prim_tests", "texel_fetches", "nan_pixels", "bvh_entries", "scene_in_lds")
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
W, H = 37, 23   # no multiple of the 4 x 4 tile
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def np_real(rt):
    return np.float64 if rt == A.CR_REAL_F64 else np.float32


def at_samples(cam, n, call):
    """call() with cam.samples = n"""
    keep = cam.samples
    cam.set_samples(n)
    try:
        return call()
    finally:
        cam.set_samples(keep)


def mixed_plane(shape, seed=7, values=(0, 1, 2, 3, 5, 8)):
    """A seeded plane whose counts differ from pixel to pixel, so inside every tile"""
    rng = np.random.default_rng(seed)
    plane = rng.choice(np.array(values, dtype=np.int32), size=shape).astype(np.int32)
    assert set(np.unique(plane)) == set(values)
    return plane


def same_bytes(got, want, mask, what):
    for n in NAMES:
        if n in got:
            assert got[n].dtype == want[n].dtype, (what, n)
            assert got[n][mask].tobytes() == want[n][mask].tobytes(), (what, n, int(mask.sum()))


def check_empty_pixels(got, mask, R):
    """n_p == 0: +0.0 (all bits clear) in albedo, normal and coverage, +inf depth"""
    for n in ("albedo", "normal", "coverage"):
        if n in got:
            assert got[n].dtype == R and not np.frombuffer(got[n][mask].tobytes(), dtype=np.uint8).any(), n
    if "depth" in got:
        assert got["depth"].dtype == R and np.isposinf(got["depth"][mask]).all()


def check_per_count(r, cam, plane, rt, sibling=None, counts_call=None, what=""):
    """The counts call over `plane` against the sibling call at every count the clamped plane holds.  Returns (planes, stats)."""
    sibling = sibling or (lambda: r.render_aov(cam, seed=SEED, real_type=rt))
    got, st = counts_call() if counts_call else r.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    assert sorted(got) == sorted(NAMES)
    n_p = np.clip(plane.astype(np.int64), 0, cam.samples)
    for c in np.unique(n_p):
        if c == 0:
            check_empty_pixels(got, n_p == 0, np_real(rt))
            continue
        want, _ = at_samples(cam, int(c), sibling)
        same_bytes(got, want, n_p == c, f"{what} count {c}")
    assert st["samples"] == st["segments"] == int(n_p.sum())
    assert st["nan_pixels"] == 0 and st["kernel_ms"] > 0
    return got, st


def few(samples=8, w=W, h=H):
    return sized(scenes.few_spheres(20), w, h, samples)


# ---- 1. uniform planes
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_uniform_planes(renderer, rt, tag, c):
    sc = few(c)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    want, wst = renderer.render_aov(cam, seed=SEED, real_type=rt)
    plane = np.full((H, W), c, dtype=np.int32)
    got, st = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    same_bytes(got, want, np.ones((H, W), dtype=bool), f"samples {c}")
    for k in INT_STATS:
        assert st[k] == wst[k], (k, st[k], wst[k])
    cam.set_samples(8)   # the same plane under a larger maximum: the same bytes
    got8, st8 = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    same_bytes(got8, want, np.ones((H, W), dtype=bool), f"samples 8, plane {c}")
    for k in INT_STATS:
        assert st8[k] == wst[k], (k, st8[k], wst[k])


# ---- 2. counts that differ inside a tile
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_counts_differ_inside_a_tile(renderer, rt, tag):
    sc = few(8)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((H, W))
    _, st = check_per_count(renderer, cam, plane, rt)
    assert st["samples"] == int(plane.sum())
    # all zero but one pixel with the maximum, in the last lane position an edge tile has inside the image: the tile at
    # (32, 20) is cut by the bottom edge (rows 20..22), its last pixel is (35, 22); the corner tile at (36, 20) is cut by
    # both edges, its last pixel is (36, 22)
    assert (W, H) == (37, 23)
    for x, y in ((35, 22), (36, 22)):
        one = np.zeros((H, W), dtype=np.int32)
        one[y, x] = 8
        got, st = check_per_count(renderer, cam, one, rt, what=f"one pixel ({x}, {y})")
        assert st["samples"] == 8 and np.isfinite(got["albedo"][y, x]).all()
    # an all-zero plane: the kernel launches and does nothing
    got, st = renderer.render_aov_counts(cam, np.zeros((H, W), dtype=np.int32), seed=SEED, real_type=rt)
    check_empty_pixels(got, np.ones((H, W), dtype=bool), np_real(rt))
    assert all(st[k] == 0 for k in ("samples",) + COUNTERS)


# ---- 3. counters over rectangles of constant count
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_counters_add_up_over_rectangles(renderer, rt, tag):
    sc = sized(scenes.mixed_scene(), W, H, 8)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    rects = [((0, 0, 13, 9), 5), ((13, 0, W - 13, 9), 2), ((0, 9, 13, H - 9), 0), ((13, 9, W - 13, H - 9), 3)]
    plane = np.zeros((H, W), dtype=np.int32)
    tot = {k: 0 for k in COUNTERS}
    for (x0, y0, w, h), c in rects:
        plane[y0:y0 + h, x0:x0 + w] = c
        if c:
            _, rst = at_samples(cam, c, lambda: renderer.render_aov_region(cam, (x0, y0, w, h), seed=SEED, real_type=rt))
            for k in COUNTERS:
                tot[k] += rst[k]
    _, st = check_per_count(renderer, cam, plane, rt)
    for k in COUNTERS:
        assert st[k] == tot[k], (k, st[k], tot[k])
    assert tot["texel_fetches"] > 0


# ---- 4. a scale below 2^52, against the Python model over the oracle's probes
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_scale_below_2_52_against_the_model(renderer, oracles, rt, tag):
    w, h = 13, 7
    sc = sized(scenes.mixed_scene(), w, h, 4096)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((h, w), seed=11, values=(0, 1, 3, 6))
    R = np_real(rt)
    words = {int(c): model(oracles[rt], sc, SEED, sample_begin=0, sample_count=int(c))[1] for c in np.unique(plane) if c}
    sums, flags, depth = [[0] * 7 for _ in range(w * h)], [0] * (w * h), np.full(w * h, np.inf, dtype=R)
    for k, c in enumerate(plane.reshape(-1).tolist()):
        if c:
            sums[k], flags[k], depth[k] = words[c][0][k], words[c][1][k], words[c][2][k]
    for output_sum in (0, 1):
        # finalize's f64 sums at the scale of 4096 (output_sum 1 in f64 is the word times 2^-S, exactly), then the divisor n_p
        want = finalize((sums, flags, depth), cam, np.float64, 1)
        if not output_sum:
            div = np.where(plane > 0, plane, 1).astype(np.float64)
            for n in ("albedo", "normal", "coverage"):
                want[n] = want[n] / (div[..., None] if want[n].ndim == 3 else div)
        want = {n: np.ascontiguousarray(v, dtype=R) for n, v in want.items()}
        got, st = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt, output_sum=output_sum)
        same_bytes(got, want, np.ones((h, w), dtype=bool), f"output_sum {output_sum}")
        assert st["samples"] == int(plane.sum())


# ---- 5. the clamp
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_clamp(renderer, rt, tag):
    sc = few(5)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((H, W), seed=3, values=(-5, I32_MIN, 6, I32_MAX, 2))
    clamped = np.clip(plane.astype(np.int64), 0, 5).astype(np.int32)
    assert set(np.unique(clamped)) == {0, 2, 5}
    got, st = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    want, wst = renderer.render_aov_counts(cam, clamped, seed=SEED, real_type=rt)
    same_bytes(got, want, np.ones((H, W), dtype=bool), "clamp")
    for k in INT_STATS:
        assert st[k] == wst[k], k
    check_per_count(renderer, cam, plane, rt)


# ---- 6. every walk
def teapot():
    from crucible_amd.demo_builder import procedural_sky, teapot_orbit_movie
    return teapot_orbit_movie(1, image_width=48, samples=8, sky=procedural_sky(64, 32))


def with_mode(sc, mode):
    sc.bvh_mode = mode
    return sc


WALKS = {
    "moving": lambda: sized(scenes.moving_scene(frame=2), 24, 16, 8),
    "scaled": lambda: sized(scenes.scaled_scene(frame=1), 24, 16, 8),
    "mixed": lambda: sized(scenes.mixed_scene(), 24, 16, 8),
    "mixed_keyed_camera": lambda: sized(scenes.mixed_scene(sky=False, animate=True), 24, 16, 8),
    "lists": lambda: sized(scenes.list_scene(), 24, 16, 8),
    "wrapped": lambda: sized(scenes.wrapped_scene(), 24, 16, 8),
    "teapot": teapot,
    "sah": lambda: with_mode(sized(scenes.mixed_scene(), 24, 16, 8), A.CR_BVH_SAH),
    "sah_ordered": lambda: with_mode(sized(scenes.mixed_scene(), 24, 16, 8), A.CR_BVH_SAH_ORDERED),
    "lbvh": lambda: with_mode(sized(scenes.mixed_scene(), 24, 16, 8), A.CR_BVH_LBVH),
    "sah_device": lambda: with_mode(sized(scenes.mixed_scene(), 24, 16, 8), A.CR_BVH_SAH | A.CR_BVH_BUILD_DEVICE),
}


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
@pytest.mark.parametrize("walk", list(WALKS))
def test_every_walk(renderer, rt, tag, walk):
    sc = WALKS[walk]()
    cam = sc.scene_cam
    assert cam.samples == 8
    renderer.upload_scene(sc.flatten())
    _, st = check_per_count(renderer, cam, mixed_plane((cam.image_height, cam.image_width), seed=5, values=(0, 1, 3, 6, 8)), rt, what=walk)
    if walk == "teapot":
        assert st["scene_in_lds"] == 2 and (cam.image_width, cam.image_height) == (48, 27)


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_global_memory_handle(hiplib, monkeypatch, rt, tag):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        sc = sized(scenes.mixed_scene(), 24, 16, 8)
        r.upload_scene(sc.flatten())
        _, st = check_per_count(r, sc.scene_cam, mixed_plane((16, 24), seed=5, values=(0, 1, 3, 6, 8)), rt)
        assert st["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
@pytest.mark.parametrize("refit", [True, "rebuild"], ids=["refit", "rebuild"])
def test_refit_as_the_sibling_handles_it(renderer, rt, tag, refit):
    sc = with_mode(sized(scenes.moving_scene(frame=1), 24, 16, 8), A.CR_BVH_SAH)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((16, 24), seed=5, values=(0, 1, 3, 6, 8))
    plain, _ = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    cam.refit_boxes = refit
    try:
        got, _ = check_per_count(renderer, cam, plane, rt, what=str(refit))
    finally:
        cam.refit_boxes = False
    again, _ = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)   # not sticky
    same_bytes(again, plain, np.ones((16, 24), dtype=bool), "after refit")


# ---- 7. masks and the device form
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_every_layer_mask_and_the_device_form(renderer, rt, tag):
    import torch
    sc = sized(scenes.mixed_scene(), 24, 16, 8)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((16, 24), seed=9)
    everything = np.ones((16, 24), dtype=bool)
    full, fst = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    for mask in range(1, 16):
        got, _ = renderer.render_aov_counts(cam, plane, mask, seed=SEED, real_type=rt)
        assert sorted(got) == sorted(n for n, bit, _ in A.AOV_LAYERS if mask & bit)
        same_bytes(got, full, everything, f"mask {mask}")
    n = 24 * 16
    d_plane = torch.from_numpy(plane).to("cuda:0")
    buf = torch.full((n * 8,), -7.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    assert renderer.render_aov_counts_device(cam, d_plane.data_ptr(), buf.data_ptr(), seed=SEED, real_type=rt) is None
    renderer.synchronize()
    want = np.concatenate([full[name].reshape(-1) for name in NAMES])
    assert buf.cpu().numpy().tobytes() == want.tobytes()
    st = renderer.render_aov_counts_device(cam, d_plane.data_ptr(), buf.data_ptr(), A.CR_AOV_DEPTH, seed=SEED, real_type=rt, want_stats=True)
    assert st["samples"] == int(plane.sum()) and all(st[k] == fst[k] for k in ("segments", "node_tests", "prim_tests"))   # (no albedo: no texels)
    assert buf.cpu().numpy()[:n].tobytes() == full["depth"].tobytes()
    # the region's and the batch's device forms
    reg = (5, 3, 13, 9)
    crop = np.ascontiguousarray(plane[3:12, 5:18])
    d_crop = torch.from_numpy(crop).to("cuda:0")
    rwant, _ = renderer.render_aov_counts_region(cam, reg, crop, seed=SEED, real_type=rt)
    renderer.render_aov_counts_region_device(cam, reg, d_crop.data_ptr(), buf.data_ptr(), seed=SEED, real_type=rt)
    renderer.synchronize()
    assert buf.cpu().numpy()[:13 * 9 * 8].tobytes() == np.concatenate([rwant[name].reshape(-1) for name in NAMES]).tobytes()
    planes2 = np.stack([plane, plane[::-1]])
    d_planes2 = torch.from_numpy(np.ascontiguousarray(planes2)).to("cuda:0")
    buf2 = torch.zeros((2 * n * 8,), dtype=buf.dtype, device="cuda:0")
    fwant, _ = renderer.render_aov_counts_frames(cam, [0, 1], planes2, seed=SEED, real_type=rt)
    renderer.render_aov_counts_frames_device(cam, [0, 1], d_planes2.data_ptr(), buf2.data_ptr(), seed=SEED, real_type=rt)
    renderer.synchronize()
    assert buf2.cpu().numpy().tobytes() == np.concatenate([f[name].reshape(-1) for f in fwant for name in NAMES]).tobytes()


# ---- 8. frames
def frames_equal_singles(single, cam, frames, planes, rt, batch=None):
    batch = batch or single
    got, st = batch.render_aov_counts_frames(cam, frames, planes, seed=SEED, real_type=rt)
    assert len(got) == len(frames)
    tot = {k: 0 for k in ("samples",) + COUNTERS}
    keep = cam.frame
    try:
        for k, f in enumerate(frames):
            cam.frame = f
            want, wst = single.render_aov_counts(cam, planes[k], seed=SEED, real_type=rt)
            same_bytes(got[k], want, np.ones(planes[k].shape, dtype=bool), f"entry {k} (frame {f})")
            for c in tot:
                tot[c] += wst[c]
    finally:
        cam.frame = keep
    for c in tot:
        assert st[c] == tot[c], (c, st[c], tot[c])
    assert st["samples"] == int(np.clip(planes, 0, cam.samples).sum())
    return got


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_frames(hiplib, renderer, monkeypatch, rt, tag):
    sc = sized(scenes.moving_scene(frame=0), W, H, 8)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    f = 1
    frames = [f, f + 2, f, f + 1]
    planes = np.stack([mixed_plane((H, W), seed=20 + k) for k in range(4)])
    got = frames_equal_singles(renderer, cam, frames, planes, rt)
    assert got[0]["coverage"].tobytes() != got[2]["coverage"].tobytes()   # one frame, two planes
    # several launches of whole frames: 60 tiles of 2 sample groups
    monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", "250")   # read by cr_create
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        frames_equal_singles(renderer, cam, frames, planes, rt, batch=r)
    finally:
        r.close()


def test_a_frames_call_that_would_refit_is_refused(renderer):
    rt = A.CR_REAL_F32
    sc = with_mode(sized(scenes.moving_scene(frame=0), 24, 16, 8), A.CR_BVH_SAH)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    planes = np.stack([mixed_plane((16, 24), seed=1), mixed_plane((16, 24), seed=2)])
    before, _ = renderer.render_aov_counts_frames(cam, [0, 1], planes, seed=SEED, real_type=rt)
    for refit in (True, "rebuild"):
        cam.refit_boxes = refit
        try:
            with pytest.raises(CrucibleError) as e:
                renderer.render_aov_counts_frames(cam, [0, 1], planes, seed=SEED, real_type=rt)
        finally:
            cam.refit_boxes = False
        assert e.value.code == A.CR_ERR_UNSUPPORTED and "cr_render_frames cannot refit boxes" in str(e.value)
        after, _ = renderer.render_aov_counts_frames(cam, [0, 1], planes, seed=SEED, real_type=rt)
        for k in range(2):
            same_bytes(after[k], before[k], np.ones((16, 24), dtype=bool), f"after {refit}")


# ---- 9. region
@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_region(renderer, rt, tag):
    sc = sized(scenes.mixed_scene(animate=True), W, H, 8)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((H, W), seed=13)
    frame, fst = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    x0, y0, w, h = 5, 3, 13, 9
    crop = np.ascontiguousarray(plane[y0:y0 + h, x0:x0 + w])
    got, st = renderer.render_aov_counts_region(cam, (x0, y0, w, h), crop, seed=SEED, real_type=rt)
    same_bytes(got, {n: np.ascontiguousarray(frame[n][y0:y0 + h, x0:x0 + w]) for n in NAMES}, np.ones((h, w), dtype=bool), "crop")
    assert st["samples"] == st["segments"] == int(crop.sum())
    whole, wst = renderer.render_aov_counts_region(cam, (0, 0, W, H), plane, seed=SEED, real_type=rt)
    same_bytes(whole, frame, np.ones((H, W), dtype=bool), "whole frame")
    for k in INT_STATS:
        assert wst[k] == fst[k], k


# ---- 10. end to end: the guide layers of an adaptive frame
def adaptive_setup(r, rt):
    """tests/test_gpu_adaptive.py's mixed-decision configuration: (scene, pass, minimum, block, tolerance)"""
    sc, P, min_samples, block = sized(scenes.mixed_scene(), 47, 37, 16), 2, 8, 8
    r.upload_scene(sc.flatten())
    words = pass_words(r, sc.scene_cam, rt, P)
    tol = median_tolerance(words, P, min_samples, 16, block)
    want_counts, _, _ = M.adaptive(words, P, min_samples, 16, block, tol, np_real(rt))
    assert len(np.unique(want_counts)) >= 3 and (want_counts == 16).any() and (want_counts == min_samples).any(), np.unique(want_counts)
    return sc, dict(tolerance=tol, min_samples=min_samples, pass_samples=P, block=block, sum_order=A.CR_SUM_RELAXED), want_counts


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_guide_layers_of_an_adaptive_frame(renderer, rt, tag):
    sc, ad, want_counts = adaptive_setup(renderer, rt)
    cam = sc.scene_cam
    _, counts, ast = renderer.render_adaptive(cam, seed=SEED, real_type=rt, **ad)
    assert np.array_equal(counts, want_counts)
    _, st = check_per_count(renderer, cam, counts, rt)
    assert st["samples"] == ast["render"]["samples"]
    # a region whose origin is no multiple of the block: its own blocks, its own counts
    reg = (5, 3, 29, 21)
    _, rcounts, _ = renderer.render_adaptive_region(cam, reg, seed=SEED, real_type=rt, **ad)
    assert len(np.unique(rcounts)) >= 2, np.unique(rcounts)
    check_per_count(renderer, cam, rcounts, rt, sibling=lambda: renderer.render_aov_region(cam, reg, seed=SEED, real_type=rt),
                    counts_call=lambda: renderer.render_aov_counts_region(cam, reg, rcounts, seed=SEED, real_type=rt), what="region")


@pytest.mark.parametrize("rt,tag", REALS, ids=IDS)
def test_guide_layers_of_adaptive_frames(renderer, rt, tag):
    sc, P, min_samples, block = sized(scenes.moving_scene(frame=1), 37, 29, 24), 3, 6, 16
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    tol = median_tolerance(pass_words(renderer, cam, rt, P), P, min_samples, 24, block)
    frames = [0, 1, 2]
    _, counts, _ = renderer.render_adaptive_frames(cam, frames, seed=SEED, real_type=rt, tolerance=tol, min_samples=min_samples, pass_samples=P,
                                                   block=block, sum_order=A.CR_SUM_RELAXED)
    assert len(np.unique(counts)) >= 2, np.unique(counts)
    got, st = renderer.render_aov_counts_frames(cam, frames, counts, seed=SEED, real_type=rt)
    assert st["samples"] == int(counts.sum())
    keep = cam.frame
    try:
        for k, f in enumerate(frames):
            cam.frame = f
            for n in np.unique(counts[k]):
                want, _ = at_samples(cam, int(n), lambda: renderer.render_aov(cam, seed=SEED, real_type=rt))
                same_bytes(got[k], want, counts[k] == n, f"frame {f} count {n}")
    finally:
        cam.frame = keep


# ---- 11. refusals
def test_refusals_leave_the_handle_alone(renderer):
    rt = A.CR_REAL_F32
    sc = few(8, 24, 16)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((16, 24), seed=4)
    before, _ = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    everything = np.ones((16, 24), dtype=bool)

    def refused(code, text, call):
        with pytest.raises(CrucibleError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
        after, _ = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
        same_bytes(after, before, everything, text)

    one = lambda **kw: renderer.render_aov_counts(cam, kw.pop("counts", plane), kw.pop("layers", A.CR_AOV_ALL), seed=SEED, real_type=rt, **kw)
    crop = np.ascontiguousarray(plane[:9, :13])
    refused(A.CR_ERR_INVALID_ARG, "counts is null", lambda: one(counts=None))
    refused(A.CR_ERR_INVALID_ARG, "counts is null", lambda: renderer.render_aov_counts_frames(cam, [0, 1], None, seed=SEED, real_type=rt))
    refused(A.CR_ERR_INVALID_ARG, "counts is null", lambda: renderer.render_aov_counts_region(cam, (0, 0, 13, 9), None, seed=SEED, real_type=rt))
    refused(A.CR_ERR_UNSUPPORTED, "from sample 0", lambda: one(sample_begin=1, sample_count=7))
    refused(A.CR_ERR_UNSUPPORTED, "from sample 0", lambda: one(sample_begin=0, sample_count=7))
    refused(A.CR_ERR_UNSUPPORTED, "fixed-point", lambda: one(output_sum=A.CR_OUTPUT_FIXED_SUM))
    # the order of the checks: the sibling's own first, then the plane, then the shard
    refused(A.CR_ERR_UNSUPPORTED, "fixed-point", lambda: one(counts=None, output_sum=A.CR_OUTPUT_FIXED_SUM))
    refused(A.CR_ERR_INVALID_ARG, "counts is null", lambda: one(counts=None, sample_begin=1, sample_count=7))
    for layers in (0, 16, -1):
        refused(A.CR_ERR_INVALID_ARG, "layers must be", lambda: one(layers=layers))
    refused(A.CR_ERR_INVALID_ARG, "layers must be", lambda: one(layers=0, counts=None))
    refused(A.CR_ERR_INVALID_ARG, "region reaches outside", lambda: renderer.render_aov_counts_region(cam, (20, 0, 13, 9), crop, seed=SEED, real_type=rt))
    refused(A.CR_ERR_INVALID_ARG, "region is null", lambda: renderer.render_aov_counts_region(cam, None, np.zeros((1, 1), dtype=np.int32), seed=SEED,
                                                                                             real_type=rt))
    refused(A.CR_ERR_INVALID_ARG, "frames is null", lambda: renderer.render_aov_counts_frames(cam, None, plane[None], seed=SEED, real_type=rt))
    # a null output, through each form
    cd, p = cam.desc(), cam.params(SEED, rt, 0, None, 0, A.CR_SUM_DEFAULT)
    lib, h = renderer.lib, renderer.h
    ptr = plane.ctypes.data_as(C.c_void_p)
    fr = (C.c_int32 * 1)(0)
    reg = A.CrRegion(0, 0, 13, 9)
    for rc in (lib.cr_render_aov_counts_host(h, C.byref(cd), C.byref(p), 15, ptr, None, None),
               lib.cr_render_aov_counts_device(h, C.byref(cd), C.byref(p), 15, ptr, None, None),
               lib.cr_render_aov_counts_frames_host(h, C.byref(cd), C.byref(p), 15, fr, 1, ptr, None, None),
               lib.cr_render_aov_counts_frames_device(h, C.byref(cd), C.byref(p), 15, fr, 1, ptr, None, None),
               lib.cr_render_aov_counts_region_host(h, C.byref(cd), C.byref(p), 15, C.byref(reg), ptr, None, None),
               lib.cr_render_aov_counts_region_device(h, C.byref(cd), C.byref(p), 15, C.byref(reg), ptr, None, None)):
        assert rc == A.CR_ERR_INVALID_ARG and b"output buffer is null" in lib.cr_last_error(h)
    after, _ = renderer.render_aov_counts(cam, plane, seed=SEED, real_type=rt)
    same_bytes(after, before, everything, "null output")


# ---- 12. settings
@pytest.mark.parametrize("setting", ["CRUCIBLE_PIPELINE=mega", "CRUCIBLE_PIPELINE=wavefront", "CRUCIBLE_PIPELINE=queue", "CRUCIBLE_SUM_ORDER=reference",
                                     "CRUCIBLE_SUM_ORDER=relaxed"])
def test_settings_do_not_reach_the_planes(hiplib, renderer, monkeypatch, setting):
    sc = sized(scenes.mixed_scene(), 24, 16, 8)
    renderer.upload_scene(sc.flatten())
    plane = mixed_plane((16, 24), seed=6)
    want, wst = renderer.render_aov_counts(sc.scene_cam, plane, seed=SEED, real_type=A.CR_REAL_F64)
    monkeypatch.setenv(*setting.split("="))
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        for sum_order in (A.CR_SUM_DEFAULT, A.CR_SUM_RELAXED, A.CR_SUM_REFERENCE_ORDER):
            got, st = r.render_aov_counts(sc.scene_cam, plane, seed=SEED, real_type=A.CR_REAL_F64, sum_order=sum_order)
            same_bytes(got, want, np.ones((16, 24), dtype=bool), setting)
            assert all(st[k] == wst[k] for k in INT_STATS)
    finally:
        r.close()
