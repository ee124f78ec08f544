"""cr_render_aov_*: the first-hit guide layers (albedo, normal, depth, coverage) pinned bit for bit against a model in plain
Python over the oracle's probes.

The model, per pixel and sample: oracle_camera_ray (the beauty render's primary ray), oracle_world_hit with tmin 0.001,
tmax inf and the ray's time, then oracle_texture_value / the material table of scene.flatten() on a hit or oracle_sky on
a miss.  The normal's encoding and the depth are formed in numpy scalars of the render's dtype; the sums are Python
integers of rint(x * 2^S); the finalize is restated from the library's (the word's magnitude in two exact halves, times
2^-S, divided by the frame's sample count unless the shard's sum is asked for, the sign put back).  Every plane is
compared with tobytes()."""
import ctypes as C
import os

import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer
from scenes import few_spheres, list_scene, mixed_scene, moving_scene, scaled_scene, wrapped_scene

pytestmark = pytest.mark.gpu

SEED = 0xA0B1
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
NAMES = [n for n, _, _ in A.AOV_LAYERS]


def resize(scene, w, h, samples=None):
    cam = scene.scene_cam
    cam.image_width, cam.image_height = w, h
    if samples is not None:
        cam.set_samples(samples)
    return scene


def fx_log2(samples):   # fx_scale_for
    lg = samples.bit_length() - 1
    return min(52, 62 - lg)


def model_words(oracle, scene_h, flat, cam, seed, sample_begin=0, sample_count=None, tmin=0.001):
    """Per pixel: the 7 integer sums (albedo, encoded normal, coverage), the flagged channels and the minimum depth.
    tmin: where the hit interval starts -- the pass's 0.001, or another value for a test that shows a scene depends on it."""
    R = oracle.np_real
    L = oracle.lib
    cd = cam.desc()
    p = cam.params(seed, oracle.real_type, sample_begin, sample_count, 0, A.CR_SUM_DEFAULT)
    W, H = cam.image_width, cam.image_height
    S = fx_log2(cam.samples)
    sums = [[0] * 7 for _ in range(W * H)]
    flags = [0] * (W * H)
    depth = np.full(W * H, np.inf, dtype=R)
    ray, rec, col = np.zeros(8, dtype=R), np.zeros(10, dtype=R), np.zeros(3, dtype=R)
    orig, dirn, loc = np.zeros(3, dtype=R), np.zeros(3, dtype=R), np.zeros(3, dtype=R)
    mat = C.c_int32()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    half = R(0.5)
    for j in range(H):
        for i in range(W):
            for s in range(p.sample_begin, p.sample_begin + p.sample_count):
                L.oracle_camera_ray(C.byref(cd), C.byref(p), i, j, s, ptr(ray))
                orig[:] = ray[0:3]
                dirn[:] = ray[3:6]
                hit = L.oracle_world_hit(scene_h, ptr(orig), ptr(dirn), oracle.real(ray[6]), oracle.real(tmin),
                                         oracle.real(np.inf), ptr(rec), C.byref(mat))
                if hit:
                    m = flat.materials[mat.value]
                    if m.kind == A.CR_MAT_LAMBERTIAN:
                        loc[:] = rec[1:4]
                        L.oracle_texture_value(scene_h, m.texture, oracle.real(rec[7]), oracle.real(rec[8]), ptr(loc), ptr(col))
                        alb = [col[0], col[1], col[2]]
                    elif m.kind == A.CR_MAT_METAL:
                        alb = [R(m.albedo[0]), R(m.albedo[1]), R(m.albedo[2])]
                    else:
                        alb = [R(1), R(1), R(1)]
                    n = [rec[4], rec[5], rec[6]]
                    d = [rec[1 + k] + (-orig[k]) for k in range(3)]
                    dep = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                    assert dep.dtype == R
                    if dep < np.inf:
                        depth[j * W + i] = min(depth[j * W + i], dep)
                else:
                    L.oracle_sky(scene_h, ptr(dirn), ptr(col))
                    alb = [col[0], col[1], col[2]]
                    n = [R(0), R(0), R(0)]
                vals = alb + [half * c + half for c in n] + [R(1) if hit else R(0)]
                for c, x in enumerate(vals):
                    assert x.dtype == R
                    y = float(x) * 2.0 ** S
                    if not np.isfinite(y) or abs(round(y)) >= 2 ** 62:
                        flags[j * W + i] |= 1 << c
                    else:
                        sums[j * W + i][c] += round(y)   # half to even, as rint
    return sums, flags, depth


def finalize(words, cam, R, output_sum):
    """The planes of model_words' sums, as the library's finalize kernel forms them."""
    sums, flags, depth = words
    W, H = cam.image_width, cam.image_height
    S = fx_log2(cam.samples)
    out = np.zeros((W * H, 7), dtype=R)
    for k in range(W * H):
        for c in range(7):
            v = sums[k][c]
            mag = abs(v)
            s = (float(mag >> 32) * 4294967296.0 + float(mag & 0xFFFFFFFF)) * 2.0 ** -S
            if not output_sum:
                s = s / float(cam.samples)
            if v < 0:
                s = -s
            if (flags[k] >> c) & 1:
                s = float("nan")
            out[k, c] = R(s)
    return {"albedo": np.ascontiguousarray(out[:, 0:3]).reshape(H, W, 3), "normal": np.ascontiguousarray(out[:, 3:6]).reshape(H, W, 3),
            "depth": depth.reshape(H, W), "coverage": np.ascontiguousarray(out[:, 6]).reshape(H, W)}


def model(oracle, scene, seed, tree=None, sample_begin=0, sample_count=None, output_sum=0, linear_list=False, tmin=0.001):
    """linear_list: the probes walk no tree at all (Oracle.render_image's switch), for an exported tree without wrappers."""
    flat = scene.flatten()
    cam = scene.scene_cam
    h = oracle.scene_create(flat)
    try:
        if tree is not None:
            oracle.set_tree(h, *tree)
        if linear_list:
            oracle.lib.oracle_use_list(h)
        # oracle_render leaves the boxes of its frame in the scene it rendered (scene_prepare_boxes: the refitted ones
        # with refit_boxes, else the construction-time ones): a one-pixel render primes the scene for the probes
        oracle.render(h, cam, seed=seed, pix_begin=0, pix_end=1, n_threads=1)
        words = model_words(oracle, h, flat, cam, seed, sample_begin, sample_count, tmin)
    finally:
        oracle.scene_destroy(h)
    return finalize(words, cam, oracle.np_real, output_sum), words


def same(got, want, what=""):
    for n in want:
        if n in got:
            assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
            if got[n].tobytes() != want[n].tobytes():
                bad = np.argwhere(~((got[n] == want[n]) | (np.isnan(got[n]) & np.isnan(want[n]))))
                raise AssertionError(f"{what} {n}: {len(bad)} values differ, first at {bad[0]}: {got[n][tuple(bad[0])]!r} != {want[n][tuple(bad[0])]!r}")


def check_counters(r, scene, rt, st):
    """segments, node_tests, prim_tests (and the texels read) of a depth-1 render of the same primary rays"""
    cam = scene.scene_cam
    depth = cam.max_depth
    cam.set_max_depth(1)
    try:
        _, rst = r.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_REFERENCE_ORDER)
    finally:
        cam.set_max_depth(depth)
    assert st["samples"] == cam.image_width * cam.image_height * cam.samples and st["segments"] == st["samples"]
    for k in ("segments", "node_tests", "prim_tests", "texel_fetches", "bvh_entries", "scene_in_lds"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["nan_pixels"] == 0 and st["kernel_ms"] > 0


def parity(r, oracles, scene, rt, tree_of_device=False, counters=True):
    r.upload_scene(scene.flatten())
    got, st = r.render_aov(scene.scene_cam, seed=SEED, real_type=rt)
    assert sorted(got) == sorted(NAMES)
    tree = r.export_bvh(rt) if tree_of_device else None
    want, _ = model(oracles[rt], scene, SEED, tree=tree)
    same(got, want)
    if counters:
        check_counters(r, scene, rt, st)
    return got, st


# ---- scenes: tile alignment (37 x 23 is no multiple of the 4 x 4 tile, 1..5 samples no multiple of the group of 4),
# residency and kernel kind
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("samples", [1, 2, 3, 5])
def test_few_spheres_odd_sizes(renderer, oracles, rt, tag, samples):
    _, st = parity(renderer, oracles, resize(few_spheres(20), 37, 23, samples), rt)
    assert st["scene_in_lds"] == 1


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_mixed_scene_with_sky_and_defocus(renderer, oracles, rt, tag):
    sc = resize(mixed_scene(), 24, 16, 3)
    assert sc.scene_cam.defocus_angle_degrees > 0
    got, st = parity(renderer, oracles, sc, rt)
    assert st["texel_fetches"] > 0 and 0 < got["coverage"].mean() < 1
    assert np.isinf(got["depth"]).any() and np.isfinite(got["depth"]).any()


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_mixed_scene_default_sky_keyed_camera(renderer, oracles, rt, tag):
    parity(renderer, oracles, resize(mixed_scene(sky=False, animate=True), 24, 16, 3), rt)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("frame", [0, 2])
@pytest.mark.parametrize("maker", [moving_scene, scaled_scene], ids=["moving", "scaled"])
def test_keyed_primitives(renderer, oracles, rt, tag, frame, maker):
    parity(renderer, oracles, resize(maker(frame=frame), 24, 16, 3), rt)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("maker", [list_scene, wrapped_scene], ids=["lists", "wrapped"])
def test_list_and_wrapper_elements(renderer, oracles, rt, tag, maker):
    parity(renderer, oracles, resize(maker(), 24, 16, 3), rt)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_teapot_top_window_keyed_camera(renderer, oracles, rt, tag):
    from crucible_amd.demo_builder import procedural_sky, teapot_orbit_movie
    sc = teapot_orbit_movie(1, image_width=48, samples=3, sky=procedural_sky(64, 32))
    _, st = parity(renderer, oracles, sc, rt)
    assert st["scene_in_lds"] == 2


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_global_memory_handle(hiplib, oracles, monkeypatch, rt, tag):
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        _, st = parity(r, oracles, resize(mixed_scene(), 24, 16, 3), rt)
        assert st["scene_in_lds"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH], ids=["sah", "sah_ordered", "lbvh"])
def test_opt_in_trees(renderer, oracles, rt, tag, mode):
    sc = resize(mixed_scene(), 24, 16, 3)
    sc.bvh_mode = mode
    parity(renderer, oracles, sc, rt, tree_of_device=True)


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_the_interval_starts_at_0_001(renderer, oracles, rt, tag):
    """A small sphere around the camera: a primary ray meets it at t = radius / |direction|, and |direction| grows from
    the focus distance (10) at the image centre to about 10.9 in the corners, so with radius 0.0105 t crosses 0.001
    inside the image -- hits at the centre, the scene behind it towards the corners."""
    from crucible_amd.scene import Metal, Sphere
    sc = resize(few_spheres(3), 37, 23, 2)
    sc.add_element(Sphere.new((0.0, 1.0, 6.0), 0.0105, Metal.new((0.5, 0.6, 0.7), 0.0)), "shell")
    got, _ = parity(renderer, oracles, sc, rt)
    assert (got["depth"] < 0.02).any() and (got["depth"] > 1.0).any()


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_the_guide_pass_stages_what_the_render_stages(hiplib, monkeypatch, rt, tag):
    """The render's ladder and the guide pass's ask one rule (crucible_amd/csrc/residency.hpp): on a handle of each
    residency -- the whole scene in LDS, a 1 KB window with and without the side tables, global memory, no screening
    records -- the guide pass reports the render's scene_in_lds, and its planes are the default handle's bit for bit."""
    from test_gpu_variants import GLOBAL, IN_LDS, NO_SCREEN, RES_GLOBAL, RES_LDS, RES_TOP, WINDOW, matrix_scene
    sc = matrix_scene("static")
    cam = sc.scene_cam
    assert (cam.image_width, cam.image_height, cam.samples) == (24, 16, 3)
    envs = [("default", {}, RES_LDS), ("window", WINDOW, RES_TOP), ("global", GLOBAL, RES_GLOBAL),
            ("window, side tables in global memory", dict(WINDOW, CRUCIBLE_LDS_SIDE_KB="0"), RES_TOP), ("no screen", NO_SCREEN, RES_LDS)]
    want = None
    for name, env, res in envs:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            r = Renderer(0)   # the knobs are read in cr_create
        try:
            r.upload_scene(sc.flatten())
            _, rst = r.render(cam, seed=SEED, real_type=rt)
            got, st = r.render_aov(cam, seed=SEED, real_type=rt)
        finally:
            r.close()
        assert st["scene_in_lds"] == rst["scene_in_lds"] == IN_LDS[res], (name, st["scene_in_lds"], rst["scene_in_lds"])
        assert sorted(got) == sorted(NAMES)
        if want is None:
            want = got
        same(got, want, name)


# ---- layers and shards
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_every_layer_mask_and_the_device_form(renderer, rt, tag):
    import torch
    sc = resize(mixed_scene(), 24, 16, 3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    full, _ = renderer.render_aov(cam, seed=SEED, real_type=rt)
    for mask in range(1, 16):
        got, _ = renderer.render_aov(cam, mask, seed=SEED, real_type=rt)
        assert sorted(got) == sorted(n for n, bit, _ in A.AOV_LAYERS if mask & bit)
        same(got, full, f"mask {mask}")
    by_name, _ = renderer.render_aov(cam, ("depth", "albedo"), seed=SEED, real_type=rt)
    assert sorted(by_name) == ["albedo", "depth"]
    same(by_name, full)
    # the device form writes the planes the host form returns, one after the other
    n = cam.image_width * cam.image_height
    buf = torch.full((n * 8,), -7.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    assert renderer.render_aov_device(cam, buf.data_ptr(), seed=SEED, real_type=rt) is None
    renderer.synchronize()
    flat = buf.cpu().numpy()
    want = np.concatenate([full[name].reshape(-1) for name in NAMES])
    assert flat.tobytes() == want.tobytes()
    st = renderer.render_aov_device(cam, buf.data_ptr(), A.CR_AOV_DEPTH, seed=SEED, real_type=rt, want_stats=True)
    assert st["samples"] == n * cam.samples
    assert buf.cpu().numpy()[:n].tobytes() == full["depth"].tobytes()


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_shards(renderer, oracles, rt, tag):
    sc = resize(mixed_scene(), 24, 16, 5)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    R = oracles[rt].np_real
    for output_sum in (0, 1):   # a shard [1, 4) of 5 samples
        want, _ = model(oracles[rt], sc, SEED, sample_begin=1, sample_count=3, output_sum=output_sum)
        got, st = renderer.render_aov(cam, seed=SEED, real_type=rt, sample_begin=1, sample_count=3, output_sum=output_sum)
        same(got, want, f"output_sum {output_sum}")
        assert st["samples"] == 24 * 16 * 3
    # The words of shards add to the whole frame's, read through output_sum = 1 in f64.  A sum in reals is word * 2^-52 here
    # (S = 52 up to 2047 samples), which f64 holds exactly only below 2^53 -- a sum of up to 2 (a pixel's 5 samples reach 5
    # and round) -- so the shards are single samples: their reals ARE their words, and Python adds them as integers.
    S = fx_log2(cam.samples)
    shards = [renderer.render_aov(cam, seed=SEED, real_type=A.CR_REAL_F64, sample_begin=k, sample_count=1, output_sum=1)[0] for k in range(5)]
    for output_sum in (0, 1):
        whole, _ = renderer.render_aov(cam, seed=SEED, real_type=A.CR_REAL_F64, output_sum=output_sum)
        for name in ("albedo", "normal", "coverage"):
            words = [[int(v * 2.0 ** S) for v in sh[name].reshape(-1)] for sh in shards]
            assert all(float(w) * 2.0 ** -S == v for ws, sh in zip(words, shards) for w, v in zip(ws, sh[name].reshape(-1)))
            total = [sum(ws[k] for ws in words) for k in range(len(words[0]))]
            want = np.array([(float(abs(t) >> 32) * 4294967296.0 + float(abs(t) & 0xFFFFFFFF)) * 2.0 ** -S * (-1 if t < 0 else 1)
                             / (1.0 if output_sum else float(cam.samples)) for t in total]).reshape(whole[name].shape)
            assert want.tobytes() == whole[name].tobytes(), (name, output_sum)
        assert np.minimum.reduce([sh["depth"] for sh in shards]).tobytes() == whole["depth"].tobytes()
    empty, st = renderer.render_aov(cam, seed=SEED, real_type=rt, sample_begin=2, sample_count=0)
    assert st["samples"] == 0 and not empty["albedo"].any() and not empty["normal"].any() and not empty["coverage"].any()
    assert np.isposinf(empty["depth"]).all() and empty["depth"].dtype == R


# ---- refit
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_refit_boxes(renderer, oracles, rt, tag):
    sc = resize(moving_scene(frame=0), 24, 16, 3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    before, _ = renderer.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    plain, _ = renderer.render_aov(cam, seed=SEED, real_type=rt)
    cam.refit_boxes = True
    got, st = renderer.render_aov(cam, seed=SEED, real_type=rt)
    want, _ = model(oracles[rt], sc, SEED)   # primed by a refit render of the oracle
    same(got, want, "refit")
    check_counters(renderer, sc, rt, st)
    assert got["coverage"].tobytes() != plain["coverage"].tobytes()   # keys move inside the exposure: the old boxes lose hits
    cam.refit_boxes = False   # a guide render is not sticky: the construction-time boxes again
    again, _ = renderer.render_aov(cam, seed=SEED, real_type=rt)
    same(again, plain, "after refit")
    after, _ = renderer.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    assert after.tobytes() == before.tobytes()


# ---- refusals
def test_refusals_leave_the_handle_alone(hiplib, renderer):
    fresh = Renderer(0)
    try:
        sc0 = resize(few_spheres(3), 8, 8, 2)
        with pytest.raises(CrucibleError) as e:
            fresh.render_aov(sc0.scene_cam, seed=SEED)
        assert e.value.code == A.CR_ERR_NO_SCENE
    finally:
        fresh.close()
    sc = resize(mixed_scene(), 24, 16, 3)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    before, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F32, sum_order=A.CR_SUM_RELAXED)

    def refused(code, layers=A.CR_AOV_ALL, **kw):
        with pytest.raises(CrucibleError) as e:
            renderer.render_aov(cam, layers, seed=SEED, **kw)
        assert e.value.code == code
        after, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F32, sum_order=A.CR_SUM_RELAXED)
        assert after.tobytes() == before.tobytes()

    refused(A.CR_ERR_INVALID_ARG, layers=0)
    refused(A.CR_ERR_INVALID_ARG, layers=16)
    refused(A.CR_ERR_INVALID_ARG, layers=-1)
    refused(A.CR_ERR_UNSUPPORTED, output_sum=A.CR_OUTPUT_FIXED_SUM)
    refused(A.CR_ERR_INVALID_ARG, sample_begin=2, sample_count=5)   # what cr_render_device rejects
    refused(A.CR_ERR_INVALID_ARG, real_type=7)
    cam.set_max_depth(-1)   # validated like a render's, though the pass does not read it
    with pytest.raises(CrucibleError) as e:
        renderer.render_aov(cam, seed=SEED)
    assert e.value.code == A.CR_ERR_INVALID_ARG
    cam.set_max_depth(12)
    got, _ = renderer.render_aov(cam, seed=SEED)
    assert sorted(got) == sorted(NAMES)
    after, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F32, sum_order=A.CR_SUM_RELAXED)
    assert after.tobytes() == before.tobytes()


@pytest.mark.parametrize("pipeline", ["wavefront", "queue"])
def test_every_pipeline_setting(hiplib, renderer, monkeypatch, pipeline):
    sc = resize(mixed_scene(), 24, 16, 3)
    renderer.upload_scene(sc.flatten())
    want, _ = renderer.render_aov(sc.scene_cam, seed=SEED, real_type=A.CR_REAL_F64)
    monkeypatch.setenv("CRUCIBLE_PIPELINE", pipeline)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        got, _ = r.render_aov(sc.scene_cam, seed=SEED, real_type=A.CR_REAL_F64)
        same(got, want, pipeline)
    finally:
        r.close()
