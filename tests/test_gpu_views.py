"""cr_render_views_* / cr_render_aov_views_*: several cameras of one scene in one launch.  The contract is bit-exact: view k
of a call is, byte for byte, what the single call writes for cams[k] at frame frames[k] (params->frame without a frame
list), the call's work counters are the sum of the single calls', and a guide call's four planes are the single guide
call's.  One view of every beauty case is also held to the relaxed oracle directly, image and four counters, so the suite
does not rest on self-consistency alone.

13 x 9 pixels: no multiple of a tile side (4 x 4 pixels at 4 and 5 samples, 8 x 4 at 3), so padding rows lie between the
views, and a view is 12 tiles -- the waves run across view boundaries and hold lanes of neighbouring views, whose cameras
differ in their defocus switch, in whether they carry keys and in how many.  Views need CR_SUM_RELAXED in the beauty form
(tests/conftest.py makes the reference order the suite default, so every render here names its sum order)."""
import copy
import ctypes as C

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import CrucibleError, Renderer, view_table
from crucible_amd.scene import LERP, NERP, WORLD
from test_gpu_frames import COUNTERS, REALS, RELAX, SEED

pytestmark = pytest.mark.gpu

W, H = 13, 9
NAMES = ("albedo", "normal", "depth", "coverage")


def sized(sc, samples):
    cam = sc.scene_cam
    cam.image_width, cam.image_height = W, H
    cam.set_samples(samples)
    cam.set_max_depth(4)
    return sc


def keyed_prims(samples=4):
    """Keyed primitives (the ANIM kernels): 1 fps, 360 degree shutter, frame f draws ray times in [f, f + 1]."""
    return sized(scenes.moving_scene(), samples)


def no_prim_keys(samples=4):
    """No primitive keys (the CAMK kernels): 24 fps, 180 degree shutter."""
    return sized(scenes.few_spheres(5), samples)


def view(cam, vfov=None, focus=None, defocus=None, vup=None, look_from=None, look_at=None, from_keys=0, at_keys=0):
    """A copy of `cam` that differs in what is named.  from_keys / at_keys: that many translate keys on look_from / look_at,
    LERP and NERP in turn, ending 0.4, 0.8, ... frames after the start so that they lie inside and across the frames 0..3."""
    c = copy.deepcopy(cam)
    if vfov is not None:
        c.set_vfov(vfov)
    if focus is not None:
        c.set_focus_dist(focus)
    if defocus is not None:
        c.set_defocus_angle(defocus)
    if vup is not None:
        c.set_vup(vup)
    if look_from is not None:
        c.look_from(look_from)
    if look_at is not None:
        c.look_at(look_at)
    for tl, n, amp in ((c.look_from_tl, from_keys, 0.8), (c.look_at_tl, at_keys, 0.3)):
        for k in range(n):
            value = tl.start_pos[k % 3] + amp * (1 + k) * (-1) ** k
            (tl.translate_x, tl.translate_y, tl.translate_z)[k % 3](value, 0.4 * (k + 1) / cam.frame_rate, NERP if k % 2 else LERP, WORLD)
    return c


def one_difference(cam):
    """Views that differ from the first in exactly one field of the camera."""
    f, a = cam.look_from_tl.start_pos, cam.look_at_tl.start_pos
    return [view(cam), view(cam, vfov=cam.vfov_degrees + 9.0), view(cam, focus=4.5), view(cam, vup=(0.3, 1.0, -0.2)),
            view(cam, look_from=(f[0] + 1.5, f[1] + 0.5, f[2] - 1.0)), view(cam, look_at=(a[0] - 0.7, a[1] + 0.4, a[2])), view(cam, defocus=2.5)]


def mixed(cam):
    """Five views whose lanes share waves: defocus on and off, keyed and unkeyed, 2, 5 and 3 keys."""
    return [view(cam), view(cam, defocus=2.0, focus=7.0), view(cam, from_keys=2), view(cam, from_keys=3, at_keys=2, defocus=1.5, focus=6.0),
            view(cam, vup=(0.2, 1.0, 0.1), vfov=cam.vfov_degrees - 7.0, at_keys=3)]


def at_frame(cam, frame):
    c = copy.copy(cam)
    c.frame = frame
    return c


def frames_of(cams, frames):
    return [cams[0].frame] * len(cams) if frames is None else list(frames)


_ORACLES = {}


def oracle_view(sc, cam, rt, **kw):
    """The relaxed oracle's image and counters of the scene through `cam`."""
    from oracle.oracle import Oracle
    o = _ORACLES.setdefault(rt, Oracle(rt))
    keep = sc.scene_cam
    sc.scene_cam = cam
    try:
        return o.render_image(sc, seed=SEED, sum_order=RELAX, **kw)
    finally:
        sc.scene_cam = keep


def check_views(r, sc, cams, frames, rt, oracle_at=0, singles_on=None, **kw):
    """The beauty call equals the single renders of its views bit for bit (singles_on: rendered on that handle instead), its
    counters are theirs summed, and view oracle_at is the relaxed oracle's image with the oracle's counters.  Returns
    (views, stats)."""
    r.upload_scene(sc.flatten())
    got, st = r.render_views(cams, frames, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
    assert got.shape == (len(cams), H, W, 3)
    s = singles_on or r
    if singles_on:
        s.upload_scene(sc.flatten())
    fr = frames_of(cams, frames)
    singles = [s.render(at_frame(c, f), seed=SEED, real_type=rt, sum_order=RELAX, **kw) for c, f in zip(cams, fr)]
    for k, (img, _) in enumerate(singles):
        assert got[k].dtype == img.dtype and got[k].tobytes() == img.tobytes(), f"view {k} differs from its single render"
    for c in COUNTERS + ("samples",):
        assert st[c] == sum(x[c] for _, x in singles), (c, st[c], [x[c] for _, x in singles])
    assert st["kernel_ms"] > 0
    if oracle_at is None:   # (a tree the oracle would have to be handed: its case's neighbour on the reference tree holds the oracle)
        return got, st
    ref, ost = oracle_view(sc, at_frame(cams[oracle_at], fr[oracle_at]), rt, **kw)
    assert got[oracle_at].dtype == ref.dtype and got[oracle_at].tobytes() == ref.tobytes(), f"view {oracle_at} differs from the relaxed oracle"
    for c in COUNTERS:
        assert singles[oracle_at][1][c] == ost[c], (c, singles[oracle_at][1][c], ost[c])
    return got, st


def check_guide_views(r, sc, cams, frames, rt, **kw):
    """The guide call equals the single guide calls of its views in all four planes, its counters are theirs summed."""
    r.upload_scene(sc.flatten())
    got, st = r.render_aov_views(cams, frames, seed=SEED, real_type=rt, **kw)
    assert len(got) == len(cams)
    singles = [r.render_aov(at_frame(c, f), seed=SEED, real_type=rt, **kw) for c, f in zip(cams, frames_of(cams, frames))]
    for k, (planes, _) in enumerate(singles):
        assert sorted(got[k]) == sorted(NAMES)
        for n in NAMES:
            assert got[k][n].shape == planes[n].shape and got[k][n].tobytes() == planes[n].tobytes(), f"view {k}: plane {n} differs from the single call's"
    for c in COUNTERS + ("samples",):
        assert st[c] == sum(x[c] for _, x in singles), (c, st[c], [x[c] for _, x in singles])
    return got, st


def differ(got):
    return [k for k in range(1, len(got)) if got[k].tobytes() != got[0].tobytes()]


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("build", [keyed_prims, no_prim_keys], ids=["anim", "camk"])
def test_views_that_differ_in_one_field(renderer, rt, name, build):
    """vfov, focus_dist, vup, look_from, look_at, defocus: each view differs from view 0 in exactly one of them, and in its image."""
    sc = build()
    cams = one_difference(sc.scene_cam)
    got, _ = check_views(renderer, sc, cams, None, rt, oracle_at=3)
    assert differ(got) == list(range(1, len(cams)))
    planes, _ = check_guide_views(renderer, sc, cams, None, rt)
    assert any(planes[k]["depth"].tobytes() != planes[0]["depth"].tobytes() for k in range(1, len(cams)))


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("build", [keyed_prims, no_prim_keys], ids=["anim", "camk"])
@pytest.mark.parametrize("n,frames", [(1, None), (1, [2]), (2, [1, 0]), (5, [3, 0, 3, 1, 0]), (5, None)],
                         ids=["one", "one-at-2", "two", "five-frames", "five-null-frames"])
def test_mixed_views_and_frame_lists(renderer, rt, name, build, n, frames):
    """1, 2 and 5 views of the mixed set, with a frame list and without: defocus on and off, keyed and unkeyed cameras and
    different key counts in one launch.  A one-view call gives the single call's bytes and counters."""
    sc = build()
    cams = mixed(sc.scene_cam)[-n:] if n < 5 else mixed(sc.scene_cam)
    check_views(renderer, sc, cams, frames, rt, oracle_at=n - 1)
    check_guide_views(renderer, sc, cams, frames, rt)


@pytest.mark.parametrize("rt,name", REALS)
def test_repeated_view(renderer, rt, name):
    """The same view twice (and the same frame twice): the same bytes twice, beside a view that differs."""
    sc = keyed_prims()
    m = mixed(sc.scene_cam)
    cams = [m[3], m[1], m[3]]
    got, _ = check_views(renderer, sc, cams, [2, 2, 2], rt)
    assert got[0].tobytes() == got[2].tobytes() != got[1].tobytes()
    planes, _ = check_guide_views(renderer, sc, cams, [2, 2, 2], rt)
    assert all(planes[0][n].tobytes() == planes[2][n].tobytes() for n in NAMES)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("output_sum", [0, 1, A.CR_OUTPUT_FIXED_SUM], ids=["mean", "sum", "fixed"])
@pytest.mark.parametrize("shard", [None, (1, 2)], ids=["whole", "shard"])
def test_output_modes_and_shards(renderer, rt, name, output_sum, shard):
    """The mean, sums in reals and fixed-point words at the whole frame's scale; the shard [1, 3) of 5 samples."""
    kw = {"output_sum": output_sum}
    if shard:
        kw.update(sample_begin=shard[0], sample_count=shard[1])
    sc = keyed_prims(samples=5)
    cams = mixed(sc.scene_cam)[1:4]
    got, _ = check_views(renderer, sc, cams, [0, 2, 1], rt, oracle_at=2, **kw)
    assert got.dtype == (np.uint64 if output_sum == A.CR_OUTPUT_FIXED_SUM else (np.float64 if rt == A.CR_REAL_F64 else np.float32))
    if output_sum != A.CR_OUTPUT_FIXED_SUM:
        check_guide_views(renderer, sc, cams, [0, 2, 1], rt, **kw)


@pytest.mark.parametrize("spp", [3, 5])
def test_other_tile_shapes(renderer, spp):
    """3 samples: 8 x 4 pixel tiles; 5 samples: two sample groups, the second mostly padding."""
    sc = no_prim_keys(samples=spp)
    check_views(renderer, sc, mixed(sc.scene_cam), [3, 0, 3, 1, 0], A.CR_REAL_F32, oracle_at=3)


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("build", [keyed_prims, no_prim_keys], ids=["anim", "camk"])
@pytest.mark.parametrize("env,res", [({}, 1), ({"CRUCIBLE_LDS_LIMIT": "0"}, 2), ({"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "0"}, 0)],
                         ids=["lds", "top", "global"])
@pytest.mark.parametrize("bvh", [A.CR_BVH_REFERENCE, A.CR_BVH_SAH_ORDERED], ids=["reference", "ordered"])
def test_residencies_and_tree_orders(monkeypatch, rt, name, build, env, res, bvh):
    """The scene in LDS, the tree's top levels in LDS, everything in global memory; the reference tree and the ordered one."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = Renderer(0)
    try:
        sc = build()
        sc.bvh_mode = bvh
        cams = mixed(sc.scene_cam)
        _, st = check_views(r, sc, cams, [3, 0, 3, 1, 0], rt, oracle_at=3 if bvh == A.CR_BVH_REFERENCE else None)
        assert st["scene_in_lds"] == res
        _, gst = check_guide_views(r, sc, cams, [3, 0, 3, 1, 0], rt)
        assert gst["scene_in_lds"] == res
    finally:
        r.close()


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("limit,spp", [(1600, 4), (768, 5)], ids=["whole-views", "sample-batches"])
def test_work_counter_split(monkeypatch, rt, name, limit, spp):
    """A small CRUCIBLE_WORK_COUNTER_MAX: 13 x 9 at 4 samples is 12 tiles x 64 = 768 work items a view, so 1600 holds two views
    per launch (five views: three launches); at 5 samples a view is two sample groups, 1536 items, and alone needs two
    sample batches under a limit of 768: the call runs view by view.  The single renders are an unrestricted handle's."""
    sc = keyed_prims(samples=spp)
    cams = mixed(sc.scene_cam)
    monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", str(limit))
    small = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_WORK_COUNTER_MAX")
    big = Renderer(0)
    try:
        check_views(small, sc, cams, [3, 0, 3, 1, 0], rt, oracle_at=4, singles_on=big)
        check_guide_views(small, sc, cams, [3, 0, 3, 1, 0], rt)
    finally:
        small.close()
        big.close()


def test_device_forms(renderer):
    """cr_render_views_device and cr_render_aov_views_device write the same views, one after the other, into device memory."""
    import torch
    sc = keyed_prims()
    renderer.upload_scene(sc.flatten())
    cams = mixed(sc.scene_cam)[:3]
    want, _ = renderer.render_views(cams, [1, 0, 2], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    d = torch.full((3, H, W, 3), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = renderer.render_views_device(cams, d.data_ptr(), [1, 0, 2], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX, want_stats=True)
    assert st["samples"] == W * H * 4 * 3
    assert d.cpu().numpy().tobytes() == want.tobytes()
    planes, _ = renderer.render_aov_views(cams, [1, 0, 2], seed=SEED, real_type=A.CR_REAL_F32)
    g = torch.full((3, 8 * H * W), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    renderer.render_aov_views_device(cams, g.data_ptr(), [1, 0, 2], seed=SEED, real_type=A.CR_REAL_F32)
    renderer.synchronize()
    host = g.cpu().numpy()
    for k in range(3):
        assert host[k].tobytes() == b"".join(planes[k][n].tobytes() for n in NAMES)


def test_nan_view_is_named(renderer):
    """The host form's Color::new check applies view by view: a camera without a basis (look_at on look_from) gives NaN
    means, and CR_ERR_NAN's message names that view."""
    sc = keyed_prims()
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    cams = [view(cam), view(cam, look_at=cam.look_from_tl.start_pos), view(cam, vfov=25.0)]
    with pytest.raises(CrucibleError) as e:
        renderer.render_views(cams, [0, 2, 1], seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    assert e.value.code == A.CR_ERR_NAN and "view 1 (frame 2)" in str(e.value)


def many_keys(cam, n_from, n_at):
    c = copy.deepcopy(cam)
    for tl, n in ((c.look_from_tl, n_from), (c.look_at_tl, n_at)):
        for k in range(n):
            (tl.translate_x, tl.translate_y, tl.translate_z)[k % 3](tl.start_pos[k % 3] + 0.01 * (k % 7), 0.001 * (k + 1), LERP, WORLD)
    return c


def test_refusals_leave_the_handle_as_it_was(renderer):
    """Every refusal of the four calls, and after each a plain cr_render_host on the handle gives a fresh handle's bytes."""
    lib, h = renderer.lib, renderer.h
    sc = keyed_prims()
    cam = sc.scene_cam
    fresh = Renderer(0)
    try:
        fresh.upload_scene(sc.flatten())
        want, _ = fresh.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
    finally:
        fresh.close()
    renderer.upload_scene(sc.flatten())

    def untouched():
        img, _ = renderer.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=RELAX)
        assert img.tobytes() == want.tobytes()

    cams = mixed(cam)[:3]
    kw = dict(seed=SEED, real_type=A.CR_REAL_F64)

    def refused(code, word, call, **more):
        with pytest.raises(CrucibleError) as e:
            call(**{**kw, **more})
        assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))
        untouched()

    beauty = lambda **k: renderer.render_views(cams, None, **k)            # noqa: E731
    guide = lambda **k: renderer.render_aov_views(cams, None, **k)         # noqa: E731
    # the sum order: named, and the handle's default (CRUCIBLE_SUM_ORDER=reference, tests/conftest.py); the guide form takes both
    refused(A.CR_ERR_UNSUPPORTED, "CR_SUM_RELAXED", beauty, sum_order=A.CR_SUM_REFERENCE_ORDER)
    refused(A.CR_ERR_UNSUPPORTED, "CR_SUM_RELAXED", beauty, sum_order=A.CR_SUM_DEFAULT)
    guide(**kw)
    # fixed-point words on the guide form
    refused(A.CR_ERR_UNSUPPORTED, "fixed-point", guide, output_sum=A.CR_OUTPUT_FIXED_SUM)
    # a refit that would change boxes (keyed primitives)
    for c in cams:
        c.refit_boxes = True
    refused(A.CR_ERR_UNSUPPORTED, "refit", beauty, sum_order=RELAX)
    refused(A.CR_ERR_UNSUPPORTED, "refit", guide)
    for c in cams:
        c.refit_boxes = False
    # 513 keys over all views: 300 + 212 are a single camera's limit, one more view with one key passes it
    full = many_keys(cam, 300, 212)
    renderer.render_views([full, view(cam)], None, sum_order=RELAX, **kw)
    over = [full, view(cam), view(cam, from_keys=1)]
    refused(A.CR_ERR_UNSUPPORTED, "512", lambda **k: renderer.render_views(over, None, **k), sum_order=RELAX)
    refused(A.CR_ERR_UNSUPPORTED, "512", lambda **k: renderer.render_aov_views(over, None, **k))
    # views of another size
    other = view(cam)
    other.image_width = W + 1
    refused(A.CR_ERR_INVALID_ARG, "view 2", lambda **k: renderer.render_views([cams[0], cams[1], other], None, **k), sum_order=RELAX)
    refused(A.CR_ERR_INVALID_ARG, "view 2", lambda **k: renderer.render_aov_views([cams[0], cams[1], other], None, **k))
    # what the single call rejects for one view: the message names the first such view
    table, keep = view_table(cams)
    table[1].from_key_count = -1
    table[2].image_width = 0
    p = cam.params(SEED, A.CR_REAL_F64, sum_order=RELAX)
    out = np.empty((3, H, W, 3), dtype=np.float64)
    outp = out.ctypes.data_as(C.c_void_p)
    for fn, extra in ((lib.cr_render_views_host, ()), (lib.cr_render_views_device, ()), (lib.cr_render_aov_views_host, (A.CR_AOV_ALL,)),
                      (lib.cr_render_aov_views_device, (A.CR_AOV_ALL,))):
        assert fn(h, table, 3, None, C.byref(p), *extra, outp, None) == A.CR_ERR_INVALID_ARG
        assert "view 1" in lib.cr_last_error(h).decode()
    untouched()
    # null cams, n_views < 1, a null output, params the single call rejects, an empty layer mask
    table, keep = view_table(cams)
    bad = cam.params(SEED, A.CR_REAL_F64, sample_begin=3, sample_count=2, sum_order=RELAX)   # 4 samples: [3, 5) is outside
    for fn, extra in ((lib.cr_render_views_host, ()), (lib.cr_render_views_device, ()), (lib.cr_render_aov_views_host, (A.CR_AOV_ALL,)),
                      (lib.cr_render_aov_views_device, (A.CR_AOV_ALL,))):
        for t, n, params, o in ((None, 3, p, outp), (table, 0, p, outp), (table, -2, p, outp), (table, 3, p, None), (table, 3, bad, outp)):
            assert fn(h, t, n, None, C.byref(params), *extra, o, None) == A.CR_ERR_INVALID_ARG, (fn.__name__, n)
    assert lib.cr_render_aov_views_host(h, table, 3, None, C.byref(p), 0, outp, None) == A.CR_ERR_INVALID_ARG
    untouched()
    del keep
