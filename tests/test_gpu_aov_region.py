"""cr_render_aov_region_device / cr_render_aov_region_host: the guide layers of a region.  Every plane of a region
(x0, y0, w, h) is, byte for byte, the crop of cr_render_aov_host's plane of the whole frame -- all layers, a subset and a
single layer (the layout follows the region's size), in f32 and f64, output_sum 1 and a shard, under the suite's default
sum order and on a CRUCIBLE_PIPELINE=queue handle -- and the counters of a partition add up to the frame's."""
import ctypes as C

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from test_gpu_region import COUNTERS, EXTRA, H, P, REALS, SCENES, W, crop, odd_size, scaled  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
LAYER_SETS = [A.CR_AOV_ALL, ("albedo", "depth"), ("coverage",)]


def check_planes(r, sc, rt, regions, partition, layers=A.CR_AOV_ALL, **kw):
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    full, fst = r.render_aov(cam, layers, seed=SEED, real_type=rt, **kw)
    tot = {c: 0 for c in COUNTERS + ("samples",)}
    for reg in regions:
        got, st = r.render_aov_region(cam, reg, layers, seed=SEED, real_type=rt, **kw)
        assert list(got) == list(full)
        for name, plane in got.items():
            want = crop(full[name], reg)
            assert plane.shape == want.shape and plane.dtype == want.dtype
            assert plane.tobytes() == want.tobytes(), f"{name} of region {reg} differs from the crop"
        assert st["segments"] == st["samples"] and st["nan_pixels"] == 0
        if reg in partition:
            for c in tot:
                tot[c] += st[c]
    if partition:
        for c in tot:
            assert tot[c] == fst[c], (c, tot[c], fst[c])
    return full, fst


@pytest.mark.parametrize("rt,name", REALS)
@pytest.mark.parametrize("which", list(SCENES))
def test_planes_are_crops(renderer, rt, name, which):
    sc = SCENES[which]()
    cam = sc.scene_cam
    part = scaled(P, cam.image_width, cam.image_height)
    extra = scaled(EXTRA, cam.image_width, cam.image_height)
    _, fst = check_planes(renderer, sc, rt, part + extra, part)
    if which == "teapot":
        assert fst["scene_in_lds"] == 2
    for layers in LAYER_SETS[1:]:
        check_planes(renderer, sc, rt, part + extra, part, layers)


@pytest.mark.parametrize("rt,name", REALS)
def test_output_sum_and_shard(renderer, rt, name):
    sc = odd_size(scenes.mixed_scene(samples=5, animate=True))
    check_planes(renderer, sc, rt, P, P, output_sum=1)
    check_planes(renderer, sc, rt, P, P, sample_begin=1, sample_count=3)
    check_planes(renderer, sc, rt, [P[3]], [], output_sum=1, sample_begin=1, sample_count=3)


@pytest.mark.parametrize("rt,name", REALS)
def test_depth_is_inf_where_the_regions_samples_miss(renderer, rt, name):
    """A scene without a sky sphere leaves pixels whose samples all miss: their depth is +inf in the region too."""
    sc = odd_size(scenes.few_spheres(6, samples=3))
    full, _ = check_planes(renderer, sc, rt, P + EXTRA, P)
    got, _ = renderer.render_aov_region(sc.scene_cam, P[1], ("depth", "coverage"), seed=SEED, real_type=rt)
    miss = got["coverage"] == 0
    assert miss.any() and np.isposinf(got["depth"][miss]).all() and np.isfinite(got["depth"][~miss]).all()
    # an empty shard writes what the single guide call writes: no hit anywhere
    got, st = renderer.render_aov_region(sc.scene_cam, P[3], seed=SEED, real_type=rt, sample_begin=3, sample_count=0)
    want, _ = renderer.render_aov(sc.scene_cam, seed=SEED, real_type=rt, sample_begin=3, sample_count=0)
    assert st["samples"] == 0
    for name_, plane in got.items():
        assert plane.tobytes() == crop(want[name_], P[3]).tobytes(), name_


def test_queue_pipeline_handle(monkeypatch):
    """Guide calls work under every pipeline setting, region calls too."""
    monkeypatch.setenv("CRUCIBLE_PIPELINE", "queue")
    r = Renderer(0)
    monkeypatch.delenv("CRUCIBLE_PIPELINE")
    try:
        check_planes(r, odd_size(scenes.moving_scene(samples=5, frame=1)), A.CR_REAL_F64, P, P)
    finally:
        r.close()


def test_device_form(renderer):
    import torch
    sc = odd_size(scenes.moving_scene(samples=3, frame=1))
    cam = sc.scene_cam
    reg = P[3]
    renderer.upload_scene(sc.flatten())
    want, _ = renderer.render_aov_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64)
    d = torch.full((reg[2] * reg[3] * 8,), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert renderer.render_aov_region_device(cam, reg, d.data_ptr(), seed=SEED, real_type=A.CR_REAL_F64) is None
    renderer.synchronize()
    flat = np.concatenate([want[n].reshape(-1) for n, _, _ in A.AOV_LAYERS])
    assert d.cpu().numpy().tobytes() == flat.tobytes()
    assert renderer.last_kernel_ms() > 0


def test_refusals_leave_the_handle_usable(renderer):
    lib = renderer.lib
    sc = odd_size(scenes.moving_scene(samples=2, frame=1))
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    reg = P[3]
    ok = lambda: renderer.render_aov_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F64)[0]  # noqa: E731
    good = ok()
    same = lambda: all(ok()[n].tobytes() == good[n].tobytes() for n in good)  # noqa: E731
    cd, p = cam.desc(), cam.params(SEED, A.CR_REAL_F64, sum_order=A.CR_SUM_DEFAULT)
    out = np.empty(W * H * 8, dtype=np.float64)
    outp = out.ctypes.data_as(C.c_void_p)
    region = A.CrRegion(*reg)
    int_max = 2 ** 31 - 1
    for fn in (lib.cr_render_aov_region_host, lib.cr_render_aov_region_device):
        for layers in (0, 16, -1):
            assert fn(renderer.h, C.byref(cd), C.byref(p), layers, C.byref(region), outp, None) == A.CR_ERR_INVALID_ARG
            assert same(), layers
        fixed = cam.params(SEED, A.CR_REAL_F64, output_sum=A.CR_OUTPUT_FIXED_SUM, sum_order=A.CR_SUM_RELAXED)
        assert fn(renderer.h, C.byref(cd), C.byref(fixed), A.CR_AOV_ALL, C.byref(region), outp, None) == A.CR_ERR_UNSUPPORTED
        assert same()
        assert fn(renderer.h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, None, outp, None) == A.CR_ERR_INVALID_ARG
        assert same()
        assert fn(renderer.h, None, C.byref(p), A.CR_AOV_ALL, C.byref(region), outp, None) == A.CR_ERR_INVALID_ARG
        assert same()
        assert fn(renderer.h, C.byref(cd), None, A.CR_AOV_ALL, C.byref(region), outp, None) == A.CR_ERR_INVALID_ARG
        assert same()
        assert fn(renderer.h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, C.byref(region), None, None) == A.CR_ERR_INVALID_ARG
        assert same()
        for bad in ((0, 0, 0, 3), (0, 0, 3, -1), (-1, 0, 3, 3), (0, -1, 3, 3), (int_max, 0, 2, 1), (30, 0, 8, 3), (0, 20, 3, 4)):
            assert fn(renderer.h, C.byref(cd), C.byref(p), A.CR_AOV_ALL, C.byref(A.CrRegion(*bad)), outp, None) == A.CR_ERR_INVALID_ARG, bad
            assert same(), bad
        # a region above 2^26 pixels (the whole 16384 x 4100 frame), and a frame above 2^31 - 1 pixels
        big = odd_size(scenes.moving_scene(samples=2, frame=1), 16384, 4100).scene_cam.desc()
        assert fn(renderer.h, C.byref(big), C.byref(p), A.CR_AOV_DEPTH, C.byref(A.CrRegion(0, 0, 16384, 4100)), outp, None) == A.CR_ERR_INVALID_ARG
        assert same()
        huge = odd_size(scenes.moving_scene(samples=2, frame=1), 50000, 50000).scene_cam.desc()
        assert fn(renderer.h, C.byref(huge), C.byref(p), A.CR_AOV_DEPTH, C.byref(region), outp, None) == A.CR_ERR_INVALID_ARG
        assert b"2^31" in lib.cr_last_error(renderer.h)
        assert same()
