"""The division-free decode of work items (crucible_amd/csrc/fastdiv.hpp) and the out-of-line trigonometry of the f64
kernels, on the device.  Frames whose decode is awkward -- one pixel, one row, sides that are multiples of no tile side, sample
counts around the group of four and around 64, a shard that begins past sample 0 -- under the default tile and under
CRUCIBLE_SG_TILE = 8x8 and 2x2: the reference order bit for bit against the oracle, the relaxed sums within the relaxed
tolerance of tests/test_gpu_relaxed.py (and bit for bit against the relaxed oracle), with samples == W * H * spp and the
oracle's work counters.  A batch of three frames through cr_render_frames_device and the guide layers at 5 x 7 decode the
same items.  A scene with an image-textured sphere under the spherical sky runs acos, atan2 and asin, with the tree in LDS
and forced below the LDS window."""
import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer
from crucible_amd.scene import ImageTexture, Lambertian, Metal, RTWImage, Scene, Sphere
from test_gpu_aov import parity as aov_parity
from test_gpu_frames import oracle_frames
from test_gpu_relaxed import TOL

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
REAL_IDS = [t for _, t in REALS]
REF, RELAX = A.CR_SUM_REFERENCE_ORDER, A.CR_SUM_RELAXED
SIZES = [(1, 1), (3, 2), (5, 7), (13, 1), (67, 9)]
SPPS = [1, 3, 5, 64, 65]
TILES = [None, "8x8", "2x2"]
TILE_IDS = ["tile-default", "tile-8x8", "tile-2x2"]


def sized(w, h, spp):
    sc = scenes.extent_scene(w, h, spp)
    assert (sc.scene_cam.image_width, sc.scene_cam.image_height, sc.scene_cam.samples) == (w, h, spp)
    return sc


_WANT = {}


def want(oracles, rt, w, h, spp, order, **kw):
    """The oracle's frame and counters, computed once per case and shared by the tile shapes."""
    key = (rt, w, h, spp, order, tuple(sorted(kw.items())))
    if key not in _WANT:
        img, st = oracles[rt].render_image(sized(w, h, spp), seed=SEED, sum_order=order, **kw)
        img.setflags(write=False)
        _WANT[key] = (img, st)
    return _WANT[key]


@pytest.fixture(scope="module", params=TILES, ids=TILE_IDS)
def tiled(request):
    """A handle under the tile shape of the case (None: the renderer's own choice by the sample count)."""
    mp = pytest.MonkeyPatch()
    if request.param:
        mp.setenv("CRUCIBLE_SG_TILE", request.param)
    r = Renderer(0)
    mp.undo()   # (the handle read its settings when it was created)
    yield r
    r.close()


def check_frame(r, oracles, rt, w, h, spp, **kw):
    sc = sized(w, h, spp)
    r.upload_scene(sc.flatten())
    n = kw.get("sample_count", spp)
    ref, rst = want(oracles, rt, w, h, spp, REF, **kw)
    img, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=REF, **kw)
    assert img.dtype == ref.dtype and img.shape == (h, w, 3)
    assert np.array_equal(img, ref), f"reference order: {(img != ref).any(axis=-1).sum()} pixels differ"
    xref, xst = want(oracles, rt, w, h, spp, RELAX, **kw)
    fast, fst = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=RELAX, **kw)
    assert np.abs(fast.astype(np.float64) - ref.astype(np.float64)).max() <= TOL[rt]
    assert np.array_equal(fast, xref), f"relaxed sums: {(fast != xref).any(axis=-1).sum()} pixels differ from the relaxed oracle"
    for s, o in ((st, rst), (fst, xst)):
        assert s["samples"] == w * h * n
        for k in COUNTERS:
            assert s[k] == o[k], (k, s[k], o[k])


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_awkward_frames(tiled, oracles, rt, tag, w, h, spp):
    check_frame(tiled, oracles, rt, w, h, spp)


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("spp,begin,count", [(5, 2, 3), (65, 3, 62), (65, 64, 1)])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_awkward_shards(tiled, oracles, rt, tag, w, h, spp, begin, count):
    """Samples [begin, begin + count) of the frame's spp: the groups start at a sample that is no multiple of their size.
    (The shard's mean, not its sum: the relaxed tolerance is one of colours in [0, 1].)"""
    check_frame(tiled, oracles, rt, w, h, spp, sample_begin=begin, sample_count=count)


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("w,h,spp", [(5, 7, 3), (67, 9, 5), (13, 1, 1)])
def test_three_frames_on_the_device(tiled, rt, tag, w, h, spp):
    """A batch's tile rows follow each other: the decode divides by tiles_x, the frame of a row by tiles_y."""
    import torch
    sc = scenes.extent_scene(w, h, spp, keyed=True)
    frames = [2, 0, 5]
    tiled.upload_scene(sc.flatten())
    d = torch.full((len(frames), h, w, 3), -1.0, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    st = tiled.render_frames_device(sc.scene_cam, frames, d.data_ptr(), seed=SEED, real_type=rt, sum_order=RELAX, want_stats=True)
    got = d.cpu().numpy()
    refs, rst = oracle_frames(sc, frames, rt)
    assert st["samples"] == w * h * spp * len(frames)
    for k, ref in enumerate(refs):
        assert got[k].tobytes() == ref.tobytes(), f"frame {frames[k]} (entry {k}) differs from the relaxed oracle"
    for c in COUNTERS:
        assert st[c] == rst[c], (c, st[c], rst[c])
    assert got[0].tobytes() != got[1].tobytes()   # (the camera moved)


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("spp", [1, 5])
def test_guide_layers_5x7(renderer, oracles, rt, tag, spp):
    _, st = aov_parity(renderer, oracles, sized(5, 7, spp), rt)
    assert st["samples"] == 5 * 7 * spp


# ---- acos, atan2, asin: Sphere uv on an image texture, the spherical sky
def globe_scene():
    """16 x 12: a sphere with an image texture (Sphere::get_sphere_uv: acos, atan2), a mirror that shows the sky all around,
    under a spherical sky map (atan2, asin).  Image sizes that are no power of two, so that texel indices move with the last bits."""
    sc = Scene.new_image(4.0 / 3.0, 16, 24, 180.0, 1)
    cam = sc.scene_cam
    assert (cam.image_width, cam.image_height) == (16, 12)
    cam.set_samples(4)
    cam.set_max_depth(6)
    cam.look_from((0.0, 1.2, 5.0))
    cam.look_at((0.0, 0.6, 0.0))
    cam.set_vfov(40.0)
    rs = np.random.RandomState(5)
    sc.add_element(Sphere.new((-0.9, 0.8, 0.0), 0.8, Lambertian.new_from_texture(ImageTexture(RTWImage(rs.randint(0, 256, size=(23, 47, 3)).astype(np.uint8))), 1.0)), "globe")
    sc.add_element(Sphere.new((0.9, 0.7, 0.2), 0.7, Metal.new((0.9, 0.9, 0.9), 0.0)), "mirror")
    sc.add_element(Sphere.new((0.0, -50.0, 0.0), 50.0, Lambertian.new_from_texture(ImageTexture(RTWImage(rs.randint(0, 256, size=(31, 61, 3)).astype(np.uint8))), 0.9)), "ground")
    sc.load_spherical_skybox(RTWImage(rs.randint(40, 256, size=(37, 75, 3)).astype(np.uint8)))
    return sc


@pytest.fixture(scope="module")
def globe_want(oracles):
    sc = globe_scene()
    out = {}
    for rt, _ in REALS:
        for order in (REF, RELAX):
            img, st = oracles[rt].render_image(sc, seed=SEED, sum_order=order)
            img.setflags(write=False)
            out[rt, order] = (img, st)
    return out


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("env,res", [({}, 1), ({"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "1"}, 2), ({"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "0"}, 0)],
                         ids=["scene-in-lds", "tree-top-in-lds", "scene-in-global-memory"])
def test_textured_sphere_under_the_spherical_sky(monkeypatch, oracles, globe_want, rt, tag, env, res):
    sc = globe_scene()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        ref, rst = globe_want[rt, REF]
        img, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=REF)
        assert st["scene_in_lds"] == res
        assert st["texel_fetches"] > 16 * 12 * 4   # the sky or a texture in every path, both in most
        assert np.array_equal(img, ref), f"reference order: {(img != ref).any(axis=-1).sum()} pixels differ"
        xref, xst = globe_want[rt, RELAX]
        fast, fst = r.render(sc.scene_cam, seed=SEED, real_type=rt, sum_order=RELAX)
        assert fst["scene_in_lds"] == res
        assert np.abs(fast.astype(np.float64) - ref.astype(np.float64)).max() <= TOL[rt]
        assert np.array_equal(fast, xref)
        for s, o in ((st, rst), (fst, xst)):
            assert s["samples"] == 16 * 12 * 4
            for k in COUNTERS:
                assert s[k] == o[k], (k, s[k], o[k])
        # the guide layers' albedo of the globe goes through the same acos / atan2
        aov_parity(r, oracles, sc, rt)
    finally:
        r.close()
