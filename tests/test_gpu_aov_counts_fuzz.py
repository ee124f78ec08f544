"""The hostile corpus of tests/test_gpu_fuzz.py through cr_render_aov_counts_*: the scenes that
tests/test_gpu_fuzz_entry_points.py names for the NaN flags, the negative words, the depth minimum and the start of the hit
interval (EDGES, by the rota of their seeds: reference tree, refit boxes, an opt-in tree), under a fixed two-valued plane split
along the diagonal, so that tiles straddle it.  Every pixel is compared with the sibling cr_render_aov_* call at its own
count, bytes and NaN positions.  The selection is made on the CPU: a guide call has no Color::new check, so no seed has
to be left out for the oracle's nan_pixels -- test_gpu_fuzz_entry_points.py asks that of its beauty and batch cases only --
and the scenes the Python mirror itself rejects are not among EDGES (checked below).  The rest of the hostile list
(HOSTILE_SEEDS beyond EDGES, which tests/test_gpu_fuzz_entry_points.py runs through the plain guide pass) is left out on
purpose: those scenes show none of the named properties, and the count plane's own paths are in tests/test_gpu_aov_counts.py."""
import numpy as np
import pytest

from crucible_amd import _abi as A
from test_gpu_aov import NAMES
from test_gpu_fuzz_entry_points import EDGES, make_scene, set_variant

REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
SEEDS = sorted({seed for cases in EDGES.values() for seed, _ in cases})


def diagonal_plane(w, h, low, high):
    """`low` below the diagonal from (0, 0) to (w, h), `high` on and above it"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(x * h >= y * w, high, low).astype(np.int32)


def case(seed):
    sc, rseed = make_scene("hostile", seed)
    set_variant(sc, seed)
    cam = sc.scene_cam
    low = max(1, cam.samples // 2) if cam.samples > 1 else 0
    return sc, rseed, diagonal_plane(cam.image_width, cam.image_height, low, cam.samples), low


def test_the_selection():
    assert len(SEEDS) >= 8 and {"a", "b"} <= set(EDGES)   # flagged channels and negative words are in the corpus
    for seed in SEEDS:
        sc, _, plane, low = case(seed)   # (a scene the mirror rejects would raise ValueError here)
        cam = sc.scene_cam
        assert cam.samples <= 2047 and low < cam.samples and set(np.unique(plane)) == {low, cam.samples}, seed
        # some 4 x 4 tile holds both values
        th, tw = -(-cam.image_height // 4), -(-cam.image_width // 4)
        pad = np.full((th * 4, tw * 4), -1, dtype=np.int32)
        pad[:cam.image_height, :cam.image_width] = plane
        tiles = pad.reshape(th, 4, tw, 4).transpose(0, 2, 1, 3).reshape(th * tw, 16)
        assert any((t == low).any() and (t == cam.samples).any() for t in tiles), seed


@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("seed", SEEDS)
def test_hostile_scenes_per_count(renderer, seed, rt, tag):
    sc, rseed, plane, low = case(seed)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    got, st = renderer.render_aov_counts(cam, plane, seed=rseed, real_type=rt)
    assert sorted(got) == sorted(NAMES) and st["samples"] == st["segments"] == int(plane.sum()) and st["nan_pixels"] == 0
    samples = cam.samples
    for c in (low, samples):
        mask = plane == c
        if c == 0:
            for n in ("albedo", "normal", "coverage"):
                assert not np.frombuffer(got[n][mask].tobytes(), dtype=np.uint8).any(), n
            assert np.isposinf(got["depth"][mask]).all()
            continue
        cam.set_samples(c)
        try:
            want, _ = renderer.render_aov(cam, seed=rseed, real_type=rt)
        finally:
            cam.set_samples(samples)
        for n in NAMES:
            assert np.array_equal(np.isnan(got[n][mask]), np.isnan(want[n][mask])), (n, c)
            assert got[n][mask].tobytes() == want[n][mask].tobytes(), (n, c)
