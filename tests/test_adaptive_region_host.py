"""The region functions of crucible_amd/csrc/adaptive.hpp (cr_render_adaptive_region_*), checked without a device:
tests/adaptive_region_check.cpp compiles the header with g++ (plain, and with -fsanitize=address,undefined) and prints, for a
region of a frame, the predicate "the region's blocks are the frame's", the region's block grid and every block's rectangle
in the frame's pixels.  What they must be is worked out here in Python integers: the region's blocks are those of a frame of
the region's size (adaptive_model.blocks_of), moved to the region's origin; the predicate holds exactly when every one of
them is also a block of the whole frame.  Also here: render_tiled(adaptive=...) refuses, before it needs a device, a tile that
is no multiple of the block."""
import os
import subprocess

import pytest

import adaptive_model as M
import scenes
from crucible_amd.renderer import Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 61, 45
# (x0, y0, w, h): unaligned; aligned interior; aligned up to the frame's right and bottom edge; the whole frame; origin aligned
# but the right / the bottom edge inside a block; an unaligned origin with aligned edges; one pixel; a region inside one block;
# right edge on the frame's edge only
REGIONS = [(5, 3, 43, 37), (16, 16, 32, 16), (48, 32, 13, 13), (0, 0, 61, 45), (16, 16, 20, 16), (16, 16, 32, 10), (8, 4, 24, 12),
           (60, 44, 1, 1), (17, 17, 5, 5), (32, 0, 29, 32), (0, 32, 32, 13), (0, 0, 32, 32), (32, 32, 29, 13), (32, 32, 28, 13)]
BLOCKS = [3, 4, 5]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("adaptive_region_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"adaptive_region_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "adaptive_region_check.cpp")])
        built.append(exe)
    return built


def run(exes, *args):
    outs = []
    for exe in exes:
        res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    rows = [[int(x) for x in line.split()] for line in outs[0].splitlines()]
    return rows[0], rows[1:]


@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("L", BLOCKS)
def test_region_blocks_and_the_predicate(exes, region, L):
    x0, y0, w, h = region
    B = 1 << L
    (aligned, bx_n, by_n), rows = run(exes, W, H, x0, y0, w, h, L)
    local = M.blocks_of(w, h, B)   # the region as if it were the frame
    assert (bx_n, by_n) == (-(-w // B), -(-h // B)) and len(rows) == len(local) == bx_n * by_n
    frame_blocks = M.blocks_of(W, H, B)
    want_rects = [(x0 + bx, y0 + by, bw, bh) for bx, by, bw, bh in local]
    want_aligned = all(r in frame_blocks for r in want_rects)
    assert aligned == int(want_aligned)
    # the rule as the documents state it
    assert want_aligned == (x0 % B == 0 and y0 % B == 0 and ((x0 + w) % B == 0 or x0 + w == W) and ((y0 + h) % B == 0 or y0 + h == H))
    covered = 0
    for b, (bb, rx, ry, bw, bh, fb) in enumerate(rows):
        assert bb == b and (rx, ry, bw, bh) == want_rects[b]
        assert x0 <= rx and rx + bw <= x0 + w and y0 <= ry and ry + bh <= y0 + h   # N_b counts pixels inside the region only
        assert fb == (frame_blocks.index(want_rects[b]) if want_aligned else -1)
        covered += bw * bh
    assert covered == w * h


def test_the_cases_cover_every_kind():
    kinds = set()
    for x0, y0, w, h in REGIONS:
        for L in BLOCKS:
            B = 1 << L
            kinds.add((x0 % B == 0 and y0 % B == 0, (x0 + w) % B == 0, x0 + w == W, (y0 + h) % B == 0, y0 + h == H, w % B != 0 or h % B != 0))
    assert any(k[0] and k[1] and k[3] for k in kinds)                # aligned, interior
    assert any(k[0] and k[2] and k[4] and k[5] for k in kinds)       # aligned up to the frame's edges, with partial blocks
    assert any(k[0] and not k[1] and not k[2] for k in kinds)        # right edge inside a block
    assert any(k[0] and not k[3] and not k[4] for k in kinds)        # bottom edge inside a block
    assert any(not k[0] and k[1] and k[3] for k in kinds)            # only the origin is off
    assert W % 32 and H % 32 and W % 8 and H % 8


@pytest.mark.parametrize("tile,block", [((24, 16), 16), ((16, 24), 16), ((32, 36), 8), ((20, 20), None), ((48, 48), 32)])
def test_render_tiled_refuses_a_tile_that_is_no_multiple_of_the_block(tile, block):
    """Before anything needs a device: the object below has no handle at all."""
    r = Renderer.__new__(Renderer)
    sc = scenes.mixed_scene()
    adaptive = dict(tolerance=0.01, min_samples=8, pass_samples=2)
    if block is not None:
        adaptive["block"] = block   # (None: the default, 16)
    with pytest.raises(ValueError, match="multiples of the block"):
        r.render_tiled(sc.scene_cam, tile, seed=1, adaptive=adaptive)
