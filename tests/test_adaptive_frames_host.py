"""The batch functions of crucible_amd/csrc/adaptive.hpp (cr_render_adaptive_frames_*), checked without a device:
tests/adaptive_frames_check.cpp compiles the header with g++ (plain, and with -fsanitize=address,undefined) and prints, per
global block of a batch, the frame and the block it is, its rectangle and its tiles as batch-wide tile numbers.  What they
must be is worked out here in Python integers: global block g is block g % n_blocks of frame g // n_blocks; tile (tx, ty) of
frame f is number (f * tiles_y + ty) * tiles_x + tx; a block's tiles are those whose pixels lie in the block; and the tiles of
all blocks of all frames partition [0, n_frames * tiles_x * tiles_y)."""
import os
import subprocess

import pytest

import adaptive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 29), (47, 37)]
TILES = [(2, 2), (1, 1), (3, 3)]   # log2 of the tile's sides: 4x4, 2x2, 8x8
BLOCKS = [3, 4, 5]
FRAMES = [1, 2, 5]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("adaptive_frames_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"adaptive_frames_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "adaptive_frames_check.cpp")])
        built.append(exe)
    return built


def run(exes, *args):
    outs = []
    for exe in exes:
        res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    rows = []
    for line in outs[0].splitlines():
        head, tiles = line.split(":")
        rows.append(([int(x) for x in head.split()], [int(x) for x in tiles.split()]))
    return rows


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("lw,lh", TILES)
@pytest.mark.parametrize("n_frames", FRAMES)
def test_blocks_and_tiles_of_a_batch(exes, W, H, lw, lh, n_frames):
    for L in BLOCKS:
        if lw > L or lh > L:
            continue   # (the library renders such a block on the default tile: tiles must divide blocks)
        rects = M.blocks_of(W, H, 1 << L)
        tiles_x, tiles_y = -(-W // (1 << lw)), -(-H // (1 << lh))
        rows = run(exes, W, H, L, lw, lh, n_frames)
        assert len(rows) == n_frames * len(rects)
        seen = []
        for g, ((gg, f, b, x0, y0, bw, bh), tiles) in enumerate(rows):
            assert gg == g and (f, b) == divmod(g, len(rects)) and f < n_frames
            assert (x0, y0, bw, bh) == rects[b]
            # the tiles whose first pixel lies in the block, row by row, in frame f's rows of the batch's tile grid
            want = [(f * tiles_y + ty) * tiles_x + tx
                    for ty in range(tiles_y) if y0 <= ty << lh < y0 + (1 << L)
                    for tx in range(tiles_x) if x0 <= tx << lw < x0 + (1 << L)]
            assert tiles == want and len(want) > 0, (g, tiles, want)
            assert all(f * tiles_x * tiles_y <= t < (f + 1) * tiles_x * tiles_y for t in tiles)
            seen += tiles
        assert sorted(seen) == list(range(n_frames * tiles_x * tiles_y))   # a partition: every tile of every frame once


def test_the_cases_cover_partial_blocks_and_tiles():
    """The sizes are no multiple of any tile or block side, so every grid has partial edge tiles and partial edge blocks."""
    for W, H in SIZES:
        for side in (2, 4, 8, 16, 32):
            assert W % side and H % side
