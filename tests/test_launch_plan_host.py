"""crucible_amd/csrc/launch_plan.hpp, the arithmetic that cuts a render (render.hpp launch()) and a guide pass
(aov_kernel.hpp aov_launch()) into kernel launches, checked without a device: tests/launch_plan_check.cpp compiles the
header with g++ (plain, and with -fsanitize=address,undefined) and prints the plan of each case.  With relaxed sums no
frame shows a wrong chunk, grid or frames-per-launch -- it costs speed, not pixels --, so the numbers are pinned here.  The
expectations are written out by hand from the rule, with the sum in a comment, not computed by a second
copy of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL, LDS, TOP = 0, 1, 2
INT32_MAX = 2147483647
COUNTER = 0xF0000000        # the handle's work_counter_max: 4026531840
BUF = 40 << 30              # ... and its sample_buf_limit


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("launch_plan_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"launch_plan_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "launch_plan_check.cpp")])
        built.append(exe)
    return built


def check(exes, tmp_path, cases):
    """cases: (name, the case's line, the expected numbers); both builds print them."""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in cases))
    outs = []
    for exe in exes:
        res = subprocess.run([exe, path], capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    got = [tuple(int(x) for x in line.split()) for line in outs[0].splitlines()]
    assert len(got) == len(cases)
    for (name, _, want), g in zip(cases, got):
        assert g == tuple(want), (name, g, want)


def test_chunk_and_tile(exes, tmp_path):
    check(exes, tmp_path, [
        ("the override wins, rounded to whole rounds", "C 1000000 256 256 100", (128,)),
        ("the override wins over the clamp", "C 1000000 256 256 4096", (4096,)),
        ("lower clamp: 6400 items over 40 waves, 160 / 128 = 1", "C 6400 10 256 0", (64,)),
        ("upper clamp: 2^30 items over 4096 waves, 262144 / 128 = 2048", "C 1073741824 256 1024 0", (1024,)),
        ("just inside: 131072 items over one wave, 1024", "C 131072 1 64 0", (1024,)),
        ("rounding: 51200 items over 4 waves, 12800 / 128 = 100", "C 51200 1 256 0", (128,)),
        ("a multiple of 64 stays: 24576 / 128 = 192", "C 24576 1 64 0", (192,)),
        ("grid * block < 64 counts as one wave: 25600 / 128 = 200", "C 25600 1 32 0", (256,)),
        ("no work", "C 0 1 256 0", (64,)),
        ("1 sample: 8 x 8", "T 1", (3, 3)),
        ("2 samples: 8 x 4", "T 2", (3, 2)),
        ("3 samples: 8 x 4", "T 3", (3, 2)),
        ("4 samples: 4 x 4", "T 4", (2, 2)),
        ("many samples: 4 x 4", "T 2147483647", (2, 2)),
    ])


def test_fx_scale(exes, tmp_path):
    """S = min(52, 62 - floor(log2 n)): n * 2^S < 2^63."""
    check(exes, tmp_path, [
        ("1 sample", "X 1", (52,)),
        ("512 samples", "X 512", (52,)),
        ("2047 = 2^11 - 1: 62 - 10", "X 2047", (52,)),
        ("2048: 62 - 11", "X 2048", (51,)),
        ("INT32_MAX: 62 - 30", "X 2147483647", (32,)),
    ])


def P(n_samples, tile=(-1, -1), block_log2=-1, relax=1, res=LDS, scene=1000, max_block=1024, block=256):
    return f"P {tile[0]} {tile[1]} {n_samples} {block_log2} {relax} {res} {scene} {max_block} {block}"


def test_tile_and_lds(exes, tmp_path):
    """(lw, lh, fx_off, lds_base, lds_per_wave, use_lds, bytes(max_block), bytes(block)).  A wave's two slots of 3 words per pixel:
    2 * 3 * 8 B = 48 B per pixel -- 3072 B for 8 x 8, 1536 B for 8 x 4, 768 B for 4 x 4; max_block 1024 is 16 waves, block 256
    is 4.  The scene's 1000 B end at 1008."""
    check(exes, tmp_path, [
        ("1 sample: 8 x 8; 1008 + 16 * 3072, 1008 + 4 * 3072", P(1), (3, 3, 1008, 1008, 3072, 1, 50160, 13296)),
        ("2 samples: 8 x 4; 1008 + 24576, 1008 + 6144", P(2), (3, 2, 1008, 1008, 1536, 1, 25584, 7152)),
        ("3 samples: 8 x 4", P(3), (3, 2, 1008, 1008, 1536, 1, 25584, 7152)),
        ("4 samples: 4 x 4; 1008 + 12288, 1008 + 3072", P(4), (2, 2, 1008, 1008, 768, 1, 13296, 4080)),
        ("INT32_MAX samples: 4 x 4", P(INT32_MAX), (2, 2, 1008, 1008, 768, 1, 13296, 4080)),
        ("the handle's 2 x 2 is kept at 1 sample: 4 * 48 = 192 B per wave", P(1, tile=(1, 1)), (1, 1, 1008, 1008, 192, 1, 4080, 1776)),
        ("the handle's 8 x 4 is kept at 512 samples", P(512, tile=(3, 2)), (3, 2, 1008, 1008, 1536, 1, 25584, 7152)),
        ("adaptive, 4 x 4 blocks: the handle's 8 x 8 is re-defaulted by the pass's 8 samples", P(8, tile=(3, 3), block_log2=2), (2, 2, 1008, 1008, 768, 1, 13296, 4080)),
        ("adaptive, 4 x 4 blocks: one side above is enough, both go", P(1, tile=(3, 1), block_log2=2), (3, 3, 1008, 1008, 3072, 1, 50160, 13296)),
        ("adaptive, 4 x 4 blocks: the handle's 4 x 2 divides them and stays: 8 * 48 = 384", P(8, tile=(2, 1), block_log2=2), (2, 1, 1008, 1008, 384, 1, 7152, 2544)),
        ("adaptive, 8 x 8 blocks: the handle's 8 x 8 stays", P(8, tile=(3, 3), block_log2=3), (3, 3, 1008, 1008, 3072, 1, 50160, 13296)),
        # 160 KB = 163840; 1024 threads of 8 x 8 tiles need 16 * 3072 = 49152 B of slots: fx_off may be 114688
        ("160 KB: fx_off 114688 stays at 8 x 8; 114688 + 49152 = 163840", P(1, scene=114688), (3, 3, 114688, 114688, 3072, 1, 163840, 126976)),
        ("160 KB: fx_off 114704 falls to 4 x 4 with 12288 B", P(1, scene=114689), (2, 2, 114704, 114704, 768, 1, 126992, 117776)),
        ("the 6-waves-per-SIMD entry point's 512 threads: 139264 + 8 * 3072 = 163840 stays", P(1, scene=139264, max_block=512), (3, 3, 139264, 139264, 3072, 1, 163840, 151552)),
        # (the known weakness: the fallback is taken whenever the tile asked for does not fit, and is not measured itself --
        # pick_block refuses such a launch afterwards; today's answer, 160000 + 12288 > 163840)
        ("160 KB: the 4 x 4 fallback is not measured again", P(4, scene=160000), (2, 2, 160000, 160000, 768, 1, 172288, 163072)),
        ("RES_GLOBAL: no scene in LDS, the slots at 0", P(4, res=GLOBAL, scene=5000), (2, 2, 0, 0, 768, 1, 12288, 3072)),
        ("RES_TOP: behind the window", P(4, res=TOP, scene=131072), (2, 2, 131072, 131072, 768, 1, 143360, 134144)),
        # the reference order keeps no slots: a block takes the scene's bytes, as they are
        ("reference order, scene in LDS", P(4, relax=0), (2, 2, 1008, 1000, 0, 1, 1000, 1000)),
        ("reference order, 1 sample: the tile all the same", P(1, relax=0), (3, 3, 1008, 1000, 0, 1, 1000, 1000)),
        ("reference order, RES_GLOBAL: no dynamic LDS", P(4, relax=0, res=GLOBAL, scene=0), (2, 2, 0, 0, 0, 0, 0, 0)),
    ])


def test_call_shapes(exes, tmp_path):
    """K relax keyed latency list n_frames whole adaptive -> 0 ok, 1 one frame per launch, 2 whole frames, 3 no tile list."""
    check(exes, tmp_path, [
        ("a frame on a relaxed kernel with keys", "K 1 1 0 0 1 1 0", (0,)),
        ("a frame on a static kernel", "K 1 0 0 0 1 1 0", (0,)),
        ("a frame in the reference order", "K 0 0 0 0 1 1 0", (0,)),
        ("a batch on a static kernel", "K 1 0 0 0 3 1 0", (1,)),
        ("a batch in the reference order", "K 0 1 0 0 3 1 0", (1,)),
        ("a batch on a relaxed kernel with keys", "K 1 1 0 0 3 1 0", (0,)),
        ("a region on a relaxed kernel with keys", "K 1 1 0 0 1 0 0", (0,)),
        ("a region on a static kernel", "K 1 0 0 0 1 0 0", (2,)),
        ("a region on the 6-waves-per-SIMD entry point", "K 1 1 1 0 1 0 0", (2,)),
        ("a region in the reference order", "K 0 1 0 0 1 0 0", (2,)),
        ("an adaptive run on a kernel without the list", "K 1 1 0 0 1 1 1", (3,)),
        ("a listed kernel outside an adaptive run", "K 1 1 0 1 1 1 0", (3,)),
        ("an adaptive run on a listed kernel", "K 1 1 0 1 1 1 1", (0,)),
        ("an adaptive batch of regions on a listed kernel", "K 1 1 0 1 3 0 1", (0,)),
        ("the order: one frame per launch first", "K 1 0 0 0 3 0 1", (1,)),
        ("the order: whole frames before the list", "K 1 0 0 1 1 0 0", (2,)),
    ])


QUERY = "relax sample_granular s_begin s_end reg_w reg_h real_bytes sample_buf_limit work_counter_max lw lh tile_fixed n_frames adaptive split_passes fixed_sums px_tiles_x px_tiles_y".split()


def Q(samples, size, px_tiles, **kw):
    """The query of samples [s_begin, s_end) of a size[0] x size[1] launch; px_tiles: the frame's 8 x 8 tiles, as prepare_args hands them over."""
    q = dict(relax=1, sample_granular=1, s_begin=samples[0], s_end=samples[1], reg_w=size[0], reg_h=size[1], real_bytes=8, sample_buf_limit=BUF,
             work_counter_max=COUNTER, lw=2, lh=2, tile_fixed=0, n_frames=1, adaptive=0, split_passes=0, fixed_sums=0, px_tiles_x=px_tiles[0], px_tiles_y=px_tiles[1])
    q.update(kw)
    assert sorted(q) == sorted(QUERY)
    return " ".join(str(int(q[k])) for k in QUERY)


def S(*a, alloc_fails=0, **kw):
    return "S " + Q(*a, **kw) + f" {alloc_fails}"


def B(*a, n_cus=256, per_cu=1, block=256, chunk_override=0, **kw):
    return "B " + Q(*a, **kw) + f" {n_cus} {per_cu} {block} {chunk_override}"


OK, COUNTER_FULL, COUNTER_FULL_PASS = 0, 1, 2
HEADLINE = ((0, 512), (1920, 1080), (240, 135))
SMALL = ((0, 100), (64, 64), (8, 8))
MOVIE = ((0, 8), (16, 16), (2, 2))


def test_relaxed_sample_plan(exes, tmp_path):
    """(refusal, tiled, batch, lw, lh, tiles_x, tiles_y, ns, fpl, fx_acc_bytes, sample_buf_bytes, sg_acc_bytes).  A group is 64 work
    items of a tile; max_groups = work_counter_max / (tiles * 64)."""
    check(exes, tmp_path, [
        # 480 x 270 = 129600 tiles, x 64 = 8294400; 4026531840 / 8294400 = 485.4; 485 * 4 = 1940 samples; 512 samples are 128
        # groups, 485 / 128 = 3 frames, of 1; sums: 1920 * 1080 * 3 * 8 B
        ("the headline: max_groups 485", S(*HEADLINE), (OK, 1, 512, 2, 2, 480, 270, 4, 1, 49766400, 0, 0)),
        # 16 x 16 = 256 tiles, x 64 = 16384; 100000 / 16384 = 6.1; 6 * 4 = 24 samples; sums 64 * 64 * 24 B
        ("64 x 64 @ 100 at a counter of 100000: max_groups 6, batch 24", S(*SMALL, work_counter_max=100000), (OK, 1, 24, 2, 2, 16, 16, 4, 1, 98304, 0, 0)),
        # 4 x 4 = 16 tiles, x 64 = 1024; 4096 / 1024 = 4 groups; 8 samples are 2: two frames; sums 10 * 256 * 24 B
        ("16 x 16 @ 8, 10 frames at a counter of 4096: two frames per launch", S(*MOVIE, n_frames=10, work_counter_max=4096), (OK, 1, 8, 2, 2, 4, 4, 4, 2, 61440, 0, 0)),
        ("... at the default counter: all ten; 3932160 groups", S(*MOVIE, n_frames=10), (OK, 1, 8, 2, 2, 4, 4, 4, 10, 61440, 0, 0)),
        # 4 groups hold 16 samples of a frame: 12 samples are 3 groups, 4 / 3 = 1 frame
        ("... 12 samples: one frame per launch", S((0, 12), (16, 16), (2, 2), n_frames=10, work_counter_max=4096), (OK, 1, 12, 2, 2, 4, 4, 4, 1, 61440, 0, 0)),
        ("... 20 samples: a frame in batches of 16 renders frame by frame", S((0, 20), (16, 16), (2, 2), n_frames=10, work_counter_max=4096), (OK, 1, 16, 2, 2, 4, 4, 4, 1, 61440, 0, 0)),
        # 2 x 2 tiles x 64 = 256 > 64
        ("a counter of 64 and a frame of 2 x 2 tiles: refused", S((0, 4), (8, 8), (1, 1), work_counter_max=64), (COUNTER_FULL, 1, 0, 2, 2, 2, 2, 4, 1, 0, 0, 0)),
        ("an adaptive pass of 100 at a batch of 24: refused", S(*SMALL, work_counter_max=100000, adaptive=1), (COUNTER_FULL_PASS, 1, 24, 2, 2, 16, 16, 4, 1, 0, 0, 0)),
        ("... split with split_passes; the pass loop keeps its own sums", S(*SMALL, work_counter_max=100000, adaptive=1, split_passes=1), (OK, 1, 24, 2, 2, 16, 16, 4, 1, 0, 0, 0)),
        ("an adaptive pass that fits", S(*MOVIE, adaptive=1), (OK, 1, 8, 2, 2, 4, 4, 4, 1, 0, 0, 0)),
        ("fixed sums go into the caller's buffer", S(*MOVIE, fixed_sums=1), (OK, 1, 8, 2, 2, 4, 4, 4, 1, 0, 0, 0)),
        ("CRUCIBLE_SAMPLE_GRANULAR=0 does not reach the relaxed kernels", S(*MOVIE, sample_granular=0), (OK, 1, 8, 2, 2, 4, 4, 4, 1, 6144, 0, 0)),
        ("f32 sums are 64-bit words too", S(*MOVIE, real_bytes=4), (OK, 1, 8, 2, 2, 4, 4, 4, 1, 6144, 0, 0)),
        ("no samples: the arguments stay", S((5, 5), (16, 16), (2, 2)), (OK, 0, 0, 2, 2, 2, 2, 1, 1, 0, 0, 0)),
        # 3 samples on 8 x 4 tiles of 2 samples: 2 x 4 = 8 tiles x 64 = 512: one group, 2 samples
        ("the last samples of the range", S((INT32_MAX - 3, INT32_MAX), (16, 16), (2, 2), lw=3, lh=2, work_counter_max=512), (OK, 1, 2, 3, 2, 2, 4, 2, 1, 6144, 0, 0)),
        # a region of 33 x 17 in a larger frame: 9 x 5 tiles, the frame's own 8 x 8 tiles are not the plan's
        ("a region", S((0, 9), (33, 17), (240, 135)), (OK, 1, 9, 2, 2, 9, 5, 4, 1, 13464, 0, 0)),
    ])


def test_launches(exes, tmp_path):
    """(grid, n_threads, launches), then per launch (f0, fn, b0, b1, groups, sg_total, blocks, chunk): launch()'s loops over the plan."""
    batch24 = (0, 1, 0, 24, 6, 98304, 384, 64)
    check(exes, tmp_path, [
        # 129600 tiles x 128 groups x 64 = 1061683200 items; 4096 waves take 259200 each, / 128 = 2025: the chunk's 1024
        ("the headline: one launch of 128 groups", B(*HEADLINE, block=1024), (256, 262144, 1, 0, 1, 0, 512, 128, 1061683200, 256, 1024)),
        # 256 tiles x 6 groups x 64 = 98304 items = 384 blocks of 256, of 512; 1536 waves take 64 each: the chunk's floor.
        # The last launch: 4 samples are 1 group, 16384 items, on the whole grid
        ("64 x 64 @ 100 in batches of 24: five launches", B(*SMALL, work_counter_max=100000, per_cu=2),
         (384, 98304, 5) + batch24 + (0, 1, 24, 48) + batch24[4:] + (0, 1, 48, 72) + batch24[4:] + (0, 1, 72, 96) + batch24[4:] + (0, 1, 96, 100, 1, 16384, 384, 64)),
        # 16 tiles x 2 frames x 2 groups x 64 = 4096 items = 16 blocks
        ("ten frames, two per launch: five launches", B(*MOVIE, n_frames=10, work_counter_max=4096),
         (16, 4096, 5, 0, 2, 0, 8, 2, 4096, 16, 64, 2, 2, 0, 8, 2, 4096, 16, 64, 4, 2, 0, 8, 2, 4096, 16, 64, 6, 2, 0, 8, 2, 4096, 16, 64, 8, 2, 0, 8, 2, 4096, 16, 64)),
        # 16 tiles x 64 = 1024, 3072 / 1024 = 3 groups; 4 samples are 1: three frames, 3072 items = 12 blocks; the last frame's 1024 on the whole grid
        ("ten frames of 4 samples, three per launch: the last launch has one", B((0, 4), (16, 16), (2, 2), n_frames=10, work_counter_max=3072),
         (12, 3072, 4, 0, 3, 0, 4, 1, 3072, 12, 64, 3, 3, 0, 4, 1, 3072, 12, 64, 6, 3, 0, 4, 1, 3072, 12, 64, 9, 1, 0, 4, 1, 1024, 12, 64)),
        # the loop's bound is 64 bits wide: 2147483646 + 2 is past INT32_MAX.  8 tiles x 1 group x 64 = 512 items = 8 blocks of 64, of 4
        ("the last samples of the range: two launches, no wrap", B((INT32_MAX - 3, INT32_MAX), (16, 16), (2, 2), lw=3, lh=2, work_counter_max=512, n_cus=4, block=64),
         (4, 256, 2, 0, 1, 2147483644, 2147483646, 1, 512, 4, 64, 0, 1, 2147483646, 2147483647, 1, 512, 4, 64)),
        # reference order, 64 x 64 f32 @ 14 in batches of 6 (test_reference_order_sample_plan): 256 tiles x 2 groups x 64 = 32768 items = 128 blocks
        ("reference order: batches of 6, the last of 2", B((0, 14), (64, 64), (8, 8), relax=0, real_bytes=4, sample_buf_limit=491520),
         (128, 32768, 3, 0, 1, 0, 6, 2, 32768, 128, 64, 0, 1, 6, 12, 2, 32768, 128, 64, 0, 1, 12, 14, 1, 16384, 128, 64)),
    ])


def test_reference_order_sample_plan(exes, tmp_path):
    """The colour buffer holds one colour per work item of a batch.  64 x 64 in f32: a sample of the frame is 4096 * 12 = 49152 B;
    on 4 x 4 tiles a group of 4 samples is 256 tiles * 64 * 12 = 196608 B."""
    ref = dict(relax=0, real_bytes=4)
    check(exes, tmp_path, [
        ("all 4 samples fit: no running sums", S((0, 4), (64, 64), (8, 8), **ref), (OK, 1, 4, 2, 2, 16, 16, 4, 1, 0, 196608, 0)),
        ("a limit of 12 samples cuts the batch: 3 groups, 589824 B", S(*SMALL, sample_buf_limit=589824, **ref), (OK, 1, 12, 2, 2, 16, 16, 4, 1, 0, 589824, 49152)),
        # 491520 / 49152 = 10 samples, which are 3 groups with the padding: 589824 > 491520, so 10 - 4 = 6 samples, 2 groups
        ("a limit of 10 samples: shrunk by a whole group to 6", S(*SMALL, sample_buf_limit=491520, **ref), (OK, 1, 6, 2, 2, 16, 16, 4, 1, 0, 393216, 49152)),
        # 2 samples: 8 x 4 tiles, 8 x 16 = 128 of them, one group of 2 samples: 128 * 64 * 12 B
        ("a limit of 2 samples: the batch re-defaults the tile to 8 x 4", S(*SMALL, sample_buf_limit=98304, **ref), (OK, 1, 2, 3, 2, 8, 16, 2, 1, 0, 98304, 49152)),
        # never below one group: 196608 > 98304 all the same
        ("... on a tile the handle fixed: one group's bytes are taken", S(*SMALL, sample_buf_limit=98304, tile_fixed=1, **ref), (OK, 1, 2, 2, 2, 16, 16, 4, 1, 0, 196608, 49152)),
        # one sample: an 8 x 8 tile, 8 x 8 = 64 tiles * 64 * 12 B
        ("a limit of 0: one sample, and the batch re-defaults the tile to 8 x 8", S(*SMALL, sample_buf_limit=0, **ref), (OK, 1, 1, 3, 3, 8, 8, 1, 1, 0, 49152, 49152)),
        ("... not a tile the handle fixed: a group's bytes for one sample", S(*SMALL, sample_buf_limit=0, tile_fixed=1, **ref), (OK, 1, 1, 2, 2, 16, 16, 4, 1, 0, 196608, 49152)),
        ("the counter cuts as well: 6 groups", S(*SMALL, work_counter_max=100000, **ref), (OK, 1, 24, 2, 2, 16, 16, 4, 1, 0, 1179648, 49152)),
        # 256 tiles x 64 = 16384 > 64: a lane owns a pixel, on the frame's 8 x 8 tiles
        ("max_groups < 1: a lane owns a pixel", S(*SMALL, work_counter_max=64, **ref), (OK, 1, 0, 2, 2, 8, 8, 1, 1, 0, 0, 0)),
        ("a buffer that cannot be had: the same plan", S(*SMALL, sample_buf_limit=491520, alloc_fails=1, **ref), (OK, 1, 0, 2, 2, 8, 8, 1, 1, 0, 0, 0)),
        ("CRUCIBLE_SAMPLE_GRANULAR=0: the arguments stay", S(*SMALL, sample_granular=0, **ref), (OK, 0, 0, 2, 2, 8, 8, 1, 1, 0, 0, 0)),
        # f64, 33 x 17: 9 x 5 = 45 tiles, 9 samples are 3 groups: 45 * 3 * 64 * 24 B
        ("f64, an odd frame: edge padding included", S((0, 9), (33, 17), (5, 3), relax=0), (OK, 1, 9, 2, 2, 9, 5, 4, 1, 0, 207360, 0)),
    ])


def test_grid_and_batch(exes, tmp_path):
    check(exes, tmp_path, [
        # G n_cus per_cu work block lanes_per_item -> (blocks, n_threads)
        ("more work than the device holds", "G 256 1 1061683200 1024 1", (256, 262144)),
        ("a clamp to the blocks needed: 98304 / 256 = 384 of 512", "G 256 2 98304 256 1", (384, 98304)),
        ("one item over a block: 257 items are 2 blocks", "G 256 2 257 256 1", (2, 512)),
        ("one item", "G 256 1 1 256 1", (1, 256)),
        ("no work: one block all the same", "G 256 1 0 256 1", (1, 256)),
        ("the guide pass: a unit per wave, 10 units are 3 blocks of 4 waves", "G 256 2 10 256 64", (3, 768)),
        ("the guide pass: the whole device", "G 256 2 100000 256 64", (512, 131072)),
        # F ns n_samples n_tiles fit grid block chunk_override -> (groups, sg_total, blocks, chunk)
        # 3 tiles x 2 groups x 64 = 384 items are 2 blocks
        ("a pass of 3 tiles fits 2 blocks", "F 4 8 3 1 512 256 0", (2, 384, 2, 64)),
        ("... a render's batch takes the whole grid", "F 4 8 3 0 512 256 0", (2, 384, 512, 64)),
        ("a pass of no tiles: one block", "F 4 8 0 1 512 256 0", (2, 0, 1, 64)),
        # 100000 tiles x 64 = 6400000 items are 25000 blocks; 2048 waves take 3125, / 128 = 24
        ("a pass of many tiles: the grid", "F 4 4 100000 1 512 256 0", (1, 6400000, 512, 64)),
        # 129600 tiles x 128 groups x 64 on 256 blocks of 1024
        ("the headline's chunk", "F 4 512 129600 0 256 1024 0", (128, 1061683200, 256, 1024)),
        ("3 samples of 1 per group, CRUCIBLE_SG_CHUNK=100", "F 1 3 10 0 8 64 100", (3, 1920, 8, 128)),
        ("5 samples of 4 per group are 2 groups", "F 4 5 1 0 8 64 0", (2, 128, 8, 64)),
    ])


def U(tiles, groups, frames=None, n_cus=4, per_cu=2, block=256, counter=COUNTER):
    """frames: a batch's (the BATCH kernels); None: the single-frame kernels, whose n_frames is 0.  4 CUs x 2 blocks x 4 waves = 32 resident waves."""
    return f"U {tiles[0]} {tiles[1]} {groups} {0 if frames is None else 1} {frames or 0} {n_cus} {per_cu} {block} {counter}"


def test_guide_units(exes, tmp_path):
    """(unit_groups, unit_chunks, frame_tiles, frame_units, frames_per_launch, launches, units of the last launch)."""
    check(exes, tmp_path, [
        # 64 tiles x 64 groups / (8 x 32 waves) = 16 groups per unit, 4 units per tile
        ("eight units per resident wave", U((8, 8), 64), (16, 4, 64, 256, 1, 1, 256)),
        ("never more than the groups there are: 512 x 8 / 256 = 16 of 8", U((32, 16), 8), (8, 1, 512, 512, 1, 1, 512)),
        # 256 CUs x 2 x 4 = 2048 waves: 45 x 3 / 16384 = 0
        ("at least one group: a small frame on a large device", U((9, 5), 3, n_cus=256), (1, 3, 45, 135, 1, 1, 135)),
        ("a batch counts the units of all its frames: 2 x 64 x 64 / 256 = 32", U((8, 8), 64, frames=2), (32, 2, 64, 128, 2, 1, 256)),
        ("a batch of one is sized as the frame", U((8, 8), 64, frames=1), (16, 4, 64, 256, 1, 1, 256)),
        # 64 x 4 = 256 units > 130: 130 / 64 = 2 units per tile, 64 / 2 = 32 groups each
        ("the cap recomputes the unit", U((8, 8), 64, frames=1, counter=130), (32, 2, 64, 128, 1, 1, 128)),
        ("two frames of 128 units under a cap of 200: frame by frame", U((8, 8), 64, frames=2, counter=200), (32, 2, 64, 128, 1, 2, 128)),
        ("... of 256: both", U((8, 8), 64, frames=2, counter=256), (32, 2, 64, 128, 2, 1, 256)),
        # 3 x 64 x 64 / 256 = 48 groups, ceil(64 / 48) = 2 units per tile
        ("three frames under a cap of 256: two, then one", U((8, 8), 64, frames=3, counter=256), (48, 2, 64, 128, 2, 2, 128)),
        # 3 x 64 x 64 / 256 = 48 groups, 2 units per tile = 128 > 64: one unit per tile
        ("a counter below a frame's tiles is raised to them", U((8, 8), 64, frames=3, counter=10), (64, 1, 64, 64, 1, 3, 64)),
        # the smallest count above the finalize kernel's 65535-row grid: the plan does not care
        ("70000 frames of one unit: one launch", U((1, 1), 1, frames=70000), (1, 1, 1, 1, 70000, 1, 70000)),
        ("the single-frame kernels do not ask the handle's counter", U((8, 8), 64, counter=64), (16, 4, 64, 256, 1, 1, 256)),
        # 2^22 tiles x 4096 groups on 2^16 x 2^10 x 16 = 2^30 waves: 2^34 / 2^33 = 2 groups, 2048 units per tile = 2^33 > 0xF0000000;
        # 4026531840 / 4194304 = 960 units per tile, ceil(4096 / 960) = 5 groups, ceil(4096 / 5) = 820 units, x 2^22
        ("the single-frame kernels' own cap, 0xF0000000", U((2048, 2048), 4096, n_cus=65536, per_cu=1024, block=1024), (5, 820, 4194304, 3439329280, 1, 1, 3439329280)),
    ])
