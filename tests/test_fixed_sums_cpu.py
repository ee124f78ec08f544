"""CR_OUTPUT_FIXED_SUM without a GPU: the torch.distributed reduce of the fixed-point words (reduce_fixed_sums, gloo
worlds 2 and 3) equals the header's combine rule c = ((a & M) + (b & M)) | ((a | b) & F) evaluated in numpy uint64 --
flags in some words and some ranks only, magnitudes that total exactly 2^63 - 1 -- and the output_sum values of
include/crucible_hip.h match the ctypes mirror."""
import os
import re
import socket
import sys

import numpy as np
import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crucible_hip.h")
F = np.uint64(1 << 63)
M = np.uint64((1 << 63) - 1)
N_WORDS = 64


def combine(a, b):
    """The header's rule for two sets of CR_OUTPUT_FIXED_SUM words."""
    return ((a & M) + (b & M)) | ((a | b) & F)


def rank_words(rank, world):
    """Synthetic words of one rank: magnitudes whose totals over the ranks reach 2^63 - 1 in some words, NaN flags in
    some words of some ranks (word 2: every rank, word 3: the last rank only, word 4: no rank)."""
    rng = np.random.default_rng(1000 * world + rank)
    mag = rng.integers(0, (1 << 63) // (2 * world), size=N_WORDS, dtype=np.uint64)
    top = (1 << 63) - 1
    share = top // world
    mag[0] = share + (top - share * world if rank == world - 1 else 0)   # totals 2^63 - 1 exactly
    mag[1] = top if rank == 0 else 0                                      # one rank holds all of it
    mag[4] = 0
    words = mag.copy()
    words[2] |= F
    if rank == world - 1:
        words[3] |= F
    words[5 + rank] |= F                                                  # a flag of one rank per word
    return words


def expected(world):
    acc = rank_words(0, world)
    for r in range(1, world):
        acc = combine(acc, rank_words(r, world))
    return acc


def test_combine_rule_never_carries_into_the_flag():
    for world in (2, 3):
        e = expected(world)
        assert e[0] == M and e[1] == M          # the largest total of one frame's magnitudes
        assert e[2] & F and e[3] & F and not e[4] & F
        assert all(e[5 + r] & F for r in range(world))
        total = sum(int(rank_words(r, world)[9] & M) for r in range(world))
        assert int(e[9]) == total and total < 1 << 63


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from crucible_amd.distributed import reduce_fixed_sums
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = torch.from_numpy(rank_words(rank, world).view(np.int64).copy())
        out = reduce_fixed_sums(t, dst=0)
        assert out is t
        if rank == 0:
            np.save(out_path, t.numpy().view(np.uint64))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_reduce_fixed_sums_matches_the_combine_rule(tmp_path, world):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "words.npy")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    got = np.load(out)
    assert got.dtype == np.uint64 and np.array_equal(got, expected(world))


def test_reduce_fixed_sums_without_process_group():
    import torch
    from crucible_amd.distributed import reduce_fixed_sums
    words = rank_words(0, 2)
    t = torch.from_numpy(words.view(np.int64).copy())
    assert np.array_equal(reduce_fixed_sums(t).numpy().view(np.uint64), words)


def test_output_sum_values_match_the_header():
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*CR_OUTPUT_FIXED_SUM\s*=\s*(\d+)\s*\}", text)
    assert m and int(m.group(1)) == A.CR_OUTPUT_FIXED_SUM == 2
    assert int(re.search(r"#define CR_ABI_VERSION (\d+)", text).group(1)) == A.CR_ABI_VERSION == 4
    # the field's documentation names all three values, and the new mode is not one of the old two
    field = re.search(r"int32_t output_sum;\s*/\*(.*?)\*/", text, re.S).group(1)
    assert "0:" in field and "1:" in field and "CR_OUTPUT_FIXED_SUM (2)" in field
    assert "cr_fixed_sums_to_rgb" in A.SYMBOLS
