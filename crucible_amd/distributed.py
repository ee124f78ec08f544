"""Samples-per-pixel sharding across the GPUs of a node (one process per GPU).

Every sample is an independent path (reference src/camera/ray_casting.rs:82-105)
and the RNG is keyed by (seed, pixel, sample), so rank r of N renders sample
indices [r*spp/N, (r+1)*spp/N) of EVERY pixel and the union is the 1-GPU sample
set.  Each rank holds a full-frame RGB *sum*; one reduce (RCCL over xGMI on GPUs,
gloo in CPU tests) adds them on rank 0, which divides by spp (average_samples,
ray_casting.rs:154-173).  The result differs from the 1-GPU image only by the
order of the floating-point adds -- unless the ranks render relaxed sums as
fixed-point words (output_sum=CR_OUTPUT_FIXED_SUM) and add those with
reduce_fixed_sums: rank 0's cr_fixed_sums_to_rgb then gives the 1-GPU relaxed
frame bit for bit.
"""

FX_NAN = -(1 << 63)          # bit 63 of a CR_OUTPUT_FIXED_SUM word (the NaN flag), as an int64
FX_MAGNITUDE = (1 << 63) - 1  # bits 0..62


def shard_range(rank, world, spp):
    """(sample_begin, sample_count) of `rank`; the ranges partition [0, spp)."""
    if not (0 <= rank < world):
        raise ValueError("rank outside [0, world)")
    begin = rank * spp // world
    end = (rank + 1) * spp // world
    return begin, end - begin


def reduce_to_mean(sum_tensor, spp, dst=0):
    """In-place: reduce the per-rank sums to `dst` and turn them into the per-pixel mean there.
    Without an initialised process group this is the 1-GPU case (divide only)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.reduce(sum_tensor, dst=dst, op=dist.ReduceOp.SUM)
        if dist.get_rank() != dst:
            return sum_tensor
    sum_tensor.div_(float(spp))
    return sum_tensor


def reduce_fixed_sums(t, dst=0):
    """In-place: combine the ranks' CR_OUTPUT_FIXED_SUM words (an int64 tensor holding the uint64 bits) on `dst` with
    c = ((a & M) + (b & M)) | ((a | b) & F): one SUM of the magnitudes (they total below 2^63 for one frame's shards, so
    int64 cannot overflow) and one MAX of a uint8 plane of the NaN flags.  On `dst` t then holds the frame's words;
    elsewhere its magnitudes.  Without an initialised process group this is the 1-GPU case (nothing to do)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return t
    flags = (t < 0).to(torch.uint8)
    t.bitwise_and_(FX_MAGNITUDE)
    dist.reduce(t, dst=dst, op=dist.ReduceOp.SUM)
    dist.reduce(flags, dst=dst, op=dist.ReduceOp.MAX)
    if dist.get_rank() == dst:
        t.bitwise_or_(flags.to(torch.int64) * FX_NAN)
    return t
