"""An independent model of cr_render_adaptive_* (include/crucible_hip.h): numpy and Python integers only, no code shared with
the library.  Input: the per-pass CR_OUTPUT_FIXED_SUM words of a frame -- words[p] holds the sums of the sample indices
[pP, (p+1)P) at the scale of the whole frame's `samples`, shape (passes, H, W, 3) uint64, bit 63 the NaN flag -- as the
existing Renderer.render(..., sample_begin=pP, sample_count=P, output_sum=CR_OUTPUT_FIXED_SUM) returns them.  Output: the
samples each pixel takes and the finalized frame."""
import math

import numpy as np

FLAG = np.uint64(1 << 63)
MAG = np.uint64((1 << 63) - 1)


def fx_log2(samples):
    """S of the fixed-point scale 2^S of a frame of `samples` samples: the largest S <= 52 with samples * 2^S < 2^63."""
    s = 52
    while samples << s >= 1 << 63:
        s -= 1
    return s


def term(e, o):
    """d = |mag(E) - mag(O)| >> 12 of two words (Python ints)."""
    a, b = int(e) & ((1 << 63) - 1), int(o) & ((1 << 63) - 1)
    return abs(a - b) >> 12


def weight(S, qP, n_b):
    """2^(S-12) * qP * 3 N_b as a Python int."""
    return (qP * 3 * n_b) << (S - 12)


def threshold(tolerance, S, qP, n_b):
    """T_b = min(floor(tolerance * weight), 2^63): the weight is exact as a float, then one f64 multiply and one floor."""
    w = float(weight(S, qP, n_b))
    assert int(w) == weight(S, qP, n_b)
    t = float(tolerance) * w
    if not t < 2.0 ** 63:
        return 1 << 63
    return int(math.floor(t))


def blocks_of(W, H, block):
    """(x0, y0, w, h) of every block, row by row; blocks are anchored at pixel (0, 0), edge blocks partial."""
    return [(x0, y0, min(block, W - x0), min(block, H - y0)) for y0 in range(0, H, block) for x0 in range(0, W, block)]


def block_sums(words, q, rect):
    """(E, O) magnitudes and the NaN mask of a block after q pairs of passes."""
    x0, y0, w, h = rect
    part = words[:2 * q, y0:y0 + h, x0:x0 + w, :]
    mags = part & MAG
    E = mags[0::2].sum(axis=0, dtype=np.uint64)
    O = mags[1::2].sum(axis=0, dtype=np.uint64)
    nan = ((part & FLAG) != 0).any(axis=0)
    return E, O, nan


def difference(E, O):
    """D_b: the exact integer sum of |E - O| >> 12."""
    return sum(term(e, o) for e, o in zip(E.reshape(-1).tolist(), O.reshape(-1).tolist()))


def first_judgement_ratios(words, P, min_samples, samples, block):
    """Per block D_b / (2^(S-12) * qP * 3 N_b) at the first judgement (q = min_samples / 2P), the mean absolute difference of
    the two half-frame means; None when no judgement happens before `samples`."""
    if min_samples >= samples:
        return None
    _, H, W, _ = words.shape
    S, q = fx_log2(samples), min_samples // (2 * P)
    out = []
    for rect in blocks_of(W, H, block):
        E, O, _ = block_sums(words, q, rect)
        out.append(difference(E, O) / weight(S, q * P, rect[2] * rect[3]))
    return out


def finalize(mag, nan, n, S, R):
    """((mag * 2^-S) / n) as the library's finalize kernels form it: the word in two exact halves, one add, one multiply, one
    divide, all in f64, NaN where a flag is set, then rounded to R."""
    hi = (mag >> np.uint64(32)).astype(np.float64) * 4294967296.0
    lo = (mag & np.uint64(0xFFFFFFFF)).astype(np.float64)
    s = ((hi + lo) * 2.0 ** -S) / float(n)
    s = np.where(nan, np.nan, s)
    return s.astype(R)


def adaptive(words, P, min_samples, samples, block, tolerance, R):
    """(counts (H, W) int32, frame (H, W, 3) of dtype R, decisions) -- decisions: per block the list of (n, D_b, T_b) judgements."""
    passes, H, W, _ = words.shape
    assert passes * P == samples and samples % (2 * P) == 0 and min_samples % (2 * P) == 0 and 0 < min_samples <= samples
    S = fx_log2(samples)
    counts = np.zeros((H, W), dtype=np.int32)
    frame = np.zeros((H, W, 3), dtype=R)
    decisions = []
    for rect in blocks_of(W, H, block):
        x0, y0, w, h = rect
        q, log = 0, []
        while True:
            q += 1
            n = 2 * q * P
            if n >= samples:
                break
            if n < min_samples:
                continue
            E, O, _ = block_sums(words, q, rect)
            D, T = difference(E, O), threshold(tolerance, S, q * P, w * h)
            log.append((n, D, T))
            if D <= T:
                break
        E, O, nan = block_sums(words, q, rect)
        counts[y0:y0 + h, x0:x0 + w] = n
        frame[y0:y0 + h, x0:x0 + w] = finalize(E + O, nan, n, S, R)
        decisions.append(log)
    return counts, frame, decisions
