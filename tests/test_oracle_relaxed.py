"""The oracle's CR_SUM_RELAXED frame, without a GPU (include/crucible_hip.h, "How a pixel's samples are summed").

The relaxed frame is a deterministic function of the same paths as the reference order: attenuations multiplied in path
order, each sample added as round_half_even(colour * 2^S) to a 64-bit word, S = min(52, 62 - floor(log2 n)), and a
finalize that converts the word once, scales by 2^-S and divides by the frame's sample count.  These tests pin that
restatement: its distance from the reference order stays inside the header's documented bound, the words of shards add
up, a finalize written here in plain Python reproduces the oracle's reals bit for bit, and full-scale words come out
exactly n * 2^S."""
import math

import numpy as np
import pytest

import scenes
from crucible_amd import _abi as A

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
RELAX = A.CR_SUM_RELAXED
FIXED = A.CR_OUTPUT_FIXED_SUM
FLAG = 1 << 63


def scale_log2(n):
    """S for n samples per pixel: n * 2^S < 2^63, at most 52."""
    return min(52, 62 - (int(n).bit_length() - 1))


def finalize(words, samples, real_type, output_sum=0):
    """The header's finalize in plain arithmetic: m = w & ~2^63 -> float(m) (correctly rounded) -> * 2^-S -> / samples
    for a mean (output_sum 0; kept as the sum for 1) -> NaN where the flag is set -> rounded once to the output type.
    S is of `samples`, the count the words' scale was taken from."""
    S = scale_log2(samples)
    out = np.empty(words.shape, dtype=np.float64 if real_type == A.CR_REAL_F64 else np.float32)
    flat_in, flat_out = words.reshape(-1), out.reshape(-1)
    for i, w in enumerate(flat_in):
        w = int(w)
        s = math.ldexp(float(w & (FLAG - 1)), -S)
        if output_sum == 0:
            s = s / float(samples)
        if w & FLAG:
            s = math.nan
        flat_out[i] = s if real_type == A.CR_REAL_F64 else np.float32(s)
    return out


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def render(oracle, sc, **kw):
    return oracle.render_image(sc, seed=kw.pop("seed", SEED), **kw)


@pytest.mark.parametrize("samples", [1, 2, 7, 64, 512, 2047, 2048, 5000])
def test_relaxed_within_the_documented_bound(o64, samples):
    """Deep, mostly metal paths (depth 50): the relaxed mean lies within (2 * max_depth + samples) * 2^-53 of the
    reference order's, per channel, with equal counters -- the claim include/crucible_hip.h makes."""
    sc = scenes.deep_metal_scene(width=6 if samples >= 2048 else 12, samples=samples)
    ref, rst = render(o64, sc)
    img, st = render(o64, sc, sum_order=RELAX)
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert rst["segments"] > 8 * st["samples"]   # the paths are long: 10 to 11 segments per sample
    bound = (2 * 50 + samples) * 2.0 ** -53
    d = np.abs(img - ref).max()
    assert d <= bound, (d / 2.0 ** -53, bound / 2.0 ** -53)
    assert img.min() >= 0.0 and img.max() <= 1.0 and st["nan_pixels"] == 0


@pytest.mark.parametrize("samples", [1, 64, 2048])
def test_relaxed_f32_paths_match_the_reference_order(o32, samples):
    """f32: the same paths (equal counters) and a frame in [0, 1]; the distance from the reference order is measured,
    not asserted (the f32 sequential sum rounds at 2^-24 per term)."""
    sc = scenes.deep_metal_scene(width=6, samples=samples)
    ref, rst = render(o32, sc)
    img, st = render(o32, sc, sum_order=RELAX)
    assert img.dtype == np.float32
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert img.min() >= 0.0 and img.max() <= 1.0 and st["nan_pixels"] == 0


@pytest.mark.parametrize("rt", [A.CR_REAL_F64, A.CR_REAL_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("samples,cuts", [(12, (0, 5, 5, 9, 12)), (3000, (0, 1000, 1000, 2047, 3000))],
                         ids=["12spp", "3000spp-S51"])
def test_shard_words_add_up(oracles, rt, samples, cuts):
    """CR_OUTPUT_FIXED_SUM words of shards are on the whole frame's scale, so they add up to the whole frame's words
    exactly -- an empty shard included (all zeros)."""
    o = oracles[rt]
    sc = scenes.deep_metal_scene(width=4, samples=samples, depth=12)
    whole, wst = render(o, sc, sum_order=RELAX, output_sum=FIXED)
    assert whole.dtype == np.uint64
    total = np.zeros_like(whole)
    seg = 0
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        part, pst = render(o, sc, sum_order=RELAX, output_sum=FIXED, sample_begin=s0, sample_count=s1 - s0)
        if s1 == s0:
            assert not part.any()
        total += part
        seg += pst["segments"]
    assert np.array_equal(total, whole)
    assert seg == wst["segments"]
    assert not (whole & np.uint64(FLAG)).any()
    assert int(whole.max()) < samples * 2 ** scale_log2(samples)


@pytest.mark.parametrize("rt", [A.CR_REAL_F64, A.CR_REAL_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("samples", [1, 5, 2047, 2048, 3000])
def test_python_finalize_reproduces_the_oracle(oracles, rt, samples):
    """The words through the Python finalize equal the oracle's mean (output_sum 0) and real sums (output_sum 1) bit
    for bit; for a shard the mean divides by the frame's count and the real sum is at the shard's own scale."""
    o = oracles[rt]
    sc = scenes.deep_metal_scene(width=4, samples=samples, depth=8)
    words, _ = render(o, sc, sum_order=RELAX, output_sum=FIXED)
    mean, _ = render(o, sc, sum_order=RELAX)
    sums, _ = render(o, sc, sum_order=RELAX, output_sum=1)
    assert np.array_equal(bits(finalize(words, samples, rt)), bits(mean))
    assert np.array_equal(bits(finalize(words, samples, rt, output_sum=1)), bits(sums))
    if samples >= 5:
        # a shard's mean and real sums are at its own count's scale (divided by the frame's count for the mean): the
        # frame-scale words give them bit for bit where the two scales agree
        b, n = samples // 3, samples - samples // 3
        sw, _ = render(o, sc, sum_order=RELAX, output_sum=FIXED, sample_begin=b, sample_count=n)
        smean, _ = render(o, sc, sum_order=RELAX, sample_begin=b, sample_count=n)
        ssum, _ = render(o, sc, sum_order=RELAX, output_sum=1, sample_begin=b, sample_count=n)
        fmean, fsum = finalize(sw, samples, rt), finalize(sw, samples, rt, output_sum=1)
        if scale_log2(n) == scale_log2(samples):
            assert np.array_equal(bits(fmean), bits(smean)) and np.array_equal(bits(fsum), bits(ssum))
        else:   # 2048 and 3000 spp: the frame is at 2^51, a shard of fewer than 2048 samples at 2^52
            assert scale_log2(n) == scale_log2(samples) + 1
            eps = 2.0 ** -52 if rt == A.CR_REAL_F64 else 2.0 ** -23   # the last rounding to the output type
            dsum = np.abs(ssum.astype(np.float64) - fsum)
            assert (dsum <= n * 2.0 ** -52 + eps * np.abs(fsum)).all()   # one rounding per sample at 2^-52
            assert rt == A.CR_REAL_F32 or dsum.max() > 0                 # f64 sees the finer scale
            assert (np.abs(smean.astype(np.float64) - fmean) <= 2.0 ** -51 + eps * np.abs(fmean)).all()


def test_finalize_rounds_once():
    """The finalize's own edges: a word above 2^53 rounds to nearest-even once in the conversion; f32 rounds the double
    quotient once more; the flag wins over any magnitude."""
    w = np.array([(1 << 53) + 1, (1 << 53) + 3, (1 << 63) - 1, FLAG | 5, FLAG], dtype=np.uint64)
    f = finalize(w, 1, A.CR_REAL_F64, output_sum=1)
    assert f[0] == 2.0 and f[1] == math.ldexp((1 << 53) + 4, -52) and f[2] == 2048.0
    assert np.isnan(f[3]) and np.isnan(f[4])
    g = finalize(np.array([3 << 52], dtype=np.uint64), 3, A.CR_REAL_F32)
    assert g.dtype == np.float32 and g[0] == np.float32(1.0)


@pytest.mark.parametrize("rt", [A.CR_REAL_F64, A.CR_REAL_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2047, 2048, 4095, 4096, 65535])
def test_full_scale_words(oracles, rt, n):
    """Every sample exactly 1.0 (a white sky, texel 255 / 255): the words are exactly n * 2^S -- the largest each scale
    allows, below 2^63 -- the flag is clear and the mean is exactly 1.0."""
    o = oracles[rt]
    sc = scenes.white_sky_scene(width=2, samples=n)
    words, st = render(o, sc, sum_order=RELAX, output_sum=FIXED)
    want = n * 2 ** scale_log2(n)
    assert want < 2 ** 63
    assert all(int(w) == want for w in words.reshape(-1)), (int(words.min()), int(words.max()), want)
    mean, _ = render(o, sc, sum_order=RELAX)
    assert (mean == 1.0).all() and st["texel_fetches"] == st["samples"]


def test_nan_sets_the_flag(oracles):
    """A colour that is not a number (a camera whose look-from is its look-at) sets bit 63 of its words; the mean is
    NaN and the pixel counts as a NaN pixel, as in the reference order."""
    sc = scenes.few_spheres(2, width=8, samples=2)
    sc.scene_cam.look_from((1.0, 2.0, 3.0))
    sc.scene_cam.look_at((1.0, 2.0, 3.0))
    for rt, o in oracles.items():
        words, _ = render(o, sc, sum_order=RELAX, output_sum=FIXED)
        assert ((words & np.uint64(FLAG)) != 0).all()
        mean, st = render(o, sc, sum_order=RELAX)
        ref, rst = render(o, sc)
        assert np.isnan(mean).all() and st["nan_pixels"] == rst["nan_pixels"] == mean.shape[0] * mean.shape[1]


def test_default_order_is_the_reference_order(o64):
    """The oracle has no handle default: CR_SUM_DEFAULT is the reference order, and fixed words need CR_SUM_RELAXED."""
    sc = scenes.mixed_scene(24, 3)
    ref, _ = render(o64, sc)
    dflt, _ = render(o64, sc, sum_order=A.CR_SUM_DEFAULT)
    relaxed, _ = render(o64, sc, sum_order=RELAX)
    assert np.array_equal(bits(ref), bits(dflt))
    assert not np.array_equal(bits(ref), bits(relaxed)) and np.abs(ref - relaxed).max() <= 1e-13
    with pytest.raises(AssertionError):
        render(o64, sc, output_sum=FIXED)
