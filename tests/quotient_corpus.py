"""Operand pairs for tests/test_gpu_quotient.py (and their properties, checked without a GPU by tests/test_quotient_host.py):
Sphere::hit's quotient n / a through sphere_quot of crucible_amd/csrc/pathtrace.hpp, which takes its short form when every lane
of the wave holds 2^-400 <= |n| < 2^400 and a divisor whose shared reciprocal is valid (2^-400 <= a < 2^400), and divides
otherwise.  The corpus is laid out in waves of 64 pairs; every group is padded to whole waves with its own pairs, so that the
path a group takes is the path its definition implies."""
import numpy as np

WAVE = 64
LO, HI = -400, 400            # the guard's range: 2^LO <= |x| < 2^HI
MAIN_PAIRS = 1 << 22
SHORT, DIVIDED = 1, 2         # QuotOut.path of tests/quotient_check.hip
EPS = 2.0 ** -52


def in_range(x):
    """2^LO <= |x| < 2^HI by frexp (|x| = m 2^e, 0.5 <= m < 1): -399 <= e <= 400 for a finite non-zero x."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    return np.isfinite(x) & (x != 0) & (e >= LO + 1) & (e <= HI)


def short_form_expected(pairs):
    """Per pair: the wave it lies in holds only pairs the short form is proven for (n in range, a in range and positive)."""
    ok = in_range(pairs[:, 0]) & in_range(pairs[:, 1]) & (pairs[:, 1] > 0)
    return np.repeat(ok.reshape(-1, WAVE).all(axis=1), WAVE)


def rand_in_range(rs, n, signed):
    """n numbers with the exponent uniform over the guard's range and a random 52-bit fraction."""
    e = rs.randint(LO, HI, size=n)
    frac = rs.randint(0, 1 << 52, size=n, dtype=np.int64).astype(np.float64) * EPS
    x = np.ldexp(1.0 + frac, e)
    return x * rs.choice([-1.0, 1.0], size=n) if signed else x


def pad(pairs):
    """Whole waves: the group's own pairs repeated."""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    k = (-len(pairs)) % WAVE
    return np.concatenate([pairs, pairs[np.arange(k) % len(pairs)]]) if k else pairs


def cross(ns, as_):
    return np.array([(n, a) for n in ns for a in as_], dtype=np.float64)


def near_ties(rs, count):
    """Pairs whose exact quotient lies within 2^-60 (relative) of the midpoint of two neighbouring f64 values.
    With an odd 26-bit A and an odd 54-bit T (T / 2 is such a midpoint, in units of the quotient's last place), the integer
    T A + d is a multiple of 2^27 -- so it has at most 53 significant bits and is an f64 -- when T = -d / A mod 2^27, and then
    (T A + d) / A = T + d / A with |d / A| <= 2^18 / 2^25 = 2^-7 against T >= 2^53: 2^-60.  d is odd, so T is, and not zero:
    a quotient is never a tie exactly.  Both operands are then scaled by powers of two inside the range."""
    out = []
    for _ in range(count):
        A = int(rs.randint(1 << 25, 1 << 26)) | 1
        d = (int(rs.randint(0, 1 << 18)) | 1) * (1 if rs.randint(2) else -1)
        low = (-d * pow(A, -1, 1 << 27)) % (1 << 27)
        T = (1 << 53) | (int(rs.randint(0, 1 << 26)) << 27) | low
        N = T * A + d
        assert T & 1 and N % (1 << 27) == 0 and (N >> 27).bit_length() <= 53
        n, a = float(N >> 27), float(A)
        assert int(n) == N >> 27
        ea = int(rs.randint(LO + 200, HI - 200))
        n, a = np.ldexp(n, ea + int(rs.randint(-150, 150)) - 52), np.ldexp(a, ea - 25)
        out.append((n * (1 if rs.randint(2) else -1), a))
    return np.array(out, dtype=np.float64)


def quotient_corpus(seed=20250611):
    """{group: (pairs, path)}: pairs n x 2 in whole waves; path SHORT or DIVIDED, what every pair of the group must report."""
    rs = np.random.RandomState(seed)
    sub = np.array([5e-324, 2.0 ** -1040, 2.0 ** -1023, np.nextafter(2.0 ** -1022, 0)])
    some_n, some_a = rand_in_range(rs, 16, True), rand_in_range(rs, 16, False)
    inside = np.array([2.0 ** LO, 2.0 ** LO * (1 + EPS), 2.0 ** (LO + 1), 2.0 ** (HI - 1), np.nextafter(2.0 ** HI, 0)])
    outside = np.array([2.0 ** (LO - 1), np.nextafter(2.0 ** LO, 0), 2.0 ** HI, 2.0 ** HI * (1 + EPS), 2.0 ** (HI + 1)])
    g = {}
    g["main"] = (np.stack([rand_in_range(rs, MAIN_PAIRS, True), rand_in_range(rs, MAIN_PAIRS, False)], axis=1), SHORT)
    g["n_bounds_inside"] = (cross(np.concatenate([inside, -inside]), some_a), SHORT)
    g["n_bounds_outside"] = (cross(np.concatenate([outside, -outside]), some_a), DIVIDED)
    g["a_bounds_inside"] = (cross(some_n, inside), SHORT)
    g["a_bounds_outside"] = (cross(some_n, outside), DIVIDED)
    g["bounds_both_inside"] = (cross(np.concatenate([inside, -inside]), inside), SHORT)
    g["n_zero"] = (cross([0.0, -0.0], some_a), DIVIDED)
    g["n_subnormal"] = (cross(np.concatenate([sub, -sub]), some_a), DIVIDED)
    g["n_inf"] = (cross([np.inf, -np.inf], some_a), DIVIDED)
    g["n_nan"] = (cross([np.nan, -np.nan], some_a), DIVIDED)
    g["a_zero"] = (cross(np.concatenate([some_n, [0.0, -0.0, np.inf, np.nan]]), [0.0]), DIVIDED)
    g["a_subnormal"] = (cross(some_n, sub), DIVIDED)
    g["a_inf"] = (cross(np.concatenate([some_n, [0.0, np.inf, -np.inf]]), [np.inf]), DIVIDED)
    g["a_nan"] = (cross(some_n, [np.nan]), DIVIDED)
    g["a_negative"] = (cross(some_n, -some_a), DIVIDED)   # |d|^2 is never negative; a negative reciprocal reads as out of range
    a = rand_in_range(rs, 4096, False)
    g["n_equals_a"] = (np.stack([a * rs.choice([-1.0, 1.0], size=len(a)), a], axis=1), SHORT)
    # exact multiples: a with a 30-bit fraction, k below 2^20, exponents 40 binades inside the range -- k a is exact and in range
    a = np.ldexp(1.0 + rs.randint(0, 1 << 30, size=4096).astype(np.float64) * 2.0 ** -30, rs.randint(LO + 40, HI - 40, size=4096))
    k = rs.randint(1, 1 << 20, size=4096).astype(np.float64) * rs.choice([-1.0, 1.0], size=4096)
    g["multiples"] = (np.stack([k * a, a], axis=1), SHORT)
    g["near_ties"] = (near_ties(rs, 4096), SHORT)
    # mixed waves: one lane outside the range among 63 inside -- the whole wave divides
    odd = [(0.0, None), (-0.0, None), (5e-324, None), (np.inf, None), (np.nan, None), (2.0 ** HI, None), (2.0 ** (LO - 1), None),
           (None, 0.0), (None, 5e-324), (None, np.inf), (None, np.nan), (None, 2.0 ** HI), (None, np.nextafter(2.0 ** LO, 0))]
    mixed = []
    for j, (n_odd, a_odd) in enumerate(odd * 4):
        w = np.stack([rand_in_range(rs, WAVE, True), rand_in_range(rs, WAVE, False)], axis=1)
        lane = (j * 13 + 5) % WAVE
        if n_odd is not None:
            w[lane, 0] = n_odd
        else:
            w[lane, 1] = a_odd
        mixed.append(w)
    g["mixed_waves"] = (np.concatenate(mixed), DIVIDED)
    return {k: (pad(v), p) for k, (v, p) in g.items()}
