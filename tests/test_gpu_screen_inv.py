"""walk_begin_screened's f32 1/direction on the device (tests/screen_inv_check.hip runs screen_rcp1, screen_inv and
screen_in_range_lazy of crucible_amd/csrc/pathtrace.hpp): r1 = v_rcp_f64 and one Newton step, if = (float)r1.
  * |r1 d - 1| <= 2^-40 for every d with |1/d| in [2^-101, 2^101] -- 2^8 under what the screen's bound needs (the comment above
    screen_q) -- evaluated exactly with fractions.Fraction for every one of the 3 * 10^6 components in range (the test's seconds).
  * the new `if` is within one f32 ulp of (float)(1.0 / d) there.
  * every zero, subnormal, infinite, NaN and out-of-range component fails the range test (out of range: |1/d| beyond
    2^+-100 by more than 2^-22 relative -- nearer than that, the f32 rounding may land on the bound, and either side is valid).
Each group of the corpus must bring at least 1000 cases to the class it is aimed at; that is checked from the corpus alone."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_corpus as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "crucible_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "screen_inv_check.hip")
INV_OUT = np.dtype([("r1", "<f8"), ("if_new", "<f4"), ("if_old", "<f4"), ("in_range", "<u4"), ("pad", "<u4")])
N = 1 << 20
ACCURATE, MUST_FAIL = "accurate", "must_fail"


def corpus(seed=5):
    rs = np.random.RandomState(seed)
    sign = lambda n: rs.choice([-1.0, 1.0], n)   # noqa: E731
    g = {}
    g["uniform_exponents"] = (sign(N) * rs.uniform(1.0, 2.0, N) * 2.0 ** rs.randint(-110, 111, N), ACCURATE)
    g["near_powers_of_two"] = (W.ulp_shift(sign(N) * 2.0 ** rs.randint(-101, 102, N), rs.randint(-4, 5, N)), ACCURATE)
    g["near_range_ends"] = (W.ulp_shift(sign(N) * 2.0 ** rs.choice([-100.0, 100.0], N), rs.randint(-64, 65, N)), ACCURATE)
    g["huge_and_tiny"] = (sign(N) * rs.uniform(1.0, 2.0, N) * 2.0 ** (rs.choice([-1.0, 1.0], N) * rs.randint(990, 1011, N)), MUST_FAIL)
    sub = sign(N) * (rs.randint(1, 1 << 52, N).astype(np.int64).view(np.float64))   # subnormals: exponent field 0
    special = rs.choice([0.0, -0.0, np.inf, -np.inf, np.nan], N)
    g["specials"] = (np.where(rs.uniform(size=N) < 0.5, sub, special), MUST_FAIL)
    return g


def accurate_class(d):
    with np.errstate(all="ignore"):
        a = np.abs(d)
        return np.isfinite(a) & (a >= 2.0 ** -101) & (a <= 2.0 ** 101)


def must_fail_class(d):
    with np.errstate(all="ignore"):
        a = np.abs(d)
        sub = (a < 2.0 ** -1022)   # zeros and subnormals
        return sub | ~np.isfinite(d) | (a > 2.0 ** 100 * (1 + 2.0 ** -22)) | (a < 2.0 ** -100 * (1 - 2.0 ** -22))


@pytest.fixture(scope="module")
def inv_run(tmp_path_factory):
    groups = corpus()
    # a passing run proves something only if every group reaches the class it is aimed at: from the corpus alone, first
    for name, (v, aim) in groups.items():
        got = (accurate_class(v) if aim == ACCURATE else must_fail_class(v)).sum()
        assert len(v) == N and got >= 1000, (name, aim, got)
    d = tmp_path_factory.mktemp("screen_inv")
    exe = d / "screen_inv_check"
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)
    vals = np.concatenate([v for v, _ in groups.values()])
    vals.tofile(d / "inv.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(d / "inv.out", dtype=INV_OUT)
    assert len(out) == len(vals)
    names = np.concatenate([[k] * N for k in groups])
    return vals, names, out


@pytest.mark.gpu
def test_one_newton_step_is_within_2_to_minus_40(inv_run):
    vals, names, out = inv_run
    sel = np.flatnonzero(accurate_class(vals))
    d, r1 = vals[sel], out["r1"][sel]
    assert np.isfinite(r1).all()
    bound, one = Fraction(1, 1 << 40), Fraction(1)
    worst, bad = {}, []
    for i, (r, x, g) in enumerate(zip(r1.tolist(), d.tolist(), names[sel].tolist())):   # every component, exactly
        nr, dr = r.as_integer_ratio()
        nx, dx = x.as_integer_ratio()
        err = abs(Fraction(nr * nx, dr * dx) - one)
        if err > worst.get(g, 0):
            worst[g] = err
        if err > bound:
            bad.append(i)
    print(f"\n[screen inv] {len(sel)} components in range, each |r1 d - 1| evaluated with fractions")
    for g, w in sorted(worst.items()):
        print(f"[screen inv]   {g}: {(names[sel] == g).sum()} in range, largest |r1 d - 1| = 2^{np.log2(float(w)):.2f}")
    assert not bad, f"{len(bad)} beyond 2^-40; first: d {float(d[bad[0]]).hex()} r1 {float(r1[bad[0]]).hex()} ({names[sel][bad[0]]})"


@pytest.mark.gpu
def test_new_if_is_within_one_f32_ulp_of_the_divided_one(inv_run):
    vals, names, out = inv_run
    sel = accurate_class(vals)
    new, old = out["if_new"][sel], out["if_old"][sel]
    assert np.isfinite(new).all() and np.isfinite(old).all()
    step = np.abs(new.view(np.int32).astype(np.int64) - old.view(np.int32).astype(np.int64))   # same sign: adjacent bit patterns
    bad = np.flatnonzero((step > 1) | (np.signbit(new) != np.signbit(old)))
    print(f"\n[screen inv] if: {(step == 0).sum()} equal, {(step == 1).sum()} one ulp apart, {len(bad)} further")
    assert len(bad) == 0, (float(vals[sel][bad[0]]).hex(), float(new[bad[0]]).hex(), float(old[bad[0]]).hex())
    # with the old value in the middle of the range, the decision is the old one's
    a = np.abs(vals[sel])
    mid = (a >= 2.0 ** -99) & (a <= 2.0 ** 99)
    assert (out["in_range"][sel][mid] == 1).all()


@pytest.mark.gpu
def test_what_cannot_be_screened_fails_the_range_test(inv_run):
    vals, names, out = inv_run
    sel = must_fail_class(vals)
    bad = np.flatnonzero(sel & (out["in_range"] != 0))
    with np.errstate(all="ignore"):
        print(f"\n[screen inv] {sel.sum()} components that must fail: {np.isnan(vals).sum()} NaN, {np.isinf(vals).sum()} infinite, "
              f"{(vals == 0).sum()} zero, {((vals != 0) & (np.abs(vals) < 2.0 ** -1022)).sum()} subnormal; {len(bad)} passed")
    assert len(bad) == 0, (float(vals[bad[0]]).hex(), float(out["if_new"][bad[0]]).hex(), names[bad[0]])
