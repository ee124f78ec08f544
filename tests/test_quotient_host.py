"""Sphere::hit's quotient with a shared reciprocal, the parts that need no device.
- tests/quot_range_check.cpp compiles crucible_amd/csrc/records.hpp with g++ alone (no HIP include path) and holds quot_in_range -- the guard's range test --
  to frexp over every exponent of the format (so at and around both bounds), zeros, subnormals, infinities, NaNs and seeded random
  bit patterns; built twice, plain and with -fsanitize=address,undefined, both must print the same line and nothing on stderr.
- tests/quotient_check.hip and tests/sphere_hoist_check.hip compile for gfx950.
- the corpus of tests/test_gpu_quotient.py is what its groups say: whole waves, every group on one side of the range."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_corpus as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """(plain, sanitized)"""
    out = tmp_path_factory.mktemp("quot_range_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"quot_range_check_{tag}")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "quot_range_check.cpp")])
        built.append(exe)
    return built


@pytest.mark.parametrize("seed", [1, 0xC0FFEE])
def test_the_range_test_is_frexp(exes, seed):
    lines = []
    for exe in exes:
        res = subprocess.run([exe, str(seed)], capture_output=True, timeout=300)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stdout.decode(), res.stderr.decode())
        lines.append(res.stdout.decode().strip())
    assert lines[0] == lines[1]
    words = lines[0].split()
    assert words[0::2] == ["cases", "mismatches"], lines[0]
    assert int(words[1]) >= 2 * (2098 * 5 + 2000000) and int(words[3]) == 0, lines[0]


@pytest.mark.parametrize("src", ["quotient_check.hip", "sphere_hoist_check.hip"])
def test_the_check_programs_compile_for_gfx950(tmp_path, src):
    import test_gpu_quotient as T
    subprocess.run(T.HIPCC + ["--offload-device-only", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", src)], check=True, timeout=600)


def test_the_corpus_is_what_its_groups_say():
    groups = Q.quotient_corpus()
    assert len(groups["main"][0]) >= 1 << 22
    for name, (v, path) in groups.items():
        assert len(v) % Q.WAVE == 0 and v.shape[1] == 2, name
        ok = Q.in_range(v[:, 0]) & Q.in_range(v[:, 1]) & (v[:, 1] > 0)
        if path == Q.SHORT:
            assert ok.all(), name
        elif name == "mixed_waves":
            assert ((~ok).reshape(-1, Q.WAVE).sum(axis=1) == 1).all()   # one lane of every wave
        else:
            assert not ok.any(), name
        assert (Q.short_form_expected(v) == (path == Q.SHORT)).all(), name
    n, a = groups["n_equals_a"][0].T
    assert (np.abs(n) == a).all()
    n, a = groups["multiples"][0].T
    assert (n / a == np.round(n / a)).all() and (np.abs(n / a) < 1 << 20).all()
    # the near ties, in exact arithmetic: |n / a - t| <= 2^-60 |t| for a midpoint t of two neighbouring f64 values
    from fractions import Fraction
    for n, a in groups["near_ties"][0][:512]:
        q = abs(Fraction(float(n)) / Fraction(float(a)))
        e = q.numerator.bit_length() - q.denominator.bit_length()
        scaled = q / Fraction(2) ** (e - 53)          # in [2^52, 2^54): units of (at most) the last place
        if scaled >= 1 << 53:
            scaled /= 2
        t = Fraction(2 * int(scaled) + 1, 2)          # the midpoint above floor(scaled)
        assert scaled != t and abs(scaled - t) <= t / (1 << 60), (n, a)
