"""crucible_amd/csrc/fastdiv.hpp, the division-free decode of work items, checked without a device: tests/fastdiv_check.cpp
compiles the header with g++ and holds fastdiv(n, fastdiv_make(d)) to n / d for the divisors 1, 2, 3, 5, 7, 128, 480, 16384,
65535, 2^26, 2^31, 2^32 - 1 and 2^k, 2^k +- 1 for every k; per divisor the dividends 0, 1, d - 1, d, d + 1, 2^26 - 1, 2^31,
2^32 - 1 and m * d - 1, m * d, m * d + 1 for the multiples next to 2^32; and 10^6 seeded pairs.  Zero mismatches.  The
program is built twice, plain and with -fsanitize=address,undefined, and both must print the same line with nothing on stderr."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """(plain, sanitized)"""
    out = tmp_path_factory.mktemp("fastdiv_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"fastdiv_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "fastdiv_check.cpp")])
        built.append(exe)
    return built


@pytest.mark.parametrize("seed", [1, 0xC0FFEE])
def test_fastdiv_is_the_division(exes, seed):
    lines = []
    for exe in exes:
        res = subprocess.run([exe, str(seed)], capture_output=True, timeout=300)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stdout.decode(), res.stderr.decode())
        lines.append(res.stdout.decode().strip())
    assert lines[0] == lines[1]
    words = lines[0].split()
    assert words[0::2] == ["divisors", "edge_cases", "random_cases", "mismatches"]
    divisors, edge, rnd, bad = (int(x) for x in words[1::2])
    want = {1, 2, 3, 5, 7, 128, 480, 16384, 65535, 2 ** 26, 2 ** 31, 2 ** 32 - 1} | {2 ** k + o for k in range(32) for o in (-1, 0, 1)}
    assert divisors == len([d for d in want if 1 <= d < 2 ** 32])
    assert edge >= divisors * 12 and rnd == 10 ** 6 and bad == 0   # (at least twelve distinct dividends for every divisor, d = 1 included)
