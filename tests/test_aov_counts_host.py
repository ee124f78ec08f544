"""crucible_amd/csrc/aov_counts.hpp, the integer rules of the guide pass at a count plane, checked without a device:
tests/aov_counts_check.cpp compiles the header with g++ (plain, and with -fsanitize=undefined,address as the stand-alone
program it is) and answers one line per question; the rules are restated here in Python integers.  The cases: the clamp at
the ends of int32 for the smallest and largest `samples` and on both sides of the scale's step at 2048; the group bound for
every tile maximum 0..67 and next to INT32_MAX, where `max + 3` must not be formed in int; units whose range starts
beyond the bound; the divisor rule at 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("aov_counts_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(out / f"aov_counts_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "aov_counts_check.cpp")])
        built.append(exe)
    return built


def ask(exes, lines):
    """The program's answers to `lines`, one list of ints each; both builds agree and write nothing to stderr."""
    outs = []
    for exe in exes:
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines).encode(), capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    got = [[int(v) for v in l.split()] for l in outs[0].splitlines()]
    assert len(got) == len(lines)
    return got


def clamp(count, samples):
    return min(max(count, 0), samples)


def group_end(g1, tile_max):
    return min(g1, (tile_max + 3) // 4)   # Python integers: no width


def test_clamp(exes):
    cases = [(c, s) for s in (1, 2047, 2048, I32_MAX) for c in (I32_MIN, -1, 0, s, s + 1 if s < I32_MAX else I32_MAX, I32_MAX, s - 1, 1)]
    got = ask(exes, [f"clamp {c} {s}" for c, s in cases])
    assert [g[0] for g in got] == [clamp(c, s) for c, s in cases]
    by = dict(zip(cases, (g[0] for g in got)))
    for s in (1, 2047, 2048, I32_MAX):
        assert by[(I32_MIN, s)] == by[(-1, s)] == by[(0, s)] == 0 and by[(s, s)] == by[(I32_MAX, s)] == s
    assert by[(2048, 2047)] == 2047 and by[(2049, 2048)] == 2048 and by[(2, 1)] == 1


def test_group_bound(exes):
    groups_of = lambda samples: (samples + 3) // 4
    cases = [(g1, m) for m in range(0, 68) for g1 in (1, 2, 16, 17, groups_of(67), groups_of(I32_MAX))]
    cases += [(g1, m) for m in range(I32_MAX - 3, I32_MAX + 1) for g1 in (1, groups_of(I32_MAX) - 1, groups_of(I32_MAX), 2 ** 32 - 1)]
    got = ask(exes, [f"end {g1} {m}" for g1, m in cases])
    assert [g[0] for g in got] == [group_end(g1, m) for g1, m in cases]
    by = dict(zip(cases, (g[0] for g in got)))
    assert by[(17, 0)] == 0 and by[(17, 1)] == by[(17, 4)] == 1 and by[(17, 5)] == 2 and by[(17, 64)] == 16 and by[(17, 65)] == by[(17, 67)] == 17
    assert groups_of(I32_MAX) == 2 ** 29   # (2^31 - 1 + 3) >> 2: formed in uint32_t, 2^31 + 2 does not fit an int
    for m in range(I32_MAX - 3, I32_MAX + 1):
        assert by[(2 ** 32 - 1, m)] == (m + 3) // 4 and by[(2 ** 29, m)] == (2 ** 29 if m > I32_MAX - 3 else 2 ** 29 - 1)


def test_units_beyond_the_bound_do_not_run(exes):
    # (g0, unit_groups, groups, tile_max): the unit covers [g0, min(g0 + unit_groups, groups))
    cases = [(g0, ug, groups, m) for groups, ug in ((17, 1), (17, 4), (17, 17), (2 ** 29, 2 ** 27), (2 ** 29, 1))
             for g0 in sorted({0, ug, 2 * ug, ((groups - 1) // ug) * ug}) if g0 < groups
             for m in (0, 1, 4, 5, 4 * g0, 4 * g0 + 1, 67, I32_MAX - 3, I32_MAX)]
    got = ask(exes, [f"unit {g0} {ug} {groups} {m}" for g0, ug, groups, m in cases])
    ran = 0
    for (g0, ug, groups, m), (a, end, runs) in zip(cases, got):
        want_end = group_end(min(g0 + ug, groups), m)
        assert (a, end, runs) == (g0, want_end, 1 if g0 < want_end else 0), (g0, ug, groups, m)
        assert runs == (1 if m > 4 * g0 else 0)   # the unit runs iff some pixel of the tile has a sample in or after its first group
        ran += runs
    assert 0 < ran < len(cases)


def test_divisor_rule(exes):
    cases = [(0, 0), (0, 1), (1, 0), (1, 1), (2047, 0), (I32_MAX, 0), (I32_MAX, 1)]
    got = ask(exes, [f"div {n} {o}" for n, o in cases])
    assert [g[0] for g in got] == [1 if (n and not o) else 0 for n, o in cases]
    assert got[0] == [0] and got[1] == [0]   # nothing is ever divided by zero
