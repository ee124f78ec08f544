"""Sphere::hit's quotient with a shared reciprocal on the device (tests/quotient_check.hip runs sphere_quot<true> and shared_rcp
of crucible_amd/csrc/pathtrace.hpp; tests/quotient_corpus.py makes the pairs): the helper must return the bits of n / a for every
operand -- NaN for NaN -- whichever of its two paths the wave takes, and the program reports which one ran.  The corpus has 2^22
pairs inside the guard's range in whole waves, groups at and around both exponent bounds, zeros, subnormals, infinities and
NaNs on either side, n = a, exact multiples, quotients within 2^-60 of a rounding tie, and waves with one lane outside the range."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_corpus as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "crucible_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "quotient_check.hip")
QUOT_OUT = np.dtype([("q", "<f8"), ("ref", "<f8"), ("path", "<u4"), ("pad", "<u4")])


def build_quotient_check(exe):
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)


def same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def quot_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("quotient")
    exe = d / "quotient_check"
    build_quotient_check(exe)
    groups = Q.quotient_corpus()
    pairs = np.concatenate([v for v, _ in groups.values()])
    pairs.tofile(d / "quot.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(d / "quot.out", dtype=QUOT_OUT)
    assert len(out) == len(pairs)
    return groups, pairs, out


@pytest.mark.gpu
def test_the_helper_returns_the_bits_of_the_division(quot_run):
    groups, pairs, out = quot_run
    ok = same_bits(out["q"], out["ref"])
    bad = np.flatnonzero(~ok)
    names = np.concatenate([[k] * len(v) for k, (v, _) in groups.items()])
    print(f"\n[quotient] {len(pairs)} pairs, {len(bad)} mismatches, {(out['path'] == Q.SHORT).sum()} by the short form, "
          f"{(out['path'] == Q.DIVIDED).sum()} divided")
    assert len(bad) == 0, (f"{len(bad)} mismatches; first in group {names[bad[0]]}: n {float(pairs[bad[0], 0]).hex()} a {float(pairs[bad[0], 1]).hex()} "
                           f"helper {float(out['q'][bad[0]]).hex()} n / a {float(out['ref'][bad[0]]).hex()} path {out['path'][bad[0]]}")
    # the device's division is the correctly rounded one: numpy's on the host gives the same bits
    with np.errstate(all="ignore"):
        host = pairs[:, 0] / pairs[:, 1]
    assert same_bits(out["ref"], host).all()
    assert (out["path"] == Q.SHORT).sum() >= 1 << 21


@pytest.mark.gpu
def test_every_group_takes_the_path_its_definition_implies(quot_run):
    groups, pairs, out = quot_run
    assert np.isin(out["path"], (Q.SHORT, Q.DIVIDED)).all(), "a lane that made no quotient, or more than one"
    # wave by wave, from frexp on the operands: the short form exactly when all 64 pairs are inside the range
    expect = np.where(Q.short_form_expected(pairs), Q.SHORT, Q.DIVIDED)
    wrong = np.flatnonzero(out["path"] != expect)
    assert len(wrong) == 0, f"{len(wrong)} pairs on the other path; first: n {float(pairs[wrong[0], 0]).hex()} a {float(pairs[wrong[0], 1]).hex()} path {out['path'][wrong[0]]}"
    at = 0
    for name, (v, path) in groups.items():
        got = out["path"][at:at + len(v)]
        assert (got == path).all(), f"group {name}: {(got != path).sum()} of {len(v)} pairs did not take path {path}"
        at += len(v)
        print(f"[quotient] {name}: {len(v)} pairs, all {'short' if path == Q.SHORT else 'divided'}")
