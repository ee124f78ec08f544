"""Sphere::hit's root search on the device (tests/sphere_roots_check.hip runs sphere_t of crucible_amd/csrc/pathtrace.hpp;
tests/sphere_corpus.py makes the cases): sphere_t decides the second root without dividing where rule A or rule B of its comment
proves the outcome, and must return the hit flag and the bits of t of the reference's two-division search -- written out in the
check program and, on a sample of every group, the oracle's Sphere::hit -- in f64 and in f32.  The check program also reports
where each case left sphere_t, and the test refuses a corpus that does not reach rule A, rule B and the division."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sphere_corpus as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "crucible_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "sphere_roots_check.hip")
SPHERE_OUT = np.dtype([("t64", "<f8"), ("ref64", "<f8"), ("t32", "<f4"), ("ref32", "<f4"), ("flags", "<u4"), ("path", "<u4")])
SF_HIT64, SF_REF64, SF_HIT32, SF_REF32, SF_A_ONLY_DIFF64, SF_A_ONLY_DIFF32 = 1, 2, 4, 8, 16, 32
ORACLE_PER_GROUP = 12000   # cases of every group handed to the oracle (one call each)


def build_sphere_roots_check(exe):
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)


def corpus():
    groups = S.sphere_corpus()
    rows = np.concatenate(list(groups.values()))
    names = np.concatenate([[k] * len(v) for k, v in groups.items()])
    return rows, names


def same_bits(a, b):
    it = np.uint64 if a.dtype == np.float64 else np.uint32
    return (a.view(it) == b.view(it)) | (np.isnan(a) & np.isnan(b))


def first_bad(ok, rows, names, what, extra=None):
    bad = np.flatnonzero(~ok)
    if len(bad) == 0:
        return ""
    i = bad[0]
    msg = (f"{what}: {len(bad)} mismatches; first in group {names[i]}: row (centre, radius, origin, direction, tmax) = "
           + " ".join(float(v).hex() for v in rows[i]))
    return msg + ("; " + extra(i) if extra is not None else "")


def sphere_oracle(o, rows):
    """(hit, t) of the oracle's Sphere::hit in its precision, on the rows rounded to it."""
    with np.errstate(over="ignore"):
        r = np.ascontiguousarray(rows.astype(o.np_real))
    out = np.zeros(10, dtype=o.np_real)
    hit = np.zeros(len(r), dtype=bool)
    t = np.zeros(len(r), dtype=o.np_real)
    p_out, base, sz, R = out.ctypes.data_as(C.c_void_p), r.ctypes.data, r.itemsize, o.real
    for i in range(len(r)):
        row = base + i * 11 * sz
        if o.lib.oracle_sphere_hit(C.c_void_p(row), C.c_void_p(row + 4 * sz), C.c_void_p(row + 7 * sz), R(S.TMIN), R(r[i, 10]), p_out):
            hit[i] = True
            t[i] = out[0]
    return hit, t


@pytest.fixture(scope="module")
def sphere_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("sphere_roots")
    exe = d / "sphere_roots_check"
    build_sphere_roots_check(exe)
    rows, names = corpus()
    rows.tofile(d / "sphere.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(d / "sphere.out", dtype=SPHERE_OUT)
    assert len(out) == len(rows)
    return rows, names, out


PRECISIONS = ((np.float64, "t64", "ref64", SF_HIT64, SF_REF64, 0), (np.float32, "t32", "ref32", SF_HIT32, SF_REF32, 8))


@pytest.mark.gpu
def test_sphere_t_equals_the_two_division_search_bit_for_bit(sphere_run):
    rows, names, out = sphere_run
    assert len(rows) >= 1 << 20, len(rows)
    for dt, tf, rf, hb, rb, shift in PRECISIONS:
        hit, ref = (out["flags"] & hb) != 0, (out["flags"] & rb) != 0
        ok = (hit == ref) & (~ref | same_bits(out[tf], out[rf]))
        assert ok.all(), first_bad(ok, rows, names, f"sphere_t<{dt.__name__}> vs the two divisions on the device",
                                   lambda i: f"sphere_t hit {hit[i]} t {float(out[tf][i]).hex()}, two divisions hit {ref[i]} t {float(out[rf][i]).hex()}")
        # sphere_t<false>, rule A alone (the kernels that read their tree from global memory), returns the same
        same = (out["flags"] & (SF_A_ONLY_DIFF64 if dt == np.float64 else SF_A_ONLY_DIFF32)) == 0
        assert same.all(), first_bad(same, rows, names, f"sphere_t<false, {dt.__name__}> vs sphere_t")
        path = ((out["path"] >> shift) & 0xFF).astype(np.uint8)
        print(f"\n[sphere roots] {dt.__name__}: {len(rows)} cases, {ref.sum()} hits, 0 mismatches; second division skipped in "
              f"{((path == S.P_RULE_A) | (path == S.P_RULE_B)).sum()} of {(path >= S.P_RULE_A).sum()} cases whose first root was out of range")
        print(S.coverage_table(names, path))
        # the exits the program reports are consistent with what it returned, and the corpus reaches every one of them
        assert np.array_equal(hit, (path == S.P_ROOT1) | (path == S.P_DIV_HIT))
        S.check_coverage(names, path, hit, f"device, {dt.__name__}")
        # the numpy model of both forms (tests/test_sphere_roots_host.py runs it without a GPU) describes the device
        # (where root2 is NaN the exit -- rule B or the division, a miss either way -- may turn on the sign of a NaN, which
        # is the machine's choice)
        m_old, mt_old, m_new, mt_new, m_path, (_, m_root2) = S.model(rows, dt)
        ok = (m_new == hit) & (~hit | same_bits(mt_new.astype(dt), out[tf])) & ((m_path == path) | np.isnan(m_root2))
        assert ok.all(), first_bad(ok, rows, names, f"numpy model ({dt.__name__}) vs the device",
                                   lambda i: f"model hit {m_new[i]} path {m_path[i]}, device hit {hit[i]} path {path[i]}")


@pytest.mark.gpu
def test_sphere_t_equals_the_oracle_in_every_group(sphere_run, o64, o32):
    rows, names, out = sphere_run
    rs = np.random.RandomState(11)
    pick = []
    for g in dict.fromkeys(names):
        idx = np.flatnonzero(names == g)
        pick.append(idx if len(idx) <= ORACLE_PER_GROUP else np.sort(rs.choice(idx, ORACLE_PER_GROUP, replace=False)))
    pick = np.concatenate(pick)
    for o, (dt, tf, rf, hb, rb, shift) in zip((o64, o32), PRECISIONS):
        h, t = sphere_oracle(o, rows[pick])
        hit, got = (out["flags"][pick] & hb) != 0, out[tf][pick]
        ok = (hit == h) & (~h | same_bits(got, t.astype(dt)))
        assert ok.all(), first_bad(ok, rows[pick], names[pick], f"sphere_t<{dt.__name__}> vs oracle_sphere_hit",
                                   lambda i: f"device hit {hit[i]} t {float(got[i]).hex()}, oracle hit {h[i]} t {float(t[i]).hex()}")
        path = ((out["path"][pick] >> shift) & 0xFF).astype(np.uint8)
        S.check_coverage(names[pick], path, hit, f"oracle sample, {dt.__name__}")
        print(f"\n[sphere roots] {dt.__name__}: {len(pick)} cases of {len(set(names))} groups against the oracle, {h.sum()} hits, 0 mismatches")
