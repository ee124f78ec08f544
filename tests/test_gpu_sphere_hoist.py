"""Sphere::hit with the reciprocal of |d|^2 made once per segment, on the device (tests/sphere_hoist_check.hip runs walk_begin<true>
and sphere_t<.., true> of crucible_amd/csrc/pathtrace.hpp on the cases of tests/sphere_corpus.py): hit flag and bits of t must be those
of the same search with the switch off, of the reference's two divisions written out and, on a sample of every group, of the
oracle's Sphere::hit.  The corpus has directions scaled by 2^+-500 and 2^-540, zero directions and infinite / NaN operands, so
|d|^2 leaves the range the short quotient is proven for: the program reports per case how many quotients were made and how many
took the division, and the test refuses a run that does not reach both."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_corpus as Q  # noqa: E402
import test_gpu_sphere_roots as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sphere_hoist_check.hip")
HOIST_OUT = np.dtype([("t_on", "<f8"), ("t_off", "<f8"), ("t_ref", "<f8"), ("flags", "<u4"), ("quotients", "<u2"), ("divided", "<u2")])
HF_ON, HF_OFF, HF_REF, HF_A_ONLY_DIFF, HF_RDA_VALID = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def hoist_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("sphere_hoist")
    exe = d / "sphere_hoist_check"
    subprocess.run(R.HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)
    rows, names = R.corpus()
    rows.tofile(d / "sphere.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(d / "hoist.out", dtype=HOIST_OUT)
    assert len(out) == len(rows)
    return rows, names, out


@pytest.mark.gpu
def test_the_shared_reciprocal_changes_no_bit_of_sphere_t(hoist_run):
    rows, names, out = hoist_run
    assert len(rows) >= 1 << 20, len(rows)
    on, off, ref = ((out["flags"] & b) != 0 for b in (HF_ON, HF_OFF, HF_REF))
    for what, h, t in (("the switch off", off, out["t_off"]), ("the two divisions", ref, out["t_ref"])):
        ok = (on == h) & (~h | R.same_bits(out["t_on"], t))
        assert ok.all(), R.first_bad(ok, rows, names, f"sphere_t with the shared reciprocal vs {what}",
                                     lambda i: f"shared hit {on[i]} t {float(out['t_on'][i]).hex()}, {what} hit {h[i]} t {float(t[i]).hex()}")
    same = (out["flags"] & HF_A_ONLY_DIFF) == 0
    assert same.all(), R.first_bad(same, rows, names, "sphere_t<false, true> vs sphere_t<true, true>")
    # walk_begin<true> leaves a reciprocal exactly where |d|^2, as the device sums it, is inside the range
    d = rows[:, 7:10]
    with np.errstate(all="ignore"):
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    valid = (out["flags"] & HF_RDA_VALID) != 0
    assert np.array_equal(valid, Q.in_range(dd)), R.first_bad(valid == Q.in_range(dd), rows, names, "validity of the reciprocal vs frexp(|d|^2)")
    # both paths are reached, by hits and by misses, for the first root and for the second
    q, dv = out["quotients"].astype(int), out["divided"].astype(int)
    assert (dv <= q).all() and (q <= 2).all()
    short = (q > 0) & (dv == 0)
    print(f"\n[sphere hoist] {len(rows)} cases, {on.sum()} hits, 0 mismatches; quotients {q.sum()}, divided {dv.sum()}; cases all short {short.sum()} "
          f"(hits {(short & on).sum()}, two quotients {(short & (q == 2)).sum()}), cases that divided {(dv > 0).sum()} (hits {((dv > 0) & on).sum()}); "
          f"|d|^2 outside the range in {(~valid).sum()} cases, {(~valid & (q > 0)).sum()} of them reached a quotient")
    assert (short & on).sum() >= 1000 and (short & (q == 2) & on).sum() >= 100, "the short form is not reached by hits of both roots"
    assert ((dv > 0) & on).sum() >= 100 and (~valid & (dv > 0)).sum() >= 100, "the division is not reached (by hits, by |d|^2 outside the range)"
    # a case whose reciprocal is the sentinel never takes the short form
    assert (dv[~valid] == q[~valid]).all()


@pytest.mark.gpu
def test_the_shared_reciprocal_equals_the_oracle_in_every_group(hoist_run, o64):
    rows, names, out = hoist_run
    rs = np.random.RandomState(11)
    pick = []
    for g in dict.fromkeys(names):
        idx = np.flatnonzero(names == g)
        pick.append(idx if len(idx) <= R.ORACLE_PER_GROUP else np.sort(rs.choice(idx, R.ORACLE_PER_GROUP, replace=False)))
    pick = np.concatenate(pick)
    h, t = R.sphere_oracle(o64, rows[pick])
    hit, got = (out["flags"][pick] & HF_ON) != 0, out["t_on"][pick]
    ok = (hit == h) & (~h | R.same_bits(got, t))
    assert ok.all(), R.first_bad(ok, rows[pick], names[pick], "sphere_t with the shared reciprocal vs oracle_sphere_hit",
                                 lambda i: f"device hit {hit[i]} t {float(got[i]).hex()}, oracle hit {h[i]} t {float(t[i]).hex()}")
    print(f"\n[sphere hoist] {len(pick)} cases of {len(set(names))} groups against the oracle, {h.sum()} hits, 0 mismatches")
