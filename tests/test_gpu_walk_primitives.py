"""The walk's per-ray decisions on the device, one primitive at a time (tests/walk_check.hip runs the functions of
crucible_amd/csrc/pathtrace.hpp; tests/walk_corpus.py makes the inputs):
  (a) the f64 SCREEN kernels' f32 box screen against Aabb::hit, and its error bound (TH) against exact arithmetic;
  (b) the f32 kernels' record test and the min/max fast forms against Aabb::hit, bit for bit;
  (c) sphere_t and triangle_t against the oracle's Sphere::hit / Triangle::hit, f64 and f32;
  (d) the screened rejection samplers against the plain loops, draw for draw;
  (e) the software atan2 / asin / acos against the oracle's, bit for bit.
The renders of the parity tests almost never put a ray within 2^-20 of a box edge; these inputs do."""
import ctypes as C
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
SRC = os.path.join(ROOT, "tests", "walk_check.hip")

BOX_OUT = np.dtype([("d", "<f4"), ("th", "<f4"), ("flags", "<u4")])
PRIM_OUT = np.dtype([("t64", "<f8"), ("t32", "<f4"), ("flags", "<u4")])
(BF_SCREENED, BF_EXACT64, BF_HIT64, BF_FAST_HIT64, BF_FAST_MISS64, BF_EXACT32, BF_HIT32, BF_FAST_HIT32, BF_FAST_MISS32,
 BF_REC_MISS32, BF_OVERFLOW) = (1 << k for k in range(11))
SAMPLER_KEYS = 1 << 24


def build_walk_check(exe):
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)


def hexrow(row):
    return " ".join(float(v).hex() for v in row)


def first_bad(ok, rows, names, what, extra=None):
    """Assertion message for the first row where `ok` is false."""
    bad = np.flatnonzero(~ok)
    if len(bad) == 0:
        return ""
    i = bad[0]
    msg = f"{what}: {len(bad)} mismatches; first in group {names[i]}: row (box x0 x1 y0 y1 z0 z1, o, d, tmax / prim) = {hexrow(rows[i])}"
    if extra is not None:
        msg += "; " + extra(i)
    return msg


def prim_oracle(o, rows):
    """(hit, t) of the oracle's Sphere::hit / Triangle::hit for every row, in the oracle's precision (inputs rounded to it)."""
    with np.errstate(over="ignore"):   # beyond FLT_MAX: inf in f32, as on the device
        r = rows.astype(o.np_real)
    out = np.zeros(10, dtype=o.np_real)
    hit = np.zeros(len(rows), dtype=bool)
    t = np.zeros(len(rows), dtype=o.np_real)
    R = o.real
    p_out = out.ctypes.data_as(C.c_void_p)
    base = r.ctypes.data
    sz = r.itemsize
    for i in range(len(r)):
        row = base + i * 17 * sz
        fn = o.lib.oracle_sphere_hit if rows[i, 0] == 0 else o.lib.oracle_triangle_hit
        if fn(C.c_void_p(row + sz), C.c_void_p(row + 10 * sz), C.c_void_p(row + 13 * sz), R(W.TMIN), R(r[i, 16]), p_out):
            hit[i] = True
            t[i] = out[0]
    return hit, t


def aabb_oracle(o, rows):
    with np.errstate(over="ignore"):   # beyond FLT_MAX: inf in f32, as on the device
        r = rows.astype(o.np_real)
    base, sz, R = r.ctypes.data, r.itemsize, o.real
    res = np.zeros(len(r), dtype=bool)
    for i in range(len(r)):
        row = base + i * 13 * sz
        res[i] = o.lib.oracle_aabb_hit(C.c_void_p(row), C.c_void_p(row + 6 * sz), C.c_void_p(row + 9 * sz), R(W.TMIN), R(r[i, 12])) != 0
    return res


@pytest.fixture(scope="module")
def walk(tmp_path_factory, o64, o32):
    """One run of walk_check on every part's inputs."""
    d = tmp_path_factory.mktemp("walk_check")
    exe = d / "walk_check"
    build_walk_check(exe)
    groups = W.box_corpus(1)
    box = np.concatenate(list(groups.values()))
    names = np.concatenate([[k] * len(v) for k, v in groups.items()])
    # prims: the corpus, then tmax ties with the oracle's own t (f64 and f32 t, +-1 ulp)
    prim = W.prim_corpus()
    h64, t64 = prim_oracle(o64, prim)
    h32, t32 = prim_oracle(o32, prim)
    ties = []
    for h, t, dt in ((h64, t64, np.float64), (h32, t32, np.float32)):
        for step in (-1, 0, 1):
            tie = prim[h].copy()
            tie[:, 16] = W.ulp_shift(t[h].astype(dt), step).astype(np.float64)
            ties.append(tie[::3])
    prim = np.concatenate([prim] + ties)
    ty, tx = W.trig_inputs()
    box.tofile(d / "box.in")
    prim.tofile(d / "prim.in")
    np.stack([ty, tx], axis=1).astype(np.float64).tofile(d / "trig.in")
    np.array([SAMPLER_KEYS, 0x5EED0000], dtype=np.uint64).tofile(d / "sampler.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return {
        "box": box, "names": names, "box_out": np.fromfile(d / "box.out", dtype=BOX_OUT),
        "prim": prim, "prim_out": np.fromfile(d / "prim.out", dtype=PRIM_OUT),
        "trig_in": (ty, tx), "trig64": np.fromfile(d / "trig64.out", dtype=np.float64).reshape(-1, 3),
        "trig32": np.fromfile(d / "trig32.out", dtype=np.float32).reshape(-1, 3),
        "sampler": np.fromfile(d / "sampler.out", dtype=np.uint64),
    }


def _screen_inputs(box):
    with np.errstate(all="ignore"):
        inv = 1.0 / box[:, 9:12]
    if32 = np.abs(inv.astype(np.float32))
    of32 = np.abs(box[:, 6:9].astype(np.float32))
    exact = np.isinf(inv).any(axis=1)
    in_range = (if32.min(axis=1) >= np.float32(2.0 ** -100)) & (if32.max(axis=1) <= np.float32(2.0 ** 100)) & \
               (of32.max(axis=1) <= np.float32(2.0 ** 100))
    return exact, ~exact & in_range


@pytest.mark.gpu
def test_f64_screen_decides_as_aabb_hit_within_its_bound(walk, o64):
    box, names, out = walk["box"], walk["names"], walk["box_out"]
    f = out["flags"]
    ref = W.aabb_hit_ref(box)
    hit64 = (f & BF_HIT64) != 0
    assert np.array_equal(hit64, ref), first_bad(hit64 == ref, box, names, "box_hit<double> vs Aabb::hit")
    exact, screened_ref = _screen_inputs(box)
    assert np.array_equal((f & BF_SCREENED) != 0, screened_ref), first_bad(((f & BF_SCREENED) != 0) == screened_ref, box, names, "screen range predicate")
    # a record with a finite plane beyond the f32 range makes the host walk the whole tree without the screen
    with np.errstate(over="ignore"):
        overflow_ref = (np.isfinite(box[:, :6]) & np.isinf(box[:, :6].astype(np.float32))).any(axis=1)
    overflow = (f & BF_OVERFLOW) != 0
    assert np.array_equal(overflow, overflow_ref), first_bad(overflow == overflow_ref, box, names, "screen_plane overflow flag")
    screened = screened_ref & ~overflow
    # the recorded case: the screen on such a record decides a hit that Aabb::hit misses
    k = np.flatnonzero(names == "overflow_miss")[0]
    assert overflow[k] and not ref[k] and out["d"][k] > out["th"][k], (out["d"][k], out["th"][k], ref[k])
    d, th = out["d"].astype(np.float64), out["th"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        decided = screened & (np.abs(d) > th)
    band = screened & ~decided
    ok = ~decided | ((d > 0) == ref)
    assert ok.all(), first_bad(ok, box, names, "f32 screen decision vs Aabb::hit",
                               lambda i: f"hi32-lo32 {float(out['d'][i]).hex()} TH {float(out['th'][i]).hex()} f64 hit {bool(ref[i])}")
    # the oracle itself on a sample: every exact_box ray, every band case up to 20000, 20000 others
    rs = np.random.RandomState(3)
    pick = np.concatenate([np.flatnonzero(exact)[:20000], np.flatnonzero(band)[:20000], rs.choice(len(box), 20000, replace=False)])
    orc = aabb_oracle(o64, box[pick])
    assert np.array_equal(orc, hit64[pick]), first_bad(orc == hit64[pick], box[pick], names[pick], "box_hit<double> vs oracle_aabb_hit")
    # the bound itself: |(hi32 - lo32) - (hi - lo)| <= TH / 1.5, hi - lo exact from the f64 slab distances
    lo, hi = W.interval_ref(box)
    with np.errstate(all="ignore"):
        m = np.maximum(np.abs(lo), np.abs(hi))
        near = decided & (np.abs(hi - lo) <= 2.0 ** -18 * m)
        fin = screened & np.isfinite(d) & np.isfinite(th) & np.isfinite(lo) & np.isfinite(hi)
    sample = []
    for g in np.unique(names):
        idx = np.flatnonzero(fin & (names == g))
        if len(idx):
            sample.append(rs.choice(idx, min(len(idx), 8000), replace=False))
    sample = np.concatenate(sample)
    worst, bad = 0.0, []
    for i in sample:
        err = abs(Fraction(float(out["d"][i])) - (Fraction(float(hi[i])) - Fraction(float(lo[i]))))
        lim = Fraction(float(out["th"][i]))
        if lim > 0:
            worst = max(worst, float(err / lim))
        if err * 3 > lim * 2:
            bad.append(i)
    print(f"\n[walk (a)] {len(box)} box cases, {screened.sum()} screened, {band.sum()} in the band, {decided.sum()} decided, "
          f"{near.sum()} decided within 2^-18 M of the boundary, {len(bad)} bound violations of {len(sample)} checked exactly "
          f"(largest error / TH {worst:.3f}); random set: {band[names == 'random'].sum()} of {(screened & (names == 'random')).sum()} "
          f"screened cases in the band")
    for g in np.unique(names):
        sel = names == g
        print(f"[walk (a)]   {g}: {sel.sum()} cases, {screened[sel].sum()} screened, {band[sel].sum()} band")
    assert not bad, first_bad(~np.isin(np.arange(len(box)), bad), box, names, "error bound |(hi32 - lo32) - (hi - lo)| <= TH / 1.5",
                              lambda i: f"hi32-lo32 {float(out['d'][i]).hex()} TH {float(out['th'][i]).hex()} lo {lo[i].hex()} hi {hi[i].hex()}")
    # a passing run proves something only if the corpus reaches the band and the boundary
    assert band.sum() >= 5000, band.sum()
    assert near.sum() >= 1000, near.sum()
    assert worst > 0.01, worst


@pytest.mark.gpu
def test_f32_record_test_and_fast_forms_equal_aabb_hit(walk, o32):
    box, names, f = walk["box"], walk["names"], walk["box_out"]["flags"]
    with np.errstate(all="ignore"):
        exact32_ref = np.isinf(np.float32(1) / box[:, 9:12].astype(np.float32)).any(axis=1)
    exact64_ref, _ = _screen_inputs(box)
    exact32, exact64 = (f & BF_EXACT32) != 0, (f & BF_EXACT64) != 0
    assert np.array_equal(exact64, exact64_ref), first_bad(exact64 == exact64_ref, box, names, "walk_begin<double> exact_box")
    assert np.array_equal(exact32, exact32_ref), first_bad(exact32 == exact32_ref, box, names, "walk_begin<float> exact_box")
    ref32 = W.aabb_hit_ref(box, np.float32)
    hit32 = (f & BF_HIT32) != 0
    assert np.array_equal(hit32, ref32), first_bad(hit32 == ref32, box, names, "box_hit<float> vs Aabb::hit in f32")
    rec_hit = (f & BF_REC_MISS32) == 0
    ok = exact32 | (rec_hit == ref32)
    assert ok.all(), first_bad(ok, box, names, "f32 kernels' record test (screen_box_miss_exact) vs Aabb::hit in f32")
    hit64 = (f & BF_HIT64) != 0
    for name, bit, want, ex in (("box_hit_fast<double>", BF_FAST_HIT64, hit64, exact64), ("box_miss_fast<double>", BF_FAST_MISS64, ~hit64, exact64),
                                ("box_hit_fast<float>", BF_FAST_HIT32, hit32, exact32), ("box_miss_fast<float>", BF_FAST_MISS32, ~hit32, exact32)):
        got = (f & bit) != 0
        ok = ex | (got == want)
        assert ok.all(), first_bad(ok, box, names, name + " vs box_hit")
    rs = np.random.RandomState(4)
    pick = np.concatenate([np.flatnonzero(exact32)[:20000], rs.choice(len(box), 20000, replace=False)])
    orc = aabb_oracle(o32, box[pick])
    assert np.array_equal(orc, hit32[pick]), first_bad(orc == hit32[pick], box[pick], names[pick], "box_hit<float> vs oracle_aabb_hit (f32)")
    print(f"\n[walk (b)] {len(box)} box cases: exact_box {exact64.sum()} (f64) / {exact32.sum()} (f32), 0 mismatches")


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    it = np.uint64 if a.dtype == np.float64 else np.uint32
    return (a.view(it) == b.view(it)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.gpu
def test_sphere_and_triangle_match_the_oracle_bit_for_bit(walk, o64, o32):
    prim, out = walk["prim"], walk["prim_out"]
    names = np.where(prim[:, 0] == 0, "sphere", "triangle")
    for o, bit, field, dt in ((o64, 1, "t64", np.float64), (o32, 2, "t32", np.float32)):
        h, t = prim_oracle(o, prim)
        got_h = (out["flags"] & bit) != 0
        got_t = out[field]
        ok = (got_h == h) & (~h | _same_bits(got_t, t.astype(dt)))
        assert ok.all(), first_bad(ok, prim, names, f"sphere_t / triangle_t ({dt.__name__}) vs oracle",
                                   lambda i: f"device hit {got_h[i]} t {float(got_t[i]).hex()}, oracle hit {h[i]} t {float(t[i]).hex()}")
        print(f"\n[walk (c)] {dt.__name__}: {len(prim)} cases ({(prim[:, 0] == 0).sum()} spheres), {h.sum()} hits, 0 mismatches")


@pytest.mark.gpu
def test_screened_samplers_match_the_plain_loops(walk):
    mis_uv, mis_disk, band_uv, band_disk, first_uv, first_disk, rounds_uv, rounds_disk = (int(v) for v in walk["sampler"])
    print(f"\n[walk (d)] {SAMPLER_KEYS} stream keys: unit vector {rounds_uv} rounds, {band_uv} in the f64 band, {mis_uv} mismatches; "
          f"disk {rounds_disk} rounds, {band_disk} in the band, {mis_disk} mismatches")
    assert mis_uv == 0, f"random_unit_vector_dev<double> differs from random_unit_vector in {mis_uv} streams; first key index {first_uv:#x}"
    assert mis_disk == 0, f"random_in_unit_disk_dev<double> differs from the plain loop in {mis_disk} streams; first key index {first_disk:#x}"
    assert band_uv >= 300 and band_disk >= 300, (band_uv, band_disk)


@pytest.mark.gpu
def test_software_trig_matches_the_oracle_bit_for_bit(walk, o64, o32):
    ty, tx = walk["trig_in"]
    rows = np.stack([ty, tx], axis=1)
    names = np.array(["trig"] * len(ty))
    for o, got, dt in ((o64, walk["trig64"], np.float64), (o32, walk["trig32"], np.float32)):
        o.set_libm(False)
        ref = o.trig(ty.astype(dt), tx.astype(dt))
        for k, fn in enumerate(("atan2(y, x)", "asin(y)", "acos(y)")):
            ok = _same_bits(got[:, k], ref[k])
            assert ok.all(), first_bad(ok, rows, names, f"soft {fn} ({dt.__name__}) vs oracle_trig",
                                       lambda i: f"device {float(got[i, k]).hex()} oracle {float(ref[k][i]).hex()}")
    print(f"\n[walk (e)] {len(ty)} inputs x 3 functions x 2 precisions, 0 mismatches")
