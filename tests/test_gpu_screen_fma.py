"""The f64 SCREEN kernels' box screen computes each slab distance as fma(bf, if, -fl(of * if)) (pathtrace.hpp screen_box_d):
  (a) on the device, on inputs aimed at that form's weak spots -- origins far from a box met at a steep angle (|o inv| >> |T|),
      |of if| near and beyond the f32 limit, a product below the normal f32 range, tmax ties -- every case the screen decides
      is Aabb::hit's decision, and |(hi32 - lo32) - (hi - lo)| <= TH / 1.5 in exact arithmetic;
  (b) on the CPU, the screened inner loop of the headline kernel (and of its ordered-tree twin) is compiled with one
      v_pk_fma_f32 per axis and the product hoisted out of it: no v_pk_add_f32 or v_pk_mul_f32 inside the loop.
Part (a) runs tests/walk_check.hip's box part; test_gpu_walk_primitives.py checks the same functions on the general corpus."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_corpus as W  # noqa: E402
from test_gpu_walk_primitives import BF_HIT64, BF_OVERFLOW, BF_SCREENED, BOX_OUT, aabb_oracle, build_walk_check, first_bad  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA_SRC = os.path.join(ROOT, "tests", "screen_isa.hip")
ISA_FLAGS = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-S",
             "-I", os.path.join(ROOT, "crucible_amd", "csrc")]
# the headline kernel (book1, f64, scene in LDS, relaxed sums) and the same kernel on an ordered tree (the second loop),
# with the vector instructions of a screened step (the ordered step adds the octant's hit link)
ISA_KERNELS = {"headline": ("double,RES_LDS,false,false,false,true,true", 21),
               "ordered": ("double,RES_LDS,false,true,false,true,true", 24)}


def _rows(b, o, d, tmax):
    return np.concatenate([b, o, d, np.asarray(tmax, dtype=np.float64).reshape(-1, 1)], axis=1)


def _tmax(rs, n, scale):
    return np.where(rs.uniform(size=n) < 0.7, np.inf, scale * 10.0 ** rs.uniform(-1, 1, n))


def _aim(rs, b, o, k, ulps):
    """Directions from o at a point on the surface of box b, times k, moved by up to `ulps` units in the last place."""
    p = W._surface_target(rs, b)
    d = (p - o) * k[:, None]
    return W.ulp_shift(d, rs.randint(-ulps, ulps + 1, d.shape) * 2 ** rs.randint(0, 30, (len(b), 1)))


def far_origin_steep(rs, n):
    """The origin near a box far from the world origin, at a steep angle: |o inv| up to 1e9 times the slab distances
    (the FMA form's 5u |inv o| term), kept near the band's edge."""
    out, got = [], 0
    while got < n:
        m = 200000
        scale = 10.0 ** rs.uniform(-3, 3, m)
        b = W._boxes(rs, m, scale, 10.0 ** rs.uniform(3, 9, m))
        ctr = (b[:, 0::2] + b[:, 1::2]) * 0.5
        o = ctr + W._unit(rs, m) * (scale * 10.0 ** rs.uniform(0, 2, m))[:, None]
        d = _aim(rs, b, o, 10.0 ** rs.uniform(-6, 6, m), 64)
        c = _rows(b, o, d, _tmax(rs, m, 10.0 ** rs.uniform(-6, 6, m)))
        lo, hi = W.interval_ref(c)
        with np.errstate(all="ignore"):
            q = np.abs(c[:, 6:9] / c[:, 9:12]).max(axis=1)
            keep = np.isfinite(hi - lo) & (np.abs(hi - lo) <= 2.0 ** -12 * (np.maximum(np.abs(lo), np.abs(hi)) + q))
        out.append(c[keep])
        got += keep.sum()
    return np.concatenate(out)[:n]


def product_near_f32_limit(rs, n):
    """|of if| between 2^124 and 2^131 on the origin's axes (the f32 limit is 2^128: beyond it p = inf, TH = inf and
    every test of the ray goes to the f64 band), |of| and |if| inside the screen's range."""
    e_o = rs.uniform(30, 100, n)
    e_q = rs.uniform(124, 131, n)
    o = W._unit(rs, n) * (2.0 ** e_o)[:, None]
    delta = W._unit(rs, n) * (2.0 ** (e_o + rs.uniform(-30, 4, n)))[:, None]
    half = np.abs(delta) * 10.0 ** rs.uniform(-3, 0, (n, 3))
    ctr = o + delta
    b = np.empty((n, 6))
    b[:, 0::2] = ctr - half
    b[:, 1::2] = ctr + half
    d0 = W.ulp_shift(W._surface_target(rs, b) - o, rs.randint(-64, 65, (n, 3)))
    # scale the direction so that |o| / |d| is 2^e_q: the largest |o_a inv_a| sits near 2^e_q
    d = d0 * (np.linalg.norm(o, axis=1) / np.linalg.norm(d0, axis=1) * 2.0 ** -e_q)[:, None]
    return _rows(b, o, d, _tmax(rs, n, 2.0 ** rs.uniform(0, 120, n)))


def subnormal_product(rs, n):
    """Origins at or below the smallest normal f32 (1e-46 .. 1e-36, some exactly 0): fl(of if) is subnormal or 0, and of
    itself may be subnormal -- the absolute terms of TH."""
    scale = 10.0 ** rs.uniform(-6, 6, n)
    b = W._boxes(rs, n, scale)
    o = rs.choice([-1.0, 1.0], (n, 3)) * 10.0 ** rs.uniform(-46, -36, (n, 3)) * (rs.uniform(size=(n, 3)) < 0.9)
    d = _aim(rs, b, o, 10.0 ** rs.uniform(-3, 3, n), 64)
    return _rows(b, o, d, _tmax(rs, n, scale * 10.0 ** rs.uniform(-3, 3, n)))


def fma_slabs32(c):
    """The screen's f32 slab distances, fma(bf, if, -fl(of if)), emulated: bf if is exact in f64; the difference is
    rounded to f64 and then to f32 (a double rounding -- good enough to aim tmax at them)."""
    with np.errstate(all="ignore"):
        c32 = c.astype(np.float32)
        if32 = (1.0 / c[:, 9:12]).astype(np.float32)
        p = c32[:, 6:9] * if32
        t = np.empty((len(c), 6), dtype=np.float32)
        for a in range(3):
            for s in range(2):
                t[:, 2 * a + s] = (c32[:, 2 * a + s].astype(np.float64) * if32[:, a] - p[:, a].astype(np.float64)).astype(np.float32)
    return t


def tmax_ties(rs, n):
    """far_origin_steep rays whose tmax is one of the slab distances -- f64, f32 or the screen's own FMA value -- or
    one unit in the last place (of its type) beside it."""
    c = far_origin_steep(rs, n)
    t64, _ = W.slabs(c)
    t32 = fma_slabs32(c)
    k = rs.randint(0, 6, n)
    ar = np.arange(n)
    kind = rs.randint(0, 3, n)
    step = rs.randint(-1, 2, n)
    with np.errstate(all="ignore"):
        tt64 = W.ulp_shift(np.abs(t64[ar, k]), step)
        tt32 = W.ulp_shift(np.abs(t32[ar, k]), step).astype(np.float64)
        tt32f = W.ulp_shift(np.abs(t64[ar, k]).astype(np.float32), step).astype(np.float64)
    c[:, 12] = np.where(kind == 0, tt64, np.where(kind == 1, tt32, tt32f))
    return c[np.isfinite(c[:, 12])]


def fma_corpus(seed=7):
    rs = np.random.RandomState(seed)
    return {
        "far_origin_steep": far_origin_steep(rs, 60000),
        "product_near_f32_limit": product_near_f32_limit(rs, 40000),
        "subnormal_product": subnormal_product(rs, 40000),
        "tmax_ties": tmax_ties(rs, 40000),
    }


@pytest.fixture(scope="module")
def fma_walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen_fma")
    exe = d / "walk_check"
    build_walk_check(exe)
    groups = fma_corpus()
    box = np.concatenate(list(groups.values()))
    names = np.concatenate([[k] * len(v) for k, v in groups.items()])
    box.tofile(d / "box.in")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return box, names, np.fromfile(d / "box.out", dtype=BOX_OUT)


@pytest.mark.gpu
def test_fma_screen_decides_as_aabb_hit_within_its_bound(fma_walk, o64):
    box, names, out = fma_walk
    f = out["flags"]
    ref = W.aabb_hit_ref(box)
    hit64 = (f & BF_HIT64) != 0
    assert np.array_equal(hit64, ref), first_bad(hit64 == ref, box, names, "box_hit<double> vs Aabb::hit")
    rs = np.random.RandomState(11)
    pick = rs.choice(len(box), 20000, replace=False)
    orc = aabb_oracle(o64, box[pick])
    assert np.array_equal(orc, ref[pick]), first_bad(orc == ref[pick], box[pick], names[pick], "numpy Aabb::hit vs oracle_aabb_hit")
    screened = ((f & BF_SCREENED) != 0) & ((f & BF_OVERFLOW) == 0)
    d, th = out["d"].astype(np.float64), out["th"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        decided = screened & (np.abs(d) > th)
    band = screened & ~decided
    ok = ~decided | ((d > 0) == ref)
    assert ok.all(), first_bad(ok, box, names, "FMA screen decision vs Aabb::hit",
                               lambda i: f"hi32-lo32 {float(out['d'][i]).hex()} TH {float(out['th'][i]).hex()} f64 hit {bool(ref[i])}")
    # |of if| beyond the f32 range on some axis: TH is infinite and the case is left to the f64 test
    with np.errstate(all="ignore"):
        q32 = np.abs(box[:, 6:9].astype(np.float32) * (1.0 / box[:, 9:12]).astype(np.float32))
    q_over = screened & np.isinf(q32).any(axis=1)
    assert not (q_over & decided).any(), first_bad(~(q_over & decided), box, names, "a ray with fl(of if) = inf decided in f32")
    # the bound in exact arithmetic: every decided case within 8 TH of the threshold (up to 6000 per group) and 1500 others
    # per group; hi - lo from the f64 slab distances (their own rounding, 2^-52 |T|, is far inside the factor 1.5)
    lo, hi = W.interval_ref(box)
    with np.errstate(all="ignore"):
        fin = screened & np.isfinite(d) & np.isfinite(th) & np.isfinite(lo) & np.isfinite(hi)
        close = fin & decided & (np.abs(d) <= 8 * th)
        m = np.maximum(np.abs(lo), np.abs(hi))
        near = decided & (np.abs(hi - lo) <= 2.0 ** -18 * m)
    sample = []
    for g in np.unique(names):
        c_idx, f_idx = np.flatnonzero(close & (names == g)), np.flatnonzero(fin & (names == g))
        sample.append(rs.choice(c_idx, min(len(c_idx), 6000), replace=False))
        sample.append(rs.choice(f_idx, min(len(f_idx), 1500), replace=False))
    sample = np.unique(np.concatenate(sample))
    worst, bad = 0.0, []
    for i in sample:
        err = abs(Fraction(float(out["d"][i])) - (Fraction(float(hi[i])) - Fraction(float(lo[i]))))
        lim = Fraction(float(out["th"][i]))
        if lim > 0:
            worst = max(worst, float(err / lim))
        if err * 3 > lim * 2:
            bad.append(i)
    print(f"\n[screen fma] {len(box)} box cases, {screened.sum()} screened, {band.sum()} in the band, {decided.sum()} decided "
          f"({close.sum()} within 8 TH of the threshold, {near.sum()} within 2^-18 M of the boundary), {q_over.sum()} with "
          f"fl(of if) = inf; {len(bad)} bound violations of {len(sample)} checked exactly (largest error / TH {worst:.3f})")
    for g in np.unique(names):
        sel = names == g
        print(f"[screen fma]   {g}: {sel.sum()} cases, {screened[sel].sum()} screened, {band[sel].sum()} band, "
              f"{decided[sel].sum()} decided, {close[sel].sum()} close")
    assert not bad, first_bad(~np.isin(np.arange(len(box)), bad), box, names, "error bound |(hi32 - lo32) - (hi - lo)| <= TH / 1.5",
                              lambda i: f"hi32-lo32 {float(out['d'][i]).hex()} TH {float(out['th'][i]).hex()} lo {lo[i].hex()} hi {hi[i].hex()}")
    # a passing run proves something only if every group is screened and reaches the band and the threshold
    for g in np.unique(names):
        sel = names == g
        assert screened[sel].sum() >= 1000 and band[sel].sum() >= 100, (g, screened[sel].sum(), band[sel].sum())
    assert close.sum() >= 2000 and q_over.sum() >= 1000 and worst > 0.01, (close.sum(), q_over.sum(), worst)


def _screened_loop(asm):
    """The instructions of the innermost loop that holds a v_pk_fma_f32, from its header to its back edge."""
    lines = asm.splitlines()
    first = next(i for i, l in enumerate(lines) if "v_pk_fma_f32" in l)
    # the header's label line, then its comment lines ("; =>    This Inner Loop Header: Depth=N")
    mark = max(i for i in range(first) if "This Inner Loop Header" in lines[i])
    head = max(i for i in range(mark + 1) if re.match(r"^\.LBB\w+:", lines[i]))
    label = lines[head].split(":")[0]
    back = next(i for i in range(first, len(lines)) if re.match(r"\s*s_cbranch_\w+\s+" + re.escape(label) + r"\s*$", lines[i]))
    body = [l.split(";")[0].strip() for l in lines[head + 1:back + 1]]
    return [l for l in body if l and not l.startswith((".", "#", ";"))]


@pytest.mark.parametrize("kernel", sorted(ISA_KERNELS))
def test_screened_loop_is_one_packed_fma_per_axis(tmp_path, kernel):
    out = tmp_path / f"{kernel}.s"
    args, step_valu = ISA_KERNELS[kernel]
    subprocess.run(ISA_FLAGS + [f"-DSCREEN_ISA_KERNEL={args}", "-o", str(out), ISA_SRC], check=True, timeout=600)
    loop = _screened_loop(out.read_text())
    ops = [l.split()[0] for l in loop]
    valu = [op for op in ops if op.startswith("v_")]
    assert ops.count("v_pk_fma_f32") == 3, loop
    assert "v_pk_add_f32" not in ops and "v_pk_mul_f32" not in ops, loop
    assert len(valu) <= step_valu, (len(valu), loop)
