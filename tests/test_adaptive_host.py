"""crucible_amd/csrc/adaptive.hpp, the arithmetic the adaptive judge kernel shares with the host, checked without a device:
tests/adaptive_check.cpp compiles the header with g++ (plain, and with -fsanitize=address,undefined) and prints, per block of
a constructed pair of accumulators, the block's rectangle, D_b, T_b and the verdict; tests/adaptive_model.py (Python
integers) says what they must be.  The cases: D_b == T_b stops and D_b == T_b + 1 does not, the >> 12 truncation per term,
a partial edge block's N_b, a NaN flag that stays out of the magnitude, tolerance 0, a tolerance whose product passes 2^63
(and one whose product is infinite), and a scale below 2^52 (samples = 4096)."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BLOCK = 21, 11, 8   # blocks of 8: three columns (8, 8, 5 wide), two rows (8, 3 high)
RECTS = M.blocks_of(W, H, BLOCK)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("adaptive_check")
    built = []
    for tag, extra in (("plain", ()), ("san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        exe = str(out / f"adaptive_check_{tag}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "adaptive_check.cpp")])
        built.append(exe)
    return built


def run(exes, tmp_path, E, O, S, qP, tolerance):
    """The program's lines for the accumulators E, O (H, W, 3) uint64: {block: (x0, y0, bw, bh, D, T, stops)}; both builds agree."""
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(f"{W} {H} 3 {S} {qP} {float(tolerance).hex()}\n")
        for e, o in zip(E.reshape(-1).tolist(), O.reshape(-1).tolist()):
            f.write(f"{e:x} {o:x}\n")
    outs = []
    for exe in exes:
        res = subprocess.run([exe, path], capture_output=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (exe, res.returncode, res.stderr.decode())
        outs.append(res.stdout.decode())
    assert outs[0] == outs[1]
    got = {}
    for line in outs[0].splitlines():
        v = [int(x) for x in line.split()]
        got[v[0]] = tuple(v[1:])
    return got


def base(seed=5):
    """Equal accumulators: D_b = 0 everywhere."""
    rng = np.random.default_rng(seed)
    E = rng.integers(1 << 40, 1 << 54, size=(H, W, 3), dtype=np.uint64)
    return E, E.copy()


def check_against_model(got, E, O, S, qP, tolerance):
    assert sorted(got) == list(range(len(RECTS)))
    for b, (x0, y0, w, h) in enumerate(RECTS):
        D = M.difference(E[y0:y0 + h, x0:x0 + w], O[y0:y0 + h, x0:x0 + w])
        T = M.threshold(tolerance, S, qP, w * h)
        assert got[b] == (x0, y0, w, h, D, T, 1 if D <= T else 0), (b, got[b], D, T)


def test_geometry_threshold_edge_and_truncation(exes, tmp_path):
    S, qP, tol = 52, 2, 1e-3
    E, O = base()
    T = [M.threshold(tol, S, qP, w * h) for _, _, w, h in RECTS]
    assert [w * h for _, _, w, h in RECTS] == [64, 64, 40, 24, 24, 15]   # partial edge blocks: N_b enters T_b
    assert len(set(T)) == 4 and all(0 < t < 1 << 51 for t in T)
    # block 0: D == T exactly, in one term, with the twelve bits below the shift all set (they must not count)
    O[0, 0, 0] = E[0, 0, 0] + np.uint64((T[0] << 12) | 0xFFF)
    # block 1: D == T + 1, the excess in a second term and the larger word on the other side
    O[1, 9, 1] = E[1, 9, 1] + np.uint64(T[1] << 12)
    E[2, 10, 2] = O[2, 10, 2] + np.uint64(1 << 12)
    # block 2 (5 wide): two terms of 0xFFF each -- shifted per term they are 0 + 0, shifted after the sum they would be 1
    O[3, 17, 0] = E[3, 17, 0] + np.uint64(0xFFF)
    O[4, 18, 1] = E[4, 18, 1] + np.uint64(0xFFF)
    # block 3 (3 high): D == T with N_b = 24; block 5 (5 x 3): D == T + 1 with N_b = 15
    O[8, 0, 0] = E[8, 0, 0] + np.uint64(T[3] << 12)
    O[10, 20, 2] = E[10, 20, 2] + np.uint64((T[5] + 1) << 12)
    # block 4: a NaN flag on one side only, over equal magnitudes: not part of the magnitude
    E[9, 12, 1] |= M.FLAG
    got = run(exes, tmp_path, E, O, S, qP, tol)
    check_against_model(got, E, O, S, qP, tol)
    assert [got[b][4] for b in range(6)] == [T[0], T[1] + 1, 0, T[3], 0, T[5] + 1]
    assert [got[b][6] for b in range(6)] == [1, 0, 1, 1, 1, 0]


def test_tolerance_zero(exes, tmp_path):
    S, qP = 52, 4
    E, O = base(6)
    O[0, 0, 0] = E[0, 0, 0] + np.uint64(4095)    # block 0: below the shift, D = 0: stops
    O[0, 8, 0] = E[0, 8, 0] + np.uint64(4096)    # block 1: D = 1 > 0: stays
    got = run(exes, tmp_path, E, O, S, qP, 0.0)
    check_against_model(got, E, O, S, qP, 0.0)
    assert all(got[b][5] == 0 for b in got)
    assert [got[b][6] for b in range(6)] == [1, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("tol", [1e300, 1.7e308, 2.0 ** 63, 1e6])
def test_product_beyond_2_63_stops_everything(exes, tmp_path, tol):
    S, qP = 52, 2
    rng = np.random.default_rng(8)
    E = rng.integers(0, 1 << 62, size=(H, W, 3), dtype=np.uint64)    # D_b as large as the words allow: below 2^12 * 2^50
    O = rng.integers(0, 1 << 62, size=(H, W, 3), dtype=np.uint64)
    got = run(exes, tmp_path, E, O, S, qP, tol)
    check_against_model(got, E, O, S, qP, tol)
    assert all(got[b][5] == 1 << 63 and got[b][6] == 1 for b in got)


def test_scale_below_2_52(exes, tmp_path):
    """samples = 4096: S = 50, so the weight is 2^38 * qP * 3 N_b."""
    S = M.fx_log2(4096)
    assert S == 50 and M.fx_log2(2047) == 52 and M.fx_log2(2048) == 51
    qP, tol = 256, 3e-4
    E, O = base(9)
    T = [M.threshold(tol, S, qP, w * h) for _, _, w, h in RECTS]
    assert T[0] == int(np.floor(tol * float((256 * 3 * 64) << 38)))
    O[0, 0, 0] = E[0, 0, 0] + np.uint64(T[0] << 12)
    O[0, 8, 0] = E[0, 8, 0] + np.uint64((T[1] + 1) << 12)
    got = run(exes, tmp_path, E, O, S, qP, tol)
    check_against_model(got, E, O, S, qP, tol)
    assert [got[b][6] for b in range(6)] == [1, 0, 1, 1, 1, 1]
