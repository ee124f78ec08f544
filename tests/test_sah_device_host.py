"""The decision rules of the device-side SAH build on the CPU: tests/sah_device_check.cpp compiles the CR_HD functions of
crucible_amd/csrc/sah_device.hpp -- the ordered keys that skip a NaN, the centroid bounds, the bins, the cost of a plane
and the choice among the 45 -- with g++, and every inner wrapper of the model's trees (tests/sah_model.py) is put to
them: the bins of every primitive on every candidate axis, the axis, the plane and the size of the left side.  Exact,
as everything about this tree.  Once more with the program built under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import sah_model as M
from scenes import SAH_HAND as HAND
from test_gpu_sah_build import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (["r300", "subnormal_extent", "nan_centroid", "huge_1e300", "beyond_f32"] + [n for n in SCENES if n.startswith("concentric")] +
         ["hand_" + n for n in HAND])
REALS = [np.float64, np.float32]


def compile_check(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "sah_device_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sah_device_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def cases():
    """Per inner wrapper of every scene's model tree in both real types: (label, boxes (m, 6) f64 as lo xyz, hi xyz, in
    the order the range entered the wrapper, expected axis, plane, n_left, bins (m, 3))."""
    out = []
    for name in NAMES:
        flat = SCENES[name]().flatten()
        for real in REALS:
            t = M.build(flat, real, M.ORDERED)
            pos_of = {int(p): i for i, p in enumerate(t.vis)}
            pb = t.prim_boxes.astype(np.float64)
            for k in np.nonzero(t.children[:, 0] >= 0)[0]:
                pos = np.array(sorted(pos_of[int(p)] for p in t.order[t.start[k]:t.end[k]]))
                lo, hi = pb[pos][:, 0::2], pb[pos][:, 1::2]
                with np.errstate(all="ignore"):
                    cen = 0.5 * (lo + hi)
                    clo, chi = np.fmin.reduce(cen, axis=0), np.fmax.reduce(cen, axis=0)
                    ext = chi - clo
                    cand = (ext > 0.0) & np.isfinite(ext)
                    bins = np.where(cand[None, :], M.bin_index((cen - clo) * (16.0 / ext)), 0)
                left = t.children[k, 0]
                out.append((f"{name}/{real.__name__}/{k}", np.concatenate([lo, hi], axis=1), int(t.axis[k]), int(t.plane[k]),
                            int(t.end[left] - t.start[left]), bins))
    assert len(out) > 1000
    assert sum(c[3] == -1 for c in out) > 100                         # ranges with no winner
    with np.errstate(invalid="ignore"):
        assert sum(bool(np.isnan(0.5 * (c[1][:, :3] + c[1][:, 3:])).any()) for c in out) >= 1   # a centroid that is no number
    return out


def run(exe, cases, tmp_path):
    path = tmp_path / "ranges.bin"
    with open(path, "wb") as f:
        for _, boxes, *_ in cases:
            f.write(np.uint64(len(boxes)).tobytes())
            f.write(np.ascontiguousarray(boxes, dtype="<f8").tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()
    assert not res.stderr, res.stderr.decode()
    got = np.frombuffer(res.stdout, dtype="<i4")
    at = 0
    for label, boxes, axis, plane, n_left, bins in cases:
        m = len(boxes)
        assert got[at:at + 3].tolist() == [axis, plane, n_left], (label, got[at:at + 3].tolist(), [axis, plane, n_left])
        assert np.array_equal(got[at + 3:at + 3 + 3 * m].reshape(m, 3), bins), label
        at += 3 + 3 * m
    assert at == len(got)


def test_shared_rules_equal_the_model(cases, tmp_path):
    run(compile_check(tmp_path), cases, tmp_path)


def test_shared_rules_under_sanitizers(cases, tmp_path):
    """The same program with -fsanitize=address,undefined: no report, the same answers."""
    run(compile_check(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")), cases, tmp_path)
