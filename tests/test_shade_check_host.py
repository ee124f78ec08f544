"""CPU side of tests/test_gpu_shade_primitives.py: the device check program still compiles for gfx950 against the current
headers, and the refit rule of crucible_amd/csrc/refit.hpp -- compiled for the host through its __host__ __device__
functions, the same code the refit kernels run -- keeps every keyed primitive inside its box at every time the walk can
see, and is exactly the rule's union of sample boxes grown by timeline_pad, in f64 and f32.  The rule's soundness is then
guarded without a GPU."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_corpus as S  # noqa: E402
from test_gpu_shade_primitives import build_shade_check, check_refit, check_timeline  # noqa: E402


def test_shade_check_cross_compiles_for_gfx950(tmp_path):
    exe = tmp_path / "shade_check"
    build_shade_check(exe)
    assert exe.stat().st_size > 0


def test_refit_rule_contains_the_primitive_on_the_host(tmp_path, o64, o32):
    exe = tmp_path / "shade_check"
    build_shade_check(exe)
    d = S.anim_desc()
    d.write(tmp_path / "scene.bin")
    rf, rf_names = S.refit_rows(d)
    rf.tofile(tmp_path / "refit.in")
    tl, tl_names = S.timeline_rows(d)
    tl.tofile(tmp_path / "timeline.in")
    r = subprocess.run([str(exe), str(tmp_path), "--host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    load = lambda part, sfx, w: np.fromfile(tmp_path / f"{part}{sfx}.out", dtype=np.float64).reshape(-1, w)  # noqa: E731
    check_timeline(d, tl, tl_names, {s: load("timeline", s, 9) for s in ("64", "32")}, o64, o32)
    check_refit(d, rf, rf_names, {s: load("refit", s, 6) for s in ("64", "32")}, o64, o32, 100)
    # the corpus reaches the cases the rule once missed (opposite-sign keys, a centre moving while the radius shrinks,
    # zero-length keys at an interval's start) and extremes that only a key end or a left limit reaches
    for g in ("opposite_signs", "move_and_shrink", "zero_length", "scale_xyz", "key_end_extreme", "left_limit_extreme"):
        assert (rf_names == g).sum() > 50, g
