"""CPU side of tests/test_gpu_sphere_roots.py: the device check program still compiles for gfx950 against the current
pathtrace.hpp, and on the corpus the GPU test runs, a numpy model of sphere_t's root search (rule A, rule B, then the division)
returns what the model of the reference's two divisions returns, in float64 and in float32 -- with every exit reached."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sphere_corpus as S  # noqa: E402
from test_gpu_sphere_roots import build_sphere_roots_check, corpus, first_bad, same_bits, sphere_oracle  # noqa: E402


def test_sphere_roots_check_cross_compiles_for_gfx950(tmp_path):
    exe = tmp_path / "sphere_roots_check"
    build_sphere_roots_check(exe)
    assert exe.stat().st_size > 0


def test_numpy_model_of_the_decided_roots_equals_the_two_divisions():
    rows, names = corpus()
    assert len(rows) >= 1 << 20
    for dt in (np.float64, np.float32):
        h_old, t_old, h_new, t_new, path, _ = S.model(rows, dt)
        ok = (h_old == h_new) & (~h_old | same_bits(t_old.astype(dt), t_new.astype(dt)))
        assert ok.all(), first_bad(ok, rows, names, f"model of sphere_t vs model of the two divisions ({dt.__name__})")
        S.check_coverage(names, path, h_new, f"model, {dt.__name__}")
        ties = S.ties_with_tmin(rows[names == "root_at_tmin"], dt)
        assert min(ties) >= 100, f"root_at_tmin: roots one ulp below tmin, at it, one ulp above it: {ties}"
        zeros, n_tangent = S.zero_discriminants(rows[names == "disc_zero"], dt), int((names == "disc_zero").sum())
        assert zeros >= n_tangent // 2, f"disc_zero: {zeros} of {n_tangent} cases have disc == 0"
        skipped = ((path == S.P_RULE_A) | (path == S.P_RULE_B)).sum()
        print(f"\n[sphere roots model] {dt.__name__}: {len(rows)} cases, {h_old.sum()} hits; second division skipped in {skipped} of "
              f"{(path >= S.P_RULE_A).sum()} cases whose first root was out of range")
        print(S.coverage_table(names, path))


def test_numpy_model_of_the_two_divisions_equals_the_oracle(o64, o32):
    rows, names = corpus()
    pick = np.arange(0, len(rows), 97)
    for o, dt in ((o64, np.float64), (o32, np.float32)):
        h, t = sphere_oracle(o, rows[pick])
        m_h, m_t = S.model(rows[pick], dt)[:2]
        ok = (m_h == h) & (~h | same_bits(m_t.astype(dt), t.astype(dt)))
        assert ok.all(), first_bad(ok, rows[pick], names[pick], f"numpy two-division model ({dt.__name__}) vs oracle_sphere_hit")
