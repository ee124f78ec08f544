"""CPU side of tests/test_gpu_walk_primitives.py: the device check program still compiles for gfx950 against the current
pathtrace.hpp, and the numpy Aabb::hit that judges the large box sets on the GPU agrees with the oracle's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_corpus as W  # noqa: E402
from test_gpu_walk_primitives import aabb_oracle, build_walk_check, first_bad  # noqa: E402


def test_walk_check_cross_compiles_for_gfx950(tmp_path):
    exe = tmp_path / "walk_check"
    build_walk_check(exe)
    assert exe.stat().st_size > 0


def test_numpy_aabb_reference_matches_the_oracle(o64, o32):
    groups = W.box_corpus(1, scale=0.05)
    box = np.concatenate(list(groups.values()))
    names = np.concatenate([[k] * len(v) for k, v in groups.items()])
    for o, dt in ((o64, np.float64), (o32, np.float32)):
        ref = W.aabb_hit_ref(box, dt)
        orc = aabb_oracle(o, box)
        assert np.array_equal(ref, orc), first_bad(ref == orc, box, names, f"numpy Aabb::hit ({dt.__name__}) vs oracle_aabb_hit")
        # both outcomes occur in every group that is meant to sit near the boundary
        for g in ("grazing", "grazing_far_origin", "ties", "signed_zeros"):
            sel = names == g
            assert 0 < ref[sel].sum() < sel.sum(), (g, dt)
