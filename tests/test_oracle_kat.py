"""The reference's own known-answer tests, replayed against the oracle.

Each test names the Rust test it restates (file:line in the reference's sources).  These are the
only results the reference pins for this path; they cover the arithmetic helpers, the
PPM byte mapping, average_samples and the keyframe evaluation.
"""
import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.timeline import LERP, LOCAL, NERP, TransformTimeline


@pytest.fixture(params=[A.CR_REAL_F64, A.CR_REAL_F32], ids=["f64", "f32"])
def o(request, oracles):
    return oracles[request.param]


def test_neg(o):   # src/utils.rs:704 neg_test
    assert list(o.vec_fn("oracle_neg", [1, 2, 3])) == [-1, -2, -3]


def test_plus_assign(o):   # src/utils.rs:718 plus_assign_test
    assert list(o.vec_fn("oracle_add", [1, 2, 3], [2, 2, 1])) == [3, 4, 4]


def test_dot(o):   # src/utils.rs:737 dot_test
    assert o.lib.oracle_dot(o._p(o.arr([1, 2, 3])), o._p(o.arr([2, 2, 1]))) == 9.0


def test_cross(o):   # src/utils.rs:748 cross_test
    assert list(o.vec_fn("oracle_cross", [3, -3, 1], [4, 9, 2])) == [-15, -2, 39]


def test_length(o):   # src/utils.rs:765 length_test
    assert o.lib.oracle_length(o._p(o.arr([3, 4, 0]))) == 5.0


def test_invalid_color(o):   # src/utils.rs:776 invalid_color_test (#[should_panic])
    assert o.lib.oracle_color_valid(20.0, 30.0, 40.0) == 0
    assert o.lib.oracle_color_valid(0.0, 0.5, 1.0) == 1
    assert o.lib.oracle_color_valid(float("nan"), 0.5, 1.0) == 0


def test_color_display(o):   # src/utils.rs:781 color_display_test -> "185 200 217"
    out = np.zeros(3, dtype=np.uint32)
    o.lib.oracle_color_display(0.529, 0.616, 0.730, out.ctypes.data)
    assert list(out) == [185, 200, 217]


def test_inv_color(o):   # src/utils.rs:788 inv_color: -(1,0,0) == (0,1,1)
    assert list(o.vec_fn("oracle_color_neg", [1, 0, 0])) == [0, 1, 1]


def test_add_color(o):   # src/utils.rs:796 add_color_test (clamped add)
    assert list(o.vec_fn("oracle_color_add", [1, 0, 0], [0, 1, 0])) == [1, 1, 0]
    assert list(o.vec_fn("oracle_color_add", [0.75, 0.5, 1.0], [0.5, 0.25, 1.0])) == [1, 0.75, 1]


def test_degrees_convert(o64):   # src/utils.rs:808 degrees_convert_test (f64 tolerance 5e-10)
    assert abs(o64.lib.oracle_degrees_to_radians(59.2958) - 1.034906943) < 0.0000000005


def test_degrees_to_radians_circular(o):   # src/utils.rs:821
    tol = 0.000000005 if o.real_type == A.CR_REAL_F64 else 1e-4
    assert abs(o.lib.oracle_radians_to_degrees(o.lib.oracle_degrees_to_radians(90.0)) - 90.0) < tol


def test_interval(o):   # src/utils.rs:834-912 size / contains / surrounds / universe / empty / discrete / greater / less / proportion
    L = o.lib
    assert L.oracle_interval_size(3.0, 20.0) == 17.0
    assert L.oracle_interval_contains(3.0, 20.0, 3.0) and not L.oracle_interval_contains(3.0, 20.0, 21.0)
    assert L.oracle_interval_contains(3.0, 20.0, 15.0)
    assert not L.oracle_interval_surrounds(3.0, 20.0, 3.0) and not L.oracle_interval_surrounds(3.0, 20.0, 21.0)
    assert L.oracle_interval_surrounds(3.0, 20.0, 15.0)
    rs = np.random.RandomState(0)
    for x in rs.uniform(-500, 500, size=10):
        assert L.oracle_interval_contains(-np.inf, np.inf, x)       # universe_contains_test
        assert not L.oracle_interval_contains(np.inf, -np.inf, x)   # empty_contains_test
    assert L.oracle_interval_contains(5.0, 5.0, 5.0)                # discrete_contains
    assert L.oracle_interval_is_greater(3.0, 10.0, 2.0)             # interval_greater
    assert L.oracle_interval_is_less(3.0, 10.0, 11.0)               # interval_less
    assert L.oracle_interval_proportion(2.0, 10.0, 4.0) == 0.25     # get_proportion


def test_ray_at(o):   # src/camera/mod.rs:383 ray_at_test
    out = np.zeros(3, dtype=o.np_real)
    o.lib.oracle_ray_at(o._p(o.arr([0, 0, 0])), o._p(o.arr([2.0, -3.0, 1.5])), 2.0, o._p(out))
    assert list(out) == [4.0, -6.0, 3.0]


def test_average_color(o):   # src/camera/mod.rs:390 average_color_test
    cols = o.arr([[0.0, 1.0, 0.0], [0.5, 0.5, 1.0]])
    out = np.zeros(3, dtype=o.np_real)
    o.lib.oracle_average_samples(o._p(cols), 2, o._p(out))
    assert list(out) == [0.25, 0.75, 0.5]


def _eval(o, tl, t):
    keys = tl.keyframes()
    arr = (A.CrKeyframe * max(1, len(keys)))(*keys)
    init = o.arr([*tl.start_pos, tl.start_scale])
    out = np.zeros(4, dtype=o.np_real)
    o.lib.oracle_timeline_eval(o._p(init), arr, len(keys), 1 if tl.sphere else 0, t, o._p(out))
    return out


def test_matrix_info_closures(o):   # src/timeline/mod.rs:271,281 matrix_info_constant / _interpolation
    tl = TransformTimeline.new_sphere((0, 0, 0), 1.0)
    tl.scale_sphere(3.0, 1.0, LERP)   # closure 1.0 + (3.0 - 1.0) * t over [0, 1]
    assert _eval(o, tl, 0.0)[3] == 1.0 and _eval(o, tl, 0.5)[3] == 2.0 and _eval(o, tl, 1.0)[3] == 3.0
    assert _eval(o, tl, 5.0)[3] == 3.0


def test_check_nerp_scaling(o):   # src/timeline/mod.rs:293
    tl = TransformTimeline.new_sphere((2.0, 3.0, 0.0), 1.0)
    tl.scale_sphere(15.0, 5.0, NERP)
    assert _eval(o, tl, 7.0)[3] == 15.0
    assert _eval(o, tl, 3.15)[3] == 1.0


def test_check_lerp_scaling(o):   # src/timeline/mod.rs:313
    tl = TransformTimeline.new_sphere((2.0, 3.0, 0.0), 1.0)
    tl.scale_sphere(15.0, 5.0, LERP)
    tl.scale_sphere(5.0, 10.0, LERP)
    assert _eval(o, tl, 5.0)[3] == 15.0
    assert abs(_eval(o, tl, 3.15)[3] - 10.0) < 0.2


def test_check_nerp_translate(o):   # src/timeline/mod.rs:333
    tl = TransformTimeline((2.0, 3.0, 1.0))
    tl.translate_x(1.0, 5.0, NERP, LOCAL)
    tl.translate_y(10.0, 3.0, NERP, LOCAL)
    r0 = _eval(o, tl, 0.0)
    assert r0[0] == 2.0 and r0[1] == 3.0
    r5 = _eval(o, tl, 5.0)
    assert r5[0] == 3.0 and r5[1] == 13.0


# ---- ScaleX / ScaleY / ScaleZ of non-sphere timelines.  The reference holds no test for them; these are hand
# evaluations of S * T * (0,0,0,1) with the matrices transform_builder.rs:101-346 builds (ScaleY's factor sits in
# row 1, column 0, :228-246) and the "last active scale wins" rule of timeline/mod.rs:249-255.
def test_scale_axis_matrices(o):
    p = (1.0, 2.0, 3.0)
    tl = TransformTimeline(p); tl.scale_x(3.0, 1.0, NERP)
    assert list(_eval(o, tl, 0.5)[:3]) == [1.0, 2.0, 3.0] and list(_eval(o, tl, 1.0)[:3]) == [3.0, 2.0, 3.0]
    tl = TransformTimeline(p); tl.scale_z(3.0, 1.0, NERP)
    assert list(_eval(o, tl, 2.0)[:3]) == [1.0, 2.0, 9.0]
    tl = TransformTimeline(p); tl.scale_y(3.0, 1.0, NERP)       # y' = 3 * x + y: the (1,0) slot, not the diagonal
    assert list(_eval(o, tl, 2.0)[:3]) == [1.0, 5.0, 3.0]
    assert _eval(o, tl, 2.0)[3] == 1.0 and _eval(o, tl, 0.0)[3] == 1.0


def test_scale_axis_lerp_and_last_active_wins(o):
    tl = TransformTimeline((1.0, 2.0, 3.0))
    tl.scale_x(3.0, 2.0, LERP)                                  # 1 + (3 - 1) * t/2 over [0, 2]
    assert list(_eval(o, tl, 1.0)[:3]) == [2.0, 2.0, 3.0] and list(_eval(o, tl, 7.0)[:3]) == [3.0, 2.0, 3.0]
    tl.scale_z(0.5, 1.5, NERP)                                  # starts at 1.5: from then on it is the last active scale
    assert list(_eval(o, tl, 1.0)[:3]) == [2.0, 2.0, 3.0]
    assert list(_eval(o, tl, 1.5)[:3]) == [1.0, 2.0, 1.5] and list(_eval(o, tl, 9.0)[:3]) == [1.0, 2.0, 1.5]
    tl = TransformTimeline((1.0, 2.0, 3.0))
    tl.scale_point((2.0, 3.0, 4.0), 1.0, NERP)                  # X, Y, Z pushed with one interval: Z is last
    assert list(_eval(o, tl, 1.0)[:3]) == [1.0, 2.0, 12.0]
    tl.translate_x(4.0, 0.5, NERP, LOCAL)                       # translate first, then scale: S * T
    tl.scale_y(0.5, 3.0, LERP)                                  # previous ScaleY ended at 3.0, t = 1: 3 + (0.5 - 3) * s
    assert list(_eval(o, tl, 2.0)[:3]) == [5.0, (3.0 + (0.5 - 3.0) * 0.5) * 5.0 + 2.0, 3.0]


def test_scale_keys_flatten_in_list_order():
    """The scale list after scaled_teapot's calls, worked by hand from most_recent_matching_transform
    (helper_functions.rs:41-140) and the stable sort by start time (transform_builder.rs `sort_by compare_start`)."""
    from crucible_amd.demo_builder import scaled_teapot
    sc = scaled_teapot(1)
    f = sc.flatten()
    n = f.prims[0].key_count
    got = [(k.channel, k.interp, k.t0, k.t1, k.a, k.b) for k in f.keys[:n]]
    assert got == [(0, 1, 0.0, 0.02, 0.0, 0.0), (1, 1, 0.0, 0.02, 0.4, 0.0), (2, 1, 0.0, 0.02, 0.3, 0.0),
                   (4, 1, 0.0, 0.012, 1.0, 1.4), (6, 1, 0.0, 0.05, 1.0, 1.2), (4, 1, 0.012, 0.05, 1.4, 1.2),
                   (5, 0, 0.016, 0.016, 0.25, 0.0), (5, 1, 0.016, 0.05, 0.25, 1.2), (6, 1, 0.05, 0.09, 1.2, 0.7)]
    with pytest.raises(ValueError):
        sc.scale_x(2.0, 1.0, LERP, "ground")                    # "ScaleX cannot apply to Spheres" (scene_animator.rs:39-41)
