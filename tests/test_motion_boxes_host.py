"""The input of CR_REFIT_REBUILD's builders, pinned without a device: tests/motion_boxes_check.cpp compiles the CR_HD rule of
crucible_amd/csrc/refit.hpp (prim_box_over) with g++ and prints the box of every primitive over a frame's ray times; the
oracle gives the same boxes through its own refit of a comb tree of one-primitive wrappers (tests/refit_rebuild_model.py).
f32 and f64, no tolerance.  The primitives cover LERP and NERP translate keys, a radius key, scale keys (translate and scale
parts sampled independently), a zero-length key and key starts and ends inside the frame's interval."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import refit_rebuild_model as RM
from crucible_amd import _abi as A
from crucible_amd.scene import LERP, LOCAL, NERP, Lambertian, Metal, Scene, Sphere, Triangle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]


def keyed_scene(frame):
    """1 fps, 360 degree shutter: frame f draws ray times in [f, f + 1]."""
    sc = Scene.new_image(16.0 / 9.0, 8, 1, 360.0, 1)
    sc.scene_cam.frame = frame
    m = Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)
    tri = lambda dx: Triangle.new((dx - 1.0, 0.1, 3.0), (dx + 0.3, -0.2, 3.2), (dx - 0.5, 1.2, 2.6), Metal.new((0.7, 0.7, 0.9), 0.1))
    sc.add_element(Sphere.new((0.3, 0.5, -1.0), 0.5, m), "still")
    sc.add_element(Sphere.new((-3.0, 0.5, 0.1), 0.5, m), "lerp")
    sc.translate_point((6.1, 0.3, -0.7), 1.0, LERP, LOCAL, "lerp")
    sc.add_element(Sphere.new((0.1, 0.5, -2.0), 0.4, m), "nerp")                # a key start inside [0, 1] and [1, 2]
    sc.translate_point((0.0, 1.5, 0.5), 0.5, NERP, LOCAL, "nerp")
    sc.translate_point((-2.3, 0.0, 0.7), 1.25, NERP, LOCAL, "nerp")
    sc.add_element(Sphere.new((2.5, 0.3, 1.5), 0.3, m), "radius")               # grows, then snaps small
    sc.scale_r(1.2, 0.75, LERP, "radius")
    sc.scale_r(0.5, 1.5, NERP, "radius")
    sc.add_element(Sphere.new((1.7, 0.9, 0.3), 0.25, m), "opposite")            # keys of opposite signs on one channel while the radius shrinks
    sc.translate_point((7.3, 0.0, 0.0), 0.6, LERP, LOCAL, "opposite")
    sc.translate_point((-7.1, 0.2, 0.0), 1.7, LERP, LOCAL, "opposite")
    sc.scale_r(0.05, 2.0, LERP, "opposite")
    sc.add_element(Sphere.new((-1.0, 0.4, 2.0), 0.4, m), "instant")             # a zero-length LERP key: 0/0 at its own instant
    sc.translate_point((0.0, 0.0, 0.0), 0.5, NERP, LOCAL, "instant")
    sc.translate_point((1.0, 2.0, -1.0), 0.5, LERP, LOCAL, "instant")
    sc.add_element(Sphere.new((-2.0, 0.4, 2.5), 0.4, m), "late")                # waits, then moves over [2, 3]
    sc.translate_point((0.0, 0.0, 0.0), 2.0, NERP, LOCAL, "late")
    sc.translate_point((4.0, 0.5, 0.0), 3.0, LERP, LOCAL, "late")
    sc.add_element(tri(0.0), "tri_lerp")
    sc.translate_point((1.5, 0.8, -1.0), 1.0, LERP, LOCAL, "tri_lerp")
    sc.add_element(tri(3.0), "tri_scale")                                       # scale keys with a translation: every pair of samples
    sc.scale_x(1.5, 1.0, LERP, "tri_scale")
    sc.scale_y(0.3, 0.5, NERP, "tri_scale")
    sc.translate_point((0.4, 0.0, -0.5), 1.5, LERP, LOCAL, "tri_scale")
    sc.scale_y(-0.2, 2.5, LERP, "tri_scale")
    sc.add_element(tri(-3.0), "tri_uniform")
    sc.scale_all_uniform(1.3, 1.0, LERP, "tri_uniform")
    sc.scale_z(0.8, 2.0, NERP, "tri_uniform")
    sc.add_element(tri(-6.0), "tri_point")
    sc.scale_point((0.5, 2.0, 1.5), 0.25, NERP, "tri_point")
    sc.translate_point((-0.5, 0.3, 0.0), 0.75, NERP, LOCAL, "tri_point")
    return sc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("motion_boxes") / "motion_boxes_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "crucible_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "motion_boxes_check.cpp")])
    return exe


def host_boxes(exe, flat, cam, rt, path):
    d = flat.desc
    with open(path, "wb") as f:
        f.write(struct.pack("<4i2d", 1 if rt == A.CR_REAL_F64 else 0, d.n_prims, d.n_keys, cam.frame, cam.frame_rate, cam.shutter_angle))
        f.write(bytes(flat.prims)[:d.n_prims * C.sizeof(A.CrPrimitive)])
        f.write(bytes(flat.keys)[:d.n_keys * C.sizeof(A.CrKeyframe)])
    out = subprocess.check_output([exe, path], text=True)
    return np.array([[float.fromhex(x) for x in line.split()] for line in out.splitlines()])


@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_host_rule_equals_the_oracle(check, oracles, tmp_path, rt, tag, frame):
    sc = keyed_scene(frame)
    flat = sc.flatten()
    want, vis = RM.oracle_motion_boxes(oracles[rt], flat, sc.scene_cam)
    assert len(vis) == flat.desc.n_prims == 11
    got = host_boxes(check, flat, sc.scene_cam, rt, str(tmp_path / "in.bin"))
    assert got.shape == (11, 6)
    bad = np.nonzero((got != want.astype(np.float64)).any(axis=1))[0]
    assert len(bad) == 0, f"frame {frame}: primitives {bad.tolist()} differ, first {got[bad[0]]!r} != {want[bad[0]]!r}"
    assert np.isfinite(got).all() and (got[:, 0::2] <= got[:, 1::2]).all()


def test_the_cases_are_not_vacuous(check, oracles, tmp_path):
    """Over [0, 1] every keyed primitive's box differs from its construction-time box, the static one's does not, and the
    frame matters."""
    import lbvh_model as L
    sc = keyed_scene(0)
    flat = sc.flatten()
    got = host_boxes(check, flat, sc.scene_cam, A.CR_REAL_F64, str(tmp_path / "in.bin"))
    recs = L.prim_records(flat)
    still = L.prim_boxes(recs["kind"], recs["v"], np.float64)
    moved = (got != still).any(axis=1)
    assert not moved[0] and moved[1:].all()
    assert np.abs(got[6] - still[6]).max() < 1e-12       # "late" has not started in frame 0: only timeline_pad moves its faces
    later = host_boxes(check, keyed_scene(2).flatten(), keyed_scene(2).scene_cam, A.CR_REAL_F64, str(tmp_path / "in2.bin"))
    assert np.abs(later[6] - still[6]).max() > 3.9 and (later != got).any(axis=1).sum() >= 6
