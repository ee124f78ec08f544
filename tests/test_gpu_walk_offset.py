"""The headline's two kernels -- pathtrace_kernel_quiet<RES_LDS> and its counted twin -- carry the walk's position across
rounds and outer iterations as the LDS address of the next screening record (walk.hpp WalkOffset) and run
their rounds at a raised wave priority.  Neither changes a path: through the ABI, f64 with relaxed sums, every case renders
without and with a CrStats and holds
  - the quiet frame np.array_equal to the counted one,
  - the counted frame to the oracle's within the relaxed-sum bound of tests/test_gpu_relaxed.py (1e-12),
  - the four work counters equal to the oracle's,
under CRUCIBLE_WALK_ROUND 1 / 10 x CRUCIBLE_WALK_EXIT 1 / 64 x CRUCIBLE_WALK_LEAF_MIN 0 / 8: budgets at which a lane leaves a
round after every step, exits at which a wave leaves the walk with 63 lanes unfinished (their address, and a parked leaf
with it, kept across the outer iteration), and leaf phases that wait.
Scenes: book1 64 x 36 @ 4 spp; spheres alone with two-primitive leaves; trees of 1 .. 5 and 7 spheres (the address reaches
`end` on the first step, a two-primitive leaf is the last record: after_leaf == end); a scene scaled beyond the screen's
range (every step through the compare/select loop, which reads an index); a sphere edited in place with
cr_update_primitives, radius changed.
Ray by ray (the second half of the file): tests/walk_offset_check.hip walks a few hundred rays per tree on the offset state
under 13 schedules against the counted oracle probe -- trees of 1, 2, 3, 5 and 64 spheres, and one of 1229 spheres whose
staged copy is 163840 bytes, a CU's LDS to the last byte: the top of the range an address, a link and `end` can take."""
import numpy as np
import pytest

import scenes
import update_model as um
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.renderer import Renderer
from crucible_amd.scene import Dielectric, Lambertian, Metal, Scene, Sphere
from test_gpu_quiet import far_axis_scene

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
COUNTERS = ("segments", "node_tests", "prim_tests", "texel_fetches")
F64, RELAX = A.CR_REAL_F64, A.CR_SUM_RELAXED
BOUND = 1e-12   # tests/test_gpu_relaxed.py: a relaxed frame against the oracle's
KNOBS = [(r, e, m) for r in ("1", "10") for e in ("1", "64") for m in ("0", "8")]


def book1():
    sc = book1_end_scene(1, scene_seed=1, image_width=64, samples=4)
    assert (sc.scene_cam.image_width, sc.scene_cam.image_height) == (64, 36)
    return sc


def spheres_alone():
    """A ground and 22 spheres of three materials: the reference tree ends its branches in leaves of one and of two."""
    sc = Scene.new_image(16.0 / 9.0, 64, 4, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(4)
    cam.set_max_depth(12)
    cam.look_from((0.0, 2.0, 9.0))
    cam.look_at((0.0, 0.5, 0.0))
    cam.set_vfov(40.0)
    rs = np.random.RandomState(23)
    mats = [Lambertian.new_from_color((0.7, 0.3, 0.2), 1.0), Metal.new((0.8, 0.8, 0.9), 0.05), Dielectric.new(1.5)]
    sc.add_element(Sphere.new((0.0, -200.0, 0.0), 200.0, Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)), "ground")
    for k in range(22):
        r = 0.2 + 0.4 * rs.rand()
        sc.add_element(Sphere.new((-5.0 + 10.0 * rs.rand(), r, -4.0 + 7.0 * rs.rand()), r, mats[k % 3]), f"s{k}")
    return sc


SCENES = {"book1": book1, "spheres": spheres_alone}


@pytest.fixture(scope="module")
def references(o64):
    """The oracle's frame and counters of each scene, rendered once."""
    return {name: o64.render_image(build(), seed=SEED, sum_order=RELAX) for name, build in SCENES.items()}


def pair(r, cam, ref, rst, **kw):
    quiet, _ = r.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=False, **kw)
    counted, st = r.render(cam, seed=SEED, real_type=F64, sum_order=RELAX, want_stats=True, **kw)
    assert st["scene_in_lds"] == 1   # RES_LDS: the kernels this file is about
    assert np.array_equal(quiet, counted, equal_nan=True), f"differing px = {(quiet != counted).any(axis=-1).sum()}"
    err = np.nanmax(np.abs(counted - ref))
    print(f"\n[walk offset] max |frame - oracle| = {err:.3e}")
    assert err <= BOUND and np.array_equal(np.isnan(counted), np.isnan(ref)), err
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    return counted, st


@pytest.mark.parametrize("steps,exit_lanes,leaf_min", KNOBS, ids=["r%s-e%s-m%s" % k for k in KNOBS])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_schedules_against_the_oracle(references, monkeypatch, name, steps, exit_lanes, leaf_min):
    monkeypatch.setenv("CRUCIBLE_WALK_ROUND", steps)
    monkeypatch.setenv("CRUCIBLE_WALK_EXIT", exit_lanes)
    monkeypatch.setenv("CRUCIBLE_WALK_LEAF_MIN", leaf_min)
    sc = SCENES[name]()
    ref, rst = references[name]
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        if name == "spheres":
            _, kids, _ = r.export_bvh(F64)
            leaves = (kids[:, 0] < 0) & (kids[:, 1] < 0)
            assert (kids[leaves, 0] != kids[leaves, 1]).any() and (kids[leaves, 0] == kids[leaves, 1]).any()
        pair(r, sc.scene_cam, ref, rst)
    finally:
        r.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
def test_smallest_trees(renderer, o64, n):
    """One wrapper: `end` is the first link followed.  Two spheres: one leaf of two, the tree's last record."""
    sc = scenes.few_spheres(n, width=32, samples=2)
    renderer.upload_scene(sc.flatten())
    _, kids, _ = renderer.export_bvh(F64)
    assert len(kids) >= 1
    ref, rst = o64.render_image(sc, seed=SEED, sum_order=RELAX)
    pair(renderer, sc.scene_cam, ref, rst)


def test_every_step_in_the_compare_select_loop(renderer, o64):
    """Rays outside screen_in_range: the loop that reads an index makes every step, and hands an address back."""
    sc = far_axis_scene()
    renderer.upload_scene(sc.flatten())
    ref, rst = o64.render_image(sc, seed=SEED, sum_order=RELAX, output_sum=True)
    _, st = pair(renderer, sc.scene_cam, ref, rst, output_sum=True)
    assert st["prim_tests"] > 0


def test_sphere_edited_in_place(renderer, oracles):
    """cr_update_primitives: two spheres moved, one with another radius; 32 x 18 @ 2 spp against the oracle on the tree the
    handle exports."""
    sc = scenes.few_spheres(5, width=32, samples=2)
    flat = sc.flatten()
    cam = sc.scene_cam
    assert (cam.image_width, cam.image_height) == (32, 18)
    renderer.upload_scene(flat)
    before, _ = renderer.render(cam, seed=SEED, real_type=F64, sum_order=RELAX)
    _, _, v = um.prim_arrays(flat)
    idx = np.array([1, 3], dtype=np.int32)
    rows = v[idx].copy()
    rows[0, 3] *= 1.75            # radius
    rows[0, 1] += 0.4
    rows[1, 0] -= 0.6
    renderer.update_primitives(idx, rows)
    um.apply_edit(flat, idx, rows)
    tree = renderer.export_bvh(F64)
    ref, rst = um.oracle_render_flat(oracles[F64], flat, cam, seed=SEED, tree=tree, sum_order=RELAX)
    img, _ = pair(renderer, cam, ref, rst)
    assert not np.array_equal(img, before)


# ---- ray by ray: tests/walk_offset_check.hip runs walk_begin_screened and walk_round on the offset state, one wave per 64 lanes,
# against the counted oracle probe (hit primitive, the bits of t, node tests, primitive tests), as tests/test_gpu_walk_lazy.py does
import os  # noqa: E402
import subprocess  # noqa: E402

import lds_capacity as L  # noqa: E402
import walk_round_corpus as W  # noqa: E402
from test_gpu_shade_primitives import HIPCC  # noqa: E402
from test_gpu_walk_lazy import RAY_OUT, WAVE_OUT, edge_rays, scene64, unscreened_ref  # noqa: E402
from test_walk_round_corpus import MODES, build_tree_check, host_tree, probe_all  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "walk_offset_check.hip")
SCHED = np.array([(0, 0, 64)] + [(b, m, e) for b in (1, 3, 10) for m in (0, 8) for e in (1, 64)], dtype=np.int32)


def tiny(n):
    """n spheres side by side, a material each: trees of one wrapper (n = 1, 2: the second a leaf of two), three and more."""
    sc = Scene.new_image(1.5, 12, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(1)
    cam.set_max_depth(1)
    cam.look_from(tuple(W.EYE))
    cam.look_at((0.0, 0.4, 0.0))
    for k in range(n):
        sc.add_element(Sphere.new((1.5 * k - 0.75 * (n - 1), 0.5, -0.3 * k), 0.5, W.own_material()), f"t{k}")
    return sc


def aimed_rays(flat, n, seed):
    """Rays at the spheres' centres with some scatter, a third of them from inside the scene, and plain misses."""
    rs = np.random.RandomState(seed)
    cs = W.centres(flat)
    rows = []
    for k in range(n):
        c = cs[rs.randint(len(cs))] + rs.uniform(-0.6, 0.6, 3)
        o = W.EYE + rs.uniform(-2.0, 2.0, 3) if k % 3 else cs[rs.randint(len(cs))] + rs.uniform(-0.3, 0.3, 3)
        d = (c - o) * rs.uniform(0.3, 3.0) if k % 7 else rs.normal(size=3)
        rows.append(np.concatenate([o, d, [0.0]]))
    return np.array(rows)


LDS_FULL_SPHERES = 1229   # 1433 screening records of 32 bytes and 1229 primitive records of 96: 163840 bytes, a CU's LDS to the byte


def lds_full():
    """The largest scene of spheres whose staged copy (screening records | primitives) still fits the 160 KB a launch may ask
    for, and fills them to the last byte: tests/lds_capacity.py's ground, grid and marker (the marker is the primitive at the
    last leaf position, the record that ends at byte 163840).  Record addresses, the links, `end` and the leaf flag beside
    them sit at the top of the range the offset state can hold."""
    assert L.r16(L.tree_size(LDS_FULL_SPHERES) * 32) + LDS_FULL_SPHERES * 96 == L.LDS
    assert L.r16(L.tree_size(LDS_FULL_SPHERES + 1) * 32) + (LDS_FULL_SPHERES + 1) * 96 > L.LDS
    sc = Scene.new_image(1.5, 12, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(1)
    cam.set_max_depth(1)
    cam.look_from(tuple(W.EYE))
    cam.look_at((0.0, 0.4, 0.0))
    for k, v in enumerate(L.capacity_spheres(LDS_FULL_SPHERES)):
        sc.add_element(Sphere.new(tuple(v[:3]), float(v[3]), W.own_material()), f"c{k}")
    return sc


CASES = {"one": lambda: tiny(1), "two": lambda: tiny(2), "three": lambda: tiny(3), "five": lambda: tiny(5), "sixty_four": scene64,
         "lds_full": lds_full}


@pytest.fixture(scope="module")
def walked(tmp_path_factory, o64):
    dd = tmp_path_factory.mktemp("walk_offset")
    exe, tree_exe = dd / "walk_offset_check", dd / "tree_check"
    subprocess.run(HIPCC + ["-o", str(exe), CHECK_SRC], check=True, timeout=600)
    build_tree_check(tree_exe)
    cases = {}
    for name, build in CASES.items():
        flat = build().flatten()
        tree, scene_bytes = host_tree(tree_exe, dd, flat, F64, MODES["ref"])
        rows = aimed_rays(flat, 96, len(name))
        if name == "lds_full":     # and rays at the marker, the last primitive record, from both sides of the grid
            _, _, v = um.prim_arrays(flat)
            rs = np.random.RandomState(5)
            at = [np.concatenate([o, (v[-1, :3] + rs.uniform(-0.4, 0.4, 3) - o) * rs.uniform(0.5, 2.0), [0.0]])
                  for o in (W.EYE + rs.uniform(-3.0, 3.0, (64, 3)))]
            rows = np.concatenate([rows, np.array(at)])
        if name == "sixty_four":   # every fourth ray of the compare/select and band groups of tests/test_gpu_walk_lazy.py
            edge, _ = edge_rays(flat)
            rows = np.concatenate([rows, edge[::4]])
        table = W.assignments(len(rows))
        path = dd / name
        W.write_case(path, scene_bytes, rows, table)
        SCHED.tofile(path / "sched.in")
        cases[name] = (flat, tree, rows, table, path)
    r = subprocess.run([str(exe)] + [str(c[4]) for c in cases.values()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for name, (flat, tree, rows, table, path) in cases.items():
        n, (P, B) = len(rows), table.shape[:2]
        want = probe_all(o64, flat, rows, None)
        for kernel in ("lds", "lds_sl"):
            raw = np.fromfile(path / f"{kernel}.out", dtype=np.uint8)
            cut = len(SCHED) * P * n * RAY_OUT.itemsize
            out[(name, kernel)] = {"rays": raw[:cut].view(RAY_OUT).reshape(len(SCHED), P, n), "want": want, "wrappers": len(tree[0]),
                                   "staged": int((path / "lds.bytes").read_text()),
                                   "waves": raw[cut:].view(WAVE_OUT).reshape(len(SCHED), P, B), "unscreened": unscreened_ref(rows)}
    return out


def test_the_smallest_trees_are_among_the_cases(walked):
    """One sphere: one wrapper, `end` is the first link followed.  Two spheres: the reference tree is ONE wrapper whose leaf
    holds both (no tree of this builder has two wrappers) -- a two-primitive leaf as the last record, after_leaf == end.
    Three spheres: three wrappers."""
    sizes = {name: r["wrappers"] for (name, kernel), r in walked.items() if kernel == "lds"}
    print("\n[walk offset] wrappers per case:", sizes)
    assert sizes["one"] == 1 and sizes["two"] == 1 and sizes["three"] == 3, sizes
    assert sum(r["rays"].shape[2] for (name, kernel), r in walked.items() if kernel == "lds") >= 300


def test_the_full_lds_case_ends_at_the_last_byte(walked):
    """160 KB staged, to the byte; the marker at the last leaf position is hit, so the last primitive record was read."""
    r = walked[("lds_full", "lds")]
    assert r["staged"] == L.LDS == 163840 and r["wrappers"] == L.tree_size(LDS_FULL_SPHERES) == 1433
    got = r["rays"][0, 0]
    assert (got["best"] == LDS_FULL_SPHERES - 1).sum() >= 16, (got["best"] == LDS_FULL_SPHERES - 1).sum()
    assert (got["best"] == 0).any()   # and the ground, the first


def test_every_ray_equals_the_counted_oracle_probe_under_every_schedule(walked):
    for key, r in walked.items():
        want = r["want"]
        for s in range(len(SCHED)):
            for p in range(r["rays"].shape[1]):
                got = r["rays"][s, p]
                hit = got["best"] >= 0
                ok = (hit == want["hit"]) & (got["nodes"] == want["nodes"]) & (got["prims"] == want["prims"])
                dev = got["t"].view(np.float64)
                same_t = (got["t"] == want["bits"]) | (np.isnan(dev) & np.isnan(want["t"]))
                ok &= ~hit | ((got["mat"] == want["mat"]) & same_t)
                bad = np.flatnonzero(~ok)
                assert len(bad) == 0, (key, tuple(SCHED[s]), p, len(bad), bad[0], got[bad[0]], want["hit"][bad[0]], want["nodes"][bad[0]], want["prims"][bad[0]])
        assert want["nodes"].sum() > 0 and (r["rays"][0, 0]["best"] >= 0).any(), key


def test_the_run_reached_the_band_the_compare_select_loop_and_resumption(walked):
    for kernel in ("lds", "lds_sl"):
        r = walked[("sixty_four", kernel)]
        waves = r["waves"]
        assert int(r["unscreened"].sum()) >= 200   # rays whose every step reads an index
        for s in range(len(SCHED)):
            assert int(waves[s, 0]["unscreened"].sum()) == int(r["unscreened"].sum()), tuple(SCHED[s])
            assert int(waves[s, 0]["band_lanes"].sum()) >= 25, (tuple(SCHED[s]), int(waves[s, 0]["band_lanes"].sum()))
        for b in (1, 3, 10):   # lanes that leave the walk unfinished at exit 1 and resume from the address they kept
            s = int(np.flatnonzero((SCHED[:, 0] == b) & (SCHED[:, 1] == 0) & (SCHED[:, 2] == 1))[0])
            assert (waves[s]["resumed"].sum(axis=-1) >= 64).all(), (kernel, b)
        s8 = (SCHED[:, 1] == 8) & (SCHED[:, 2] == 1)
        assert (waves[s8]["survived"] > 0).any(), kernel   # a parked leaf carried across outer iterations
