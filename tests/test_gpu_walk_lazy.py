"""The f64 SCREEN walk as the kernels of lazy_inv() run it (crucible_amd/csrc/pathtrace.hpp): tests/walk_lazy_check.hip begins every
segment with walk_begin_screened<true> and runs the megakernel's loop around walk_round<double, RES, false, ORD, true, true,
/*LAZY_INV*/ true>, one wave per 64 lanes, ray by ray against the counted oracle probe (oracle_world_hit_counted): hit primitive,
the bits of t, node tests and primitive tests, as test_gpu_walk_round.py does.

Trees: a 64-sphere book-style scene staged whole in LDS (RES_LDS; also with the spheres-only primitive loop, SPHERE_LOOP), the
same tree forced to RES_TOP with a 16-record window, and its CR_BVH_SAH_ORDERED twin in both residencies.
Rays: the general corpus of tests/walk_round_corpus.py (camera rays, misses, rays from inside, the searched band rays), and
  one_zero, two_zeros    exact zero direction components: 1 / d infinite -- the compare/select form, 1.0 / rd divided where it runs
  denormal               a subnormal component
  pow105                 a component of 2^+-105 times the others: 1 / d finite but outside screen_in_range
  far_steep              origins 10^6 .. 10^8 away aimed at the spheres through a small component: |of if| is huge, so TH is, and
                         the box tests land in the band -- Aabb::hit in f64 with inv_of(rd)
Schedules: budgets 0, 1, 3 and 10 steps per round, leaf-phase thresholds 0 and 8, exit thresholds 1, 33 and 64 lanes: at exit 1
a wave leaves the walk as soon as one lane is done and the others resume in the next outer iteration with the WalkState they
kept (invf, unscreened, a parked leaf).  Every schedule and lane permutation must give the same bytes.
So that a passing run proves something: per tree and residency at least 100 band lanes and at least 1000 rays on the
compare/select path (the device's count, which must equal the count the corpus implies), and resumed lanes at every budget."""
import os
import subprocess

import numpy as np
import pytest

import walk_round_corpus as W
from crucible_amd import _abi as A
from crucible_amd.scene import Scene, Sphere
from test_gpu_shade_primitives import HIPCC
from test_walk_round_corpus import MODES, build_tree_check, host_tree, probe_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "walk_lazy_check.hip")
RAY_OUT = np.dtype([("best", "<i4"), ("mat", "<i4"), ("t", "<u8"), ("nodes", "<u4"), ("prims", "<u4")])
WAVE_OUT = np.dtype([("rounds", "<u4"), ("leaf_phases", "<u4"), ("band_lanes", "<u4"), ("survived", "<u4"), ("unscreened", "<u4"), ("resumed", "<u4")])
WINDOW = 16
SCHED = np.array([(b, m, e) for b in (0, 1, 3, 10) for m in (0, 8) for e in (1, 33, 64)], dtype=np.int32)
KERNELS = {"ref": ("lds", "top", "lds_sl"), "ord": ("lds", "top")}
COMPARE_SELECT = ("one_zero", "two_zeros", "denormal", "pow105")


def scene64():
    """A ground and 63 small spheres, each with a material of its own (the probe names the primitive by it)."""
    sc = Scene.new_image(1.5, 12, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(1)
    cam.set_max_depth(1)
    cam.look_from(tuple(W.EYE))
    cam.look_at((0.0, 0.4, 0.0))
    cam.set_vfov(42.0)
    rs = np.random.RandomState(64)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, W.own_material()), "ground")
    for k in range(63):
        r = 0.15 + 0.25 * rs.rand()
        sc.add_element(Sphere.new((-6.0 + 12.0 * rs.rand(), r, -6.0 + 10.0 * rs.rand()), r, W.own_material()), f"s{k}")
    return sc


def edge_rays(flat):
    """The groups of this test: (rows n x 7, names)."""
    rs = np.random.RandomState(17)
    cs = W.centres(flat)
    rows, names = [], []

    def add(name, o, d):
        rows.append(np.concatenate([o, d, [0.0]]))
        names.append(name)

    for k in range(300):
        c = cs[rs.randint(len(cs))] + rs.uniform(-0.2, 0.2, 3) * (rs.uniform() < 0.5)
        ax = rs.randint(3)
        d = rs.normal(size=3) * rs.uniform(0.5, 4.0)
        d[ax] = 0.0 * rs.choice([-1.0, 1.0])            # +0 and -0
        add("one_zero", c - d * rs.uniform(0.5, 3.0), d)
        d2 = np.zeros(3)
        d2[ax] = rs.choice([-1.0, 1.0]) * rs.uniform(0.5, 4.0)
        d2[(ax + 1) % 3] = 0.0 * rs.choice([-1.0, 1.0])
        add("two_zeros", c - d2 * rs.uniform(0.5, 3.0), d2)
    for k in range(200):
        c = cs[rs.randint(len(cs))]
        d = rs.normal(size=3) * rs.uniform(0.5, 4.0)
        o = c - d * rs.uniform(0.5, 3.0)
        d[rs.randint(3)] = rs.choice([-1.0, 1.0]) * 4.9e-324 * rs.randint(1, 1 << 40)
        add("denormal", o, d)
    for k in range(400):
        c = cs[rs.randint(len(cs))]
        d = rs.normal(size=3) * rs.uniform(0.5, 4.0)
        o = c - d * rs.uniform(0.5, 3.0)
        d[rs.randint(3)] = rs.choice([-1.0, 1.0]) * rs.uniform(0.5, 4.0) * 2.0 ** (105 * rs.choice([-1, 1]))
        add("pow105", o, d)
    for k in range(300):
        c = cs[rs.randint(len(cs))] + rs.uniform(-0.1, 0.1, 3)
        u = rs.normal(size=3)
        u[rs.randint(3)] *= 10.0 ** rs.uniform(-4, -2)      # steep: one component small, finite and in the screen's range
        u /= np.linalg.norm(u)
        dist = 10.0 ** rs.uniform(6, 8)
        add("far_steep", c + u * dist, -u * dist * rs.uniform(0.5, 2.0))
    return np.array(rows), np.array(names)


def unscreened_ref(rows):
    """walk_begin_screened's classification restated: some |(float)(1 / d)| outside [2^-100, 2^100] (or not a number), or an
    origin component beyond 2^100.  (No ray of the corpus sits within rounding of those bounds.)"""
    with np.errstate(all="ignore"):
        i = np.abs((1.0 / rows[:, 3:6]).astype(np.float32))
        o = np.abs(rows[:, 0:3].astype(np.float32))
        ok = (i >= np.float32(2.0 ** -100)) & (i <= np.float32(2.0 ** 100))
    return ~(ok.all(axis=1) & (o.max(axis=1) <= np.float32(2.0 ** 100)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, o64):
    dd = tmp_path_factory.mktemp("walk_lazy")
    exe, tree_exe = dd / "walk_lazy_check", dd / "tree_check"
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)
    build_tree_check(tree_exe)
    sc = scene64()
    flat = sc.flatten()
    assert flat.desc.n_prims == 64
    trees, scene_bytes = {}, {}
    for mode in KERNELS:
        trees[mode], scene_bytes[mode] = host_tree(tree_exe, dd, flat, A.CR_REAL_F64, MODES[mode])
        assert len(trees[mode][0]) > WINDOW   # the window is a part of the tree
    general, gnames = W.rays("lazy", o64, sc, trees)
    edge, enames = edge_rays(flat)
    rows, names = np.concatenate([general, edge]), np.concatenate([gnames, enames])
    # what the run must contain, from the corpus alone, before the device is asked
    unscreened = unscreened_ref(rows)
    assert unscreened[np.isin(names, COMPARE_SELECT)].all() and not unscreened[names == "far_steep"].any()
    assert unscreened.sum() >= 1000 and (names == "far_steep").sum() >= 100
    table = W.assignments(len(rows))
    paths = {}
    for mode in KERNELS:
        paths[mode] = dd / mode
        W.write_case(paths[mode], scene_bytes[mode], rows, table)
        SCHED.tofile(paths[mode] / "sched.in")
    r = subprocess.run([str(exe), str(WINDOW)] + [str(p) for p in paths.values()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    n, (P, B) = len(rows), table.shape[:2]
    for mode, kernels in KERNELS.items():
        raw = (paths[mode] / "tree.out").read_bytes()
        ne = int(np.frombuffer(raw, "<i4", 1)[0])
        boxes = np.frombuffer(raw, "<f8", ne * 6, 4).reshape(ne, 6)
        tail = np.frombuffer(raw, "<i4", ne * 3, 4 + ne * 48)
        exported = (boxes, tail[:2 * ne].reshape(ne, 2), tail[2 * ne:])
        for a, b in zip(exported, trees[mode]):
            assert np.array_equal(a, b), mode
        want = probe_all(o64, flat, rows, None if mode == "ref" else exported)
        for kernel in kernels:
            raw = np.fromfile(paths[mode] / f"{kernel}.out", dtype=np.uint8)
            cut = len(SCHED) * P * n * RAY_OUT.itemsize
            out[(mode, kernel)] = {"rays": raw[:cut].view(RAY_OUT).reshape(len(SCHED), P, n), "want": want,
                                   "waves": raw[cut:].view(WAVE_OUT).reshape(len(SCHED), P, B)}
    return out, names, unscreened


def test_every_ray_equals_the_counted_oracle_probe(runs):
    out, names, _ = runs
    assert set(out) == {("ref", "lds"), ("ref", "top"), ("ref", "lds_sl"), ("ord", "lds"), ("ord", "top")}
    for key, r in out.items():
        got, want = r["rays"][0, 0], r["want"]
        hit = got["best"] >= 0
        ok = (hit == want["hit"]) & (got["nodes"] == want["nodes"]) & (got["prims"] == want["prims"])
        dev = got["t"].view(np.float64)
        same_t = (got["t"] == want["bits"]) | (np.isnan(dev) & np.isnan(want["t"]))
        ok &= ~hit | ((got["mat"] == want["mat"]) & same_t)
        bad = np.flatnonzero(~ok)
        assert len(bad) == 0, (f"{key}: {len(bad)} rays differ from the oracle; first: group {names[bad[0]]}, ray {bad[0]}: device {got[bad[0]]}, "
                               f"oracle hit {want['hit'][bad[0]]} mat {want['mat'][bad[0]]} t bits {want['bits'][bad[0]]} nodes {want['nodes'][bad[0]]} "
                               f"prims {want['prims'][bad[0]]}")
        for g in np.unique(names):   # every group walks: it tests boxes, and the groups aimed at spheres hit some
            assert want["nodes"][names == g].sum() > 0, g
        for g in ("one_zero", "two_zeros", "denormal", "far_steep", "camera"):
            assert hit[names == g].any(), (key, g)


def test_output_is_byte_identical_across_schedules_and_permutations(runs):
    out, names, _ = runs
    for key, r in out.items():
        first = r["rays"][0, 0]
        for s in range(len(SCHED)):
            for p in range(r["rays"].shape[1]):
                if r["rays"][s, p].tobytes() != first.tobytes():
                    bad = np.flatnonzero(r["rays"][s, p] != first)
                    raise AssertionError(f"{key}: schedule (budget, leaf_min, exit) = {tuple(SCHED[s])}, permutation {p}: {len(bad)} rays differ; "
                                         f"first: group {names[bad[0]]}: {r['rays'][s, p][bad[0]]} != {first[bad[0]]}")


def test_the_run_reached_the_band_the_compare_select_path_and_resumption(runs):
    out, names, unscreened = runs
    for key, r in out.items():
        waves = r["waves"]
        for s in range(len(SCHED)):
            for p in range(waves.shape[1]):
                # the device's classification is the corpus's, ray for ray in total
                assert int(waves[s, p]["unscreened"].sum()) == int(unscreened.sum()), (key, tuple(SCHED[s]), p)
                assert int(waves[s, p]["band_lanes"].sum()) >= 100, (key, tuple(SCHED[s]), p, int(waves[s, p]["band_lanes"].sum()))
        assert int(unscreened.sum()) >= 1000
        for b in (1, 3, 10):   # stragglers: at exit threshold 1 lanes leave the loop unfinished and resume, at every budget
            s = int(np.flatnonzero((SCHED[:, 0] == b) & (SCHED[:, 1] == 0) & (SCHED[:, 2] == 1))[0])
            assert (waves[s]["resumed"].sum(axis=-1) >= 64).all(), (key, b, waves[s]["resumed"].sum(axis=-1))
        s8 = SCHED[:, 1] == 8
        assert (waves[s8 & (SCHED[:, 2] == 1)]["survived"] > 0).any(), key   # a parked leaf carried across outer iterations
        print(f"\n[walk lazy] {key}: {len(names)} rays, {int(unscreened.sum())} on the compare/select path, band lanes "
              f"{int(waves[0, 0]['band_lanes'].sum())}, resumed lanes at budgets 1/3/10, exit 1: "
              + "/".join(str(int(waves[int(np.flatnonzero((SCHED[:, 0] == b) & (SCHED[:, 1] == 0) & (SCHED[:, 2] == 1))[0]), 0]['resumed'].sum())) for b in (1, 3, 10)))
