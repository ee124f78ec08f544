"""walk_round (crucible_amd/csrc/pathtrace.hpp) on the device on its own, one wave at a time, under every schedule:
tests/walk_round_check.hip runs the megakernel's walk loop without shading -- lanes with short queues of rays, the per-round
budget, the leaf-phase threshold, the lane count at which the wave leaves the walk -- on the corpus of
tests/walk_round_corpus.py, in eleven instantiations: <f64, SCREEN>, <f64, plain>, <f64, ORD, SCREEN>, <f64, ORD, plain>,
<f32, SCREEN> (the EXACT record test), <f32, plain>, <f32, ORD, plain>, and the ANIM twins of the four unordered ones over a
scene with a HitList element (A.leaf_runs, kLeafRun).

  * against the oracle: every ray's closest primitive, the bits of t, its node tests and its primitive tests are the counted
    probe's (oracle_world_hit_counted) -- on the oracle's own tree for the reference mode, on the program's exported tree
    (oracle_set_tree, split axes included) for CR_BVH_SAH_ORDERED;
  * across schedules: the per-ray output is the same bytes under all 90 schedules and 3 lane permutations (implied by the
    first, reported separately: it points at the schedule);
  * the schedules bite: at budget 1 a wave makes at least as many rounds as its busiest lane makes budgeted steps, some wave
    has fewer leaf phases at walk_leaf_min 64 than at 0 while a threshold of 1 never waits (its waves' counts are those of 0),
    some wave leaves the walk at exit 1 with a lane still holding its parked leaf, and the band branch runs in the f64 SCREEN
    kernels and never elsewhere.

The budget binds the loops that step on screening records or with box_miss_fast.  A ray with an infinite 1/direction, and in
the f64 SCREEN kernels one outside screen_in_range, steps with Aabb::hit's compare/select form until it finds a leaf whatever
the budget (the `exact_steps` loop), so the rounds-at-budget-1 bound counts the steps of the other rays."""
import os
import subprocess

import numpy as np
import pytest

import walk_round_corpus as W
from crucible_amd import _abi as A
from test_gpu_shade_primitives import HIPCC
from test_walk_round_corpus import KINDS, MODES, build_corpus, host_tree, probe_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "walk_round_check.hip")
RAY_OUT = np.dtype([("best", "<i4"), ("mat", "<i4"), ("t", "<u8"), ("nodes", "<u4"), ("prims", "<u4")])
WAVE_OUT = np.dtype([("rounds", "<u4"), ("leaf_phases", "<u4"), ("band_lanes", "<u4"), ("survived", "<u4")])
REALS = {"f64": A.CR_REAL_F64, "f32": A.CR_REAL_F32}
SCHED = np.array(W.SCHEDULES)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, oracles, o64):
    """One run of walk_round_check over every case.  -> {(kind, mode, real, kernel): dict}, kernel = "screen" | "plain"."""
    dd = tmp_path_factory.mktemp("walk_round")
    exe = dd / "walk_round_check"
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)
    corpus = build_corpus(dd, o64)
    cases = []
    for kind, modes in KINDS.items():
        c = corpus[kind]
        c["table"] = W.assignments(len(c["rows"]))
        for mode in modes:
            for tag, rt in REALS.items():
                tree, scene_bytes = host_tree(corpus["exe"], dd, c["flat"], rt, MODES[mode])
                path = dd / f"{kind}_{mode}_{tag}"
                W.write_case(path, scene_bytes, c["rows"], c["table"])
                cases.append((kind, mode, tag, path, tree))
    r = subprocess.run([str(exe)] + [str(p) for _, _, _, p, _ in cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for kind, mode, tag, path, tree in cases:
        c = corpus[kind]
        n, (P, B) = len(c["rows"]), c["table"].shape[:2]
        raw = (path / "tree.out").read_bytes()
        ne = int(np.frombuffer(raw, "<i4", 1)[0])
        boxes = np.frombuffer(raw, "<f8", ne * 6, 4).reshape(ne, 6)
        tail = np.frombuffer(raw, "<i4", ne * 3, 4 + ne * 48)
        exported = (boxes, tail[:2 * ne].reshape(ne, 2), tail[2 * ne:])
        for a, b in zip(exported, tree):   # the program built the tree the host tree code builds
            assert np.array_equal(a, b), (kind, mode, tag)
        want = probe_all(oracles[REALS[tag]], c["flat"], c["rows"], None if mode == "ref" else exported)
        for kernel in ("screen", "plain"):
            f = path / f"{kernel}.out"
            if not f.exists():
                assert (kernel, mode, tag) == ("screen", "ord", "f32")   # the f32 kernels screen unordered trees only
                continue
            raw = np.fromfile(f, dtype=np.uint8)
            cut = len(SCHED) * P * n * RAY_OUT.itemsize
            out[(kind, mode, tag, kernel)] = {"rays": raw[:cut].view(RAY_OUT).reshape(len(SCHED), P, n), "want": want, "names": c["names"],
                                              "waves": raw[cut:].view(WAVE_OUT).reshape(len(SCHED), P, B), "table": c["table"]}
    return out


def label(key):
    kind, mode, tag, kernel = key
    return f"<{tag}, {'ANIM, ' if kind == 'list' else ''}{'ORD, ' if mode == 'ord' else ''}{'SCREEN' if kernel == 'screen' else 'plain'}> on the {kind} scene"


def test_the_eleven_instantiations_ran(runs):
    got = {(tag, kind == "list", mode == "ord", kernel == "screen") for kind, mode, tag, kernel in runs if kind != "two"}
    want = {("f64", False, False, True), ("f64", False, False, False), ("f64", False, True, True), ("f64", False, True, False),
            ("f32", False, False, True), ("f32", False, False, False), ("f32", False, True, False),
            ("f64", True, False, True), ("f64", True, False, False), ("f32", True, False, True), ("f32", True, False, False)}
    assert got == want
    total = sum(r["rays"].size for r in runs.values())
    print(f"\n[walk_round] {len(runs)} kernel runs (11 instantiations; 7 more on the two-primitive scene), "
          f"{len(SCHED)} schedules x {len(W.PERM_SEEDS)} permutations each: {total} walks")


def test_every_ray_equals_the_counted_oracle_probe(runs):
    for key, r in runs.items():
        got, want = r["rays"][0, 0], r["want"]
        hit = got["best"] >= 0
        ok = (hit == want["hit"]) & (got["nodes"] == want["nodes"]) & (got["prims"] == want["prims"])
        dev = got["t"].astype(np.uint64 if want["t"].dtype == np.float64 else np.uint32).view(want["t"].dtype)
        same_t = (got["t"] == want["bits"]) | (np.isnan(dev) & np.isnan(want["t"]))   # as same_bits: equal, or both not a number
        ok &= ~hit | ((got["mat"] == want["mat"]) & same_t)
        bad = np.flatnonzero(~ok)
        assert len(bad) == 0, (f"{label(key)}: {len(bad)} rays differ from the oracle; first: group {r['names'][bad[0]]}, ray {bad[0]}: device "
                               f"{got[bad[0]]}, oracle hit {want['hit'][bad[0]]} mat {want['mat'][bad[0]]} t bits {want['bits'][bad[0]]} "
                               f"nodes {want['nodes'][bad[0]]} prims {want['prims'][bad[0]]}")
        assert hit.any() and not hit.all()


def test_output_is_byte_identical_across_schedules_and_permutations(runs):
    for key, r in runs.items():
        first = r["rays"][0, 0]
        for s in range(len(SCHED)):
            for p in range(r["rays"].shape[1]):
                if r["rays"][s, p].tobytes() != first.tobytes():
                    bad = np.flatnonzero(r["rays"][s, p] != first)
                    raise AssertionError(f"{label(key)}: schedule (budget, leaf_min, exit) = {tuple(SCHED[s])}, permutation {p}: {len(bad)} rays differ "
                                         f"from schedule {tuple(SCHED[0])}; first: group {r['names'][bad[0]]}: {r['rays'][s, p][bad[0]]} != {first[bad[0]]}")


def budgeted_steps(key, r):
    """Per permutation, block and lane: the node tests of the lane's rays that step under the budget."""
    _, _, tag, kernel = key
    free = W.EXACT_GROUPS + (W.UNSCREENED_GROUPS if (tag, kernel) == ("f64", "screen") else ())
    nodes = np.where(np.isin(r["names"], free), 0, r["rays"][0, 0]["nodes"].astype(np.int64))
    table = r["table"]
    return np.where(table >= 0, nodes[np.maximum(table, 0)], 0).sum(axis=-1)   # (P, B, 64)


def test_the_schedules_bite(runs):
    """Without this the schedule matrix could be vacuous."""
    survived_waves = band_waves = fewer_waves = 0
    for key, r in runs.items():
        kind, mode, tag, kernel = key
        waves = r["waves"]
        busiest = budgeted_steps(key, r).max(axis=-1)   # (P, B)
        for s in np.flatnonzero(SCHED[:, 0] == 1):
            assert (waves[s]["rounds"] >= busiest).all(), (label(key), tuple(SCHED[s]), waves[s]["rounds"], busiest)
        by = {tuple(x): i for i, x in enumerate(SCHED)}
        fewer = sum(int((waves[by[(b, 64, e)]]["leaf_phases"] < waves[by[(b, 0, e)]]["leaf_phases"]).sum()) for b in W.BUDGETS for e in W.EXITS)
        survived = int((waves[SCHED[:, 2] == 1]["survived"] > 0).sum())
        assert (waves[SCHED[:, 1] == 0]["survived"] == 0).all(), label(key)   # walk_leaf_min 0: a leaf is tested in the round that found it
        # a leaf phase waits for walk_leaf_min parked lanes: with 1 it never waits -- the waves' counts are those of 0
        for b in W.BUDGETS:
            for e in W.EXITS:
                assert waves[by[(b, 1, e)]].tobytes() == waves[by[(b, 0, e)]].tobytes(), (label(key), "walk_leaf_min 1 is not 0", b, e)
        band = waves["band_lanes"]
        if (tag, kernel) == ("f64", "screen"):
            assert (band.sum(axis=-1) > 0).all(), label(key)   # every launch: the band rays are in it
            band_waves += int((band > 0).sum())
        else:
            assert (band == 0).all(), label(key)
        if kind != "two":   # (two primitives: every ray parks on the root at once)
            assert fewer > 0, label(key)
            assert survived > 0, label(key)
        fewer_waves += fewer
        survived_waves += survived
    print(f"\n[walk_round] waves (per launch) that left the walk with a parked leaf at exit 1: {survived_waves}; with a band step: {band_waves}; "
          f"with fewer leaf phases at walk_leaf_min 64 than at 0: {fewer_waves}")
