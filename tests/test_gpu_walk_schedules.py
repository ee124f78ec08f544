"""The walk's scheduling knobs are speed only: whatever CRUCIBLE_WALK_ROUND (wrappers a lane steps through per round),
CRUCIBLE_WALK_EXIT (lanes done walking at which the wave leaves the walk) and CRUCIBLE_WALK_LEAF_MIN (parked lanes a leaf
phase waits for) are set to, every lane performs BVHWrapper::hit's own sequence -- so every kernel the library can select
computes the same image and the same work counters, bit for bit, under every schedule.

  (a) every cell of tests/test_gpu_variants.py (RES / SCREEN / ORD / ANIM / CAMK / RELAX / LATENCY) under three of the nine
      SCHEDULES, by a rota that brings every selection under every schedule;
  (b) a spheres-only scene (the uniform_kind == 0 path and the other set of default knobs) under all nine, and the teapot
      (triangles) under three;
  (c) the guide pass (aov_kernel.hpp walks with the same knobs, the leaf-phase threshold among them) against the Python
      model of tests/test_gpu_aov.py;
  (d) the LDS-queue pipeline, which takes the round budget and must ignore the leaf-phase threshold;
  (e) the region, adaptive and adaptive-batch calls against the same calls on a handle with default knobs.
The handle reads the knobs in cr_create, so every render makes a fresh Renderer."""
import collections

import numpy as np
import pytest

import test_gpu_aov as G
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene, load_teapot, procedural_sky
from crucible_amd.renderer import Renderer
from test_gpu_adaptive import median_tolerance, pass_words
from test_gpu_variants import (CELLS, EXTRA_SELECTIONS, F32, F64, KINDS, REF, RELAX, SELECTIONS, WINDOW, matrix_scene,
                               render_cell, same)

REALS = [(F64, "f64"), (F32, "f32")]
KNOBS = ("CRUCIBLE_WALK_ROUND", "CRUCIBLE_WALK_EXIT", "CRUCIBLE_WALK_LEAF_MIN")
Schedule = collections.namedtuple("Schedule", "name env")


def schedule(rnd, ext, leaf_min):
    """(round, exit, leaf_min); None leaves the knob at the library's per-scene default."""
    vals = (rnd, ext, leaf_min)
    name = "-".join("d" if v is None else str(v) for v in vals)
    return Schedule(name, {k: str(v) for k, v in zip(KNOBS, vals) if v is not None})


# api.hip clamps exit to [1, 64] and leaf_min to [0, 64]; round 0 is unbounded
SCHEDULES = [schedule(1, 1, 0), schedule(1, 64, 64), schedule(0, 64, 0), schedule(0, 1, 64), schedule(3, 33, 1),
             schedule(1000, 40, 63), schedule(2, 64, 8), schedule(None, None, 0), schedule(None, None, 64)]
BY_NAME = {s.name: s for s in SCHEDULES}
ROTA = [[SCHEDULES[(3 * i + j) % 9] for j in range(3)] for i in range(len(CELLS))]
SEED = 0xC0FFEE


def set_schedule(monkeypatch, env):
    """The environment of one Renderer: the schedule's knobs, and none left over from the render before."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_schedules_stay_inside_the_accepted_ranges():
    assert len(SCHEDULES) == 9 and len(BY_NAME) == 9
    for s in SCHEDULES:
        assert set(s.env) <= set(KNOBS)
        assert 0 <= int(s.env.get("CRUCIBLE_WALK_ROUND", 0))
        assert 1 <= int(s.env.get("CRUCIBLE_WALK_EXIT", 1)) <= 64
        assert 0 <= int(s.env["CRUCIBLE_WALK_LEAF_MIN"]) <= 64   # every schedule names the leaf-phase threshold
    assert not any(k in c.env for c in CELLS for k in KNOBS)   # no cell sets a knob of its own


def test_the_rota_brings_every_selection_under_every_schedule():
    """3 of 9 schedules per cell: every selection (its 8 cells) meets all nine, and every schedule meets both sum orders, all
    four scene kinds, both precisions and both tree orders."""
    names = [s.name for s in SELECTIONS + EXTRA_SELECTIONS]
    assert len(CELLS) == 8 * len(names) == 224 and all(len({s.name for s in row}) == 3 for row in ROTA)
    met = collections.defaultdict(set)
    seen = collections.defaultdict(lambda: collections.defaultdict(set))
    for i, (cell, row) in enumerate(zip(CELLS, ROTA)):
        sel = names[i // 8]
        assert cell.id.startswith(sel + "-" + cell.scene)
        for s in row:
            met[sel].add(s.name)
            for what in ("relax", "scene", "real", "ord", "res", "kind"):
                seen[s.name][what].add(getattr(cell, what))
    assert all(met[n] == set(BY_NAME) for n in names), {n: sorted(set(BY_NAME) - met[n]) for n in names if met[n] != set(BY_NAME)}
    for s in SCHEDULES:
        got = seen[s.name]
        assert got["relax"] == {False, True} and got["scene"] == set(KINDS) and got["real"] == {F64, F32}
        assert got["ord"] == {False, True} and len(got["res"]) == 3 and got["kind"] == {"static", "CAMK", "ANIM"}
    print(f"\n[walk schedules (a)] {len(CELLS)} cells x 3 of {len(SCHEDULES)} schedules = {3 * len(CELLS)} renders")


# ------------------------------------------------------------------ (a) the megakernel cells
@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CELLS)), ids=[c.id for c in CELLS])
def test_kernel_variant_under_three_schedules(monkeypatch, oracles, index):
    cell = CELLS[index]
    batch = cell.relax and cell.kind in ("ANIM", "CAMK")
    for s in ROTA[index]:
        set_schedule(monkeypatch, {})
        try:
            render_cell(monkeypatch, oracles, dict(cell.env, **s.env), matrix_scene(cell.scene), cell.real, RELAX if cell.relax else REF,
                        cell.ord, cell.scene_in_lds, batch)
        except AssertionError as e:
            raise AssertionError(f"schedule {s.name} (round-exit-leaf_min): {e}") from e


# ------------------------------------------------------------------ (b) other scene shapes
@pytest.fixture(scope="module")
def references(oracles):
    """Oracle renders and guide-layer models, computed once and shared by the schedules."""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]
    return get


def spheres_scene():
    return book1_end_scene(1, scene_seed=1, image_width=100, samples=5)


def teapot_scene():
    return load_teapot(1, image_width=96, samples=3, sky=procedural_sky(256, 128))


def render_against_oracle(monkeypatch, references, oracles, env, name, make, rt, **kw):
    sc = make()
    ref, rst = references((name, rt), lambda: oracles[rt].render_image(sc, seed=SEED))
    set_schedule(monkeypatch, env)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        img, st = r.render(sc.scene_cam, seed=SEED, real_type=rt, **kw)
    finally:
        r.close()
    same(img, st, ref, rst, name)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("s", SCHEDULES, ids=[s.name for s in SCHEDULES])
def test_spheres_only_scene(monkeypatch, references, oracles, s, rt, tag):
    """No triangles: uniform_kind == 0, and the defaults an unset knob falls back to are the sphere scenes' (10, 56)."""
    st = render_against_oracle(monkeypatch, references, oracles, s.env, "book1", spheres_scene, rt)
    assert st["scene_in_lds"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("s", [BY_NAME["1-1-0"], BY_NAME["0-1-64"], BY_NAME["1000-40-63"]], ids=["1-1-0", "0-1-64", "1000-40-63"])
def test_teapot(monkeypatch, references, oracles, s, rt, tag):
    """6320 triangles and a ground sphere, the top of the tree in LDS."""
    st = render_against_oracle(monkeypatch, references, oracles, s.env, "teapot", teapot_scene, rt)
    assert st["scene_in_lds"] == 2 and st["bvh_entries"] == 8191


# ------------------------------------------------------------------ (c) the guide pass
@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("s", SCHEDULES, ids=[s.name for s in SCHEDULES])
def test_guide_layers(monkeypatch, references, oracles, s, rt, tag):
    for kind in ("static", "anim"):
        sc = matrix_scene(kind)
        want = references(("guide", kind, rt), lambda: G.model(oracles[rt], sc, G.SEED)[0])
        for res_name, res_env, in_lds in (("default", {}, 1), ("window", WINDOW, 2)):
            set_schedule(monkeypatch, dict(res_env, **s.env))
            r = Renderer(0)
            try:
                r.upload_scene(sc.flatten())
                got, st = r.render_aov(sc.scene_cam, seed=G.SEED, real_type=rt)
            finally:
                r.close()
            for k in res_env:
                monkeypatch.delenv(k)
            assert sorted(got) == sorted(G.NAMES) and st["scene_in_lds"] == in_lds, (kind, res_name, st["scene_in_lds"])
            G.same(got, want, f"{kind}, {res_name} residency, schedule {s.name}:")


# ------------------------------------------------------------------ (d) the LDS-queue pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
@pytest.mark.parametrize("rnd", [0, 1, 3, 1000])
def test_queue_pipeline(monkeypatch, references, oracles, rnd, rt, tag):
    """The walker waves take the round budget; the leaf-phase threshold is the megakernel's and the guide pass's alone
    (render.hip sets it to 0 for the other pipelines, whose rounds test a leaf where they find it)."""
    env = {"CRUCIBLE_PIPELINE": "queue", "CRUCIBLE_WALK_ROUND": str(rnd), "CRUCIBLE_WALK_LEAF_MIN": "64"}
    for kind in ("static", "anim"):
        render_against_oracle(monkeypatch, references, oracles, env, "matrix-" + kind, lambda: matrix_scene(kind), rt, sum_order=REF)


# ------------------------------------------------------------------ (e) listed and region kernels
def integers(st):
    """The integer fields of a stats dict (nested ones flattened): everything but the clocks."""
    out = {}
    for k, v in st.items():
        if isinstance(v, dict):
            out.update({f"{k}.{n}": x for n, x in integers(v).items()})
        elif isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            out[k] = int(v)
    return out


def region_and_adaptive_calls(r, sc, rt, tolerance):
    """What the three calls return, as bytes and integer stats.  tolerance: None = the one at which about half the blocks stop
    at their first judgement (test_gpu_adaptive's median over the blocks, from the handle's own sample-shard renders)."""
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    if tolerance is None:
        tolerance = median_tolerance(pass_words(r, cam, rt, 2), 2, 4, cam.samples, 8)
    out = {"tolerance": tolerance}
    img, st = r.render_region(cam, (5, 3, 13, 9), seed=SEED, real_type=rt, sum_order=RELAX)
    out["region"] = (img.tobytes(), b"", integers(st))
    kw = dict(seed=SEED, real_type=rt, tolerance=tolerance, min_samples=4, pass_samples=2, block=8, sum_order=RELAX)
    img, counts, st = r.render_adaptive(cam, **kw)
    out["adaptive"] = (img.tobytes(), counts.tobytes(), integers(st))
    img, counts, st = r.render_adaptive_frames(cam, [0, 1, 2], **kw)
    out["adaptive_frames"] = (img.tobytes(), counts.tobytes(), integers(st))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=[t for _, t in REALS])
def test_region_and_adaptive_calls(monkeypatch, rt, tag):
    """cr_render_region_*, cr_render_adaptive_* and cr_render_adaptive_frames_* (the REGION / listed-tile kernels) on the
    keyed scene at 12 samples per pixel: pixels, count planes and integer stats are those of a handle with default knobs."""
    sc = matrix_scene("anim", samples=12)
    results, tolerance = {}, None
    for name, env in [("default", {})] + [(n, BY_NAME[n].env) for n in ("1-1-0", "0-1-64")]:
        set_schedule(monkeypatch, env)
        r = Renderer(0)
        try:
            results[name] = region_and_adaptive_calls(r, sc, rt, tolerance)
        finally:
            r.close()
        tolerance = results[name].pop("tolerance")
    want = results.pop("default")
    stopped, blocks = want["adaptive"][2]["blocks_stopped"], want["adaptive"][2]["blocks"]
    assert 0 < stopped < blocks, (stopped, blocks)   # a condition on the inputs: the decisions are mixed
    assert want["region"][2]["samples"] == 13 * 9 * 12 and want["adaptive"][2]["render.samples"] >= 24 * 16 * 4
    print(f"\n[walk schedules (e)] {tag}: adaptive stats at default knobs {want['adaptive'][2]}")
    for name, got in results.items():
        for call in want:
            assert got[call][2] == want[call][2], (name, call, got[call][2], want[call][2])
            assert got[call][1] == want[call][1], (name, call, "count planes differ")
            assert got[call][0] == want[call][0], (name, call, "pixels differ")
