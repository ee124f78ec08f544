"""A call's result never depends on what its handle did before.

A CrHandle carries grow-only buffers that are reused at smaller sizes, the camera-key and frame-time rings, cached trees
and flags, and NaN bits inside its accumulators from one call to the next (crucible_amd/csrc/handle.hpp).  The jobs of
tests/history_jobs.py -- the 24 cr_render_* entry points and the "dirtiers" built to leave the most behind -- are run here

  fresh      each on a handle of its own: the reference of the job, with the render-family frames pinned to the oracle in
             both sum orders and the guide frames to tests/test_gpu_aov.py's model;
  in pairs   every job after every dirtier, on a fresh handle per pair: the same bytes as fresh;
  in walks   seeded random sequences of 40 steps on one handle -- jobs, dirtiers, uploads of the other scene, refused calls
             (each followed by a plain job) --, every result compared with the fresh one of the scene then uploaded; after a
             walk cr_build_info, cr_frame_build_info, cr_export_bvh and cr_export_render_bvh equal those of a fresh handle
             that ran only the last upload and the last renders;
  elsewhere  the render family's pairs on CRUCIBLE_PIPELINE=wavefront and =queue handles (the wf_* buffers, the queue's
             abort word) and under a CRUCIBLE_WORK_COUNTER_MAX that cuts every job into several launches.

Device-form calls are queued without a synchronise and read when their sequence has ended.  Everything is compared as
bytes; a failure names the dirtier or the walk's seed and step, the job, the step of the job and the first byte."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import history_jobs as J
import test_gpu_aov as aov
from crucible_amd import _abi as A

pytestmark = pytest.mark.gpu

WALK_SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)
WALK_STEPS = 40
ENVS = {"wavefront": {"CRUCIBLE_PIPELINE": "wavefront"}, "queue": {"CRUCIBLE_PIPELINE": "queue"},
        "work-counter": {"CRUCIBLE_WORK_COUNTER_MAX": str(J.SMALL_WORK_COUNTER)}}


def open_session(lib, key, monkeypatch=None, env=None):
    """A handle of its own with base scene `key`; env: read by cr_create, gone again before the first call."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return J.Session(lib, key)
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)


class Fresh:
    """The result of each job on a handle that has done nothing else, computed once."""

    def __init__(self, lib):
        self.lib, self.cache = lib, {}

    def __call__(self, key, job, monkeypatch=None, env_name=None):
        at = (env_name, key, job.name)
        if at not in self.cache:
            with open_session(self.lib, key, monkeypatch, ENVS.get(env_name)) as s:
                s.run(job)
                self.cache[at] = s.collect()[0]
        return self.cache[at]


@pytest.fixture(scope="module")
def fresh(hiplib):
    return Fresh(hiplib)


def fail_with(lines, head):
    if lines:
        text = "\n".join([head] + lines[:40])
        print(text)
        raise AssertionError(f"{head}: {len(lines)} differences, the first: {lines[0]}")


# ------------------------------------------------------------------ exports
def export_tree(lib, h, fn, rt):
    n = C.c_int32()
    rc = fn(h, rt, None, None, None, 0, C.byref(n))
    if rc != A.CR_OK:
        return (rc, (lib.cr_last_error(h) or b"").decode())
    boxes = np.zeros((max(1, n.value), 6), dtype=np.float64)
    kids = np.zeros((max(1, n.value), 2), dtype=np.int32)
    axis = np.full(max(1, n.value), -1, dtype=np.int32)
    rc = fn(h, rt, boxes.ctypes.data_as(C.c_void_p), kids.ctypes.data_as(C.c_void_p), axis.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    return (rc, n.value, boxes[:n.value].tobytes(), kids[:n.value].tobytes(), axis[:n.value].tobytes())


def tree_arrays(exported):
    rc, n, boxes, kids, axis = exported
    assert rc == A.CR_OK
    return (np.frombuffer(boxes, dtype=np.float64).reshape(n, 6).copy(), np.frombuffer(kids, dtype=np.int32).reshape(n, 2).copy(),
            np.frombuffer(axis, dtype=np.int32).copy())


def build_info(lib, h, fn, rt):
    info = A.CrBuildInfo()
    rc = fn(h, rt, C.byref(info))
    if rc != A.CR_OK:
        return (rc, (lib.cr_last_error(h) or b"").decode())
    return (rc, {k: v for k, v in info.as_dict().items() if not k.endswith("_ms")})


def ends(s):
    """What the four inspection calls answer for both precisions (times left out).  The render trees first: cr_build_info
    and cr_export_bvh build a tree that is not built yet."""
    lib, out = s.lib, {}
    for rt in (J.F64, J.F32):
        out[f"export_render_bvh {J.TAG[rt]}"] = export_tree(lib, s.h, lib.cr_export_render_bvh, rt)
        out[f"frame_build_info {J.TAG[rt]}"] = build_info(lib, s.h, lib.cr_frame_build_info, rt)
        out[f"build_info {J.TAG[rt]}"] = build_info(lib, s.h, lib.cr_build_info, rt)
        out[f"export_bvh {J.TAG[rt]}"] = export_tree(lib, s.h, lib.cr_export_bvh, rt)
    return out


# ------------------------------------------------------------------ fresh results
def scene_of(call):
    sc = copy.copy(J.base_scene("A"))
    sc.scene_cam = J.camera_of(sc, call)
    return sc


@pytest.fixture(scope="module")
def base_trees(hiplib):
    """The trees of scene A as the device walks them, for the oracle."""
    with J.Session(hiplib, "A") as s:
        return {rt: tree_arrays(export_tree(s.lib, s.h, s.lib.cr_export_bvh, rt)) for rt in (J.F64, J.F32)}


# (a frame tree has the frame's boxes: the same picture, other counters than on the base tree)
RENDER_FRAMES = [j for j in J.RENDER_JOBS if j.steps[0].shape == "one" and j.steps[0].host and not j.steps[0].shard and not j.steps[0].refit]


@pytest.mark.parametrize("job", RENDER_FRAMES, ids=[j.name for j in RENDER_FRAMES])
def test_fresh_render_frames_equal_the_oracle(fresh, oracles, base_trees, job):
    """Both precisions, both sum orders: the reference every pair and walk is held to is itself the oracle's frame."""
    call = job.steps[0]
    res = fresh("A", job)[0]
    assert res["rc"] == A.CR_OK, res["msg"]
    want, ost = oracles[call.rt].render_image(scene_of(call), seed=J.SEED, tree=base_trees[call.rt], sum_order=call.sum_order)
    got = J.output_array(res, call)[0]
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f"{job.name}: {int((got != want).sum())} values differ from the oracle"
    samples, segments, node_tests, prim_tests, _ = res["stats"]
    assert samples == J.W * J.H * call.n_samples
    assert (segments, node_tests, prim_tests) == (ost["segments"], ost["node_tests"], ost["prim_tests"])


def test_the_orders_are_both_there():
    assert {(j.steps[0].rt, j.steps[0].sum_order) for j in RENDER_FRAMES} >= {(rt, o) for rt in (J.F32, J.F64) for o in (J.RELAX, J.REFERENCE)}


@pytest.mark.parametrize("name", ["render_aov_host-f64", "render_aov_host-f32"])
def test_fresh_guide_frames_equal_the_model(fresh, oracles, base_trees, name):
    job = J.BY_NAME[name]
    call = job.steps[0]
    res = fresh("A", job)[0]
    assert res["rc"] == A.CR_OK, res["msg"]
    want, _ = aov.model(oracles[call.rt], scene_of(call), J.SEED, tree=base_trees[call.rt])
    buf = J.output_array(res, call)
    o = 0
    for plane, _, c in A.AOV_LAYERS:
        n = J.W * J.H * c
        assert buf[o:o + n].tobytes() == want[plane].tobytes(), plane
        o += n
    assert res["stats"][:2] == (J.W * J.H * call.n_samples,) * 2      # samples == segments: primary rays only


def test_fresh_results_are_results(fresh):
    """Every job of the table runs: calls that are meant to succeed do, on both scenes, and the refusals are the recorded ones."""
    with open(J.refusal_gen.PATH) as f:
        golden = json.load(f)["refusals"]
    for key in ("A", "B"):
        for job in J.TABLE:
            for k, (step, res) in enumerate(zip(job.steps, fresh(key, job))):
                ok = (A.CR_OK, A.CR_ERR_NAN) if isinstance(step, J.Call) and step.nan_camera and step.host and not step.output_sum and not step.guide else (A.CR_OK,)
                assert res["rc"] in ok, (key, job.name, k, step, res["rc"], res["msg"])
                if isinstance(step, J.Call):
                    n, w, h = step.extent() if step.scene is None else (1, 0, 0)
                    if step.scene is None:
                        assert len(res["out"]) == n * w * h * step.channels() * np.dtype(step.out_dtype()).itemsize
                if isinstance(step, J.Refusals) and key == "A":
                    assert res["refusals"] == {k: golden[k] for k in res["refusals"]}, step.entry
    nan = J.BY_NAME["nan-frames"]
    for step, res in zip(nan.steps, fresh("A", nan)):
        if step.family in ("render", "adaptive"):
            out = np.frombuffer(res["out"], dtype=step.out_dtype())
            assert ((out >> np.uint64(63)) == 1).all() if step.output_sum == J.FIXED else np.isnan(out).all(), step
    mixed = J.BY_NAME["adaptive-mixed"]
    for step, res in zip(mixed.steps, fresh("A", mixed)):
        blocks, stopped = res["stats"][-2:]
        assert 0 < stopped < blocks, (step, res["stats"])


# ------------------------------------------------------------------ pairs
def run_pairs(lib, fresh, dirtier, jobs, monkeypatch=None, env_name=None):
    lines = []
    for job in jobs:
        with open_session(lib, "A", monkeypatch, ENVS.get(env_name)) as s:
            s.run(dirtier)
            s.run(job)
            first, second = s.collect()
        if job is jobs[0]:      # the dirtier itself is a job like any other: once per dirtier
            lines += [f"[{dirtier.name} run twice on fresh handles] {line}" for line in J.differences(first, fresh("A", dirtier, monkeypatch, env_name), dirtier)]
        lines +=[f"[after {dirtier.name}] {line}" for line in J.differences(second, fresh("A", job, monkeypatch, env_name), job)]
    fail_with(lines, f"after the dirtier {dirtier.name}")


@pytest.mark.parametrize("dirtier", J.DIRTIERS, ids=[j.name for j in J.DIRTIERS])
def test_pairs(hiplib, fresh, dirtier):
    """Every job of the table straight after the dirtier, a fresh handle per pair."""
    run_pairs(hiplib, fresh, dirtier, J.TABLE)


@pytest.mark.parametrize("env_name", list(ENVS))
def test_render_family_pairs_elsewhere(hiplib, fresh, monkeypatch, env_name):
    """The render family's pairs on a handle of another pipeline (reference-order frames; what such a handle refuses it
    refuses the same way after any dirtier) and under a work counter that holds four samples of a frame."""
    dirtiers = J.RENDER_DIRTIERS if env_name == "work-counter" else J.PIPELINE_DIRTIERS
    ran = 0
    for job in J.RENDER_JOBS:
        ran += sum(res["rc"] == A.CR_OK for res in fresh("A", job, monkeypatch, env_name))
    assert ran >= (len(J.RENDER_JOBS) if env_name == "work-counter" else 4), ran
    for dirtier in dirtiers:
        run_pairs(hiplib, fresh, dirtier, J.RENDER_JOBS, monkeypatch, env_name)


# ------------------------------------------------------------------ walks
END_JOBS = tuple(J.Job(f"end-{k}", tuple(c for rt in (J.F64, J.F32) for c in (J.Call("render", "one", True, rt, frame=2, refit="rebuild"), last(rt))))
                 for k, last in enumerate((lambda rt: J.Call("render", "one", True, rt), lambda rt: J.Call("aov", "one", True, rt, frame=0, refit=True),
                                           lambda rt: J.Call("render", "one", False, rt, frame=0, refit="rebuild"))))
REFUSAL_JOBS = tuple(J.Job("refusals-" + e, (J.Refusals(e),)) for e in J.refusal_gen.ENTRIES)


def walk_plan(seed, steps=WALK_STEPS):
    """The sequence of a seed: ("upload", key), ("job", Job) and ("refused", Job) entries; a refused call is followed by the
    plain check job."""
    rs = np.random.RandomState(seed)
    plan, key = [], "A"
    while len(plan) < steps:
        u = rs.uniform()
        if u < 0.10:
            key = "B" if key == "A" else "A"
            plan.append(("upload", key))
        elif u < 0.22:
            plan.append(("refused", REFUSAL_JOBS[rs.randint(len(REFUSAL_JOBS))]))
            plan.append(("job", J.PLAIN_CHECK))
        elif u < 0.50:
            plan.append(("job", J.DIRTIERS[rs.randint(len(J.DIRTIERS))]))
        else:
            plan.append(("job", J.PLAIN[rs.randint(len(J.PLAIN))]))
    return plan[:steps], END_JOBS[rs.randint(len(END_JOBS))]


def run_walk(lib, fresh, plan, end, what):
    """Runs the plan on one handle; returns (lines of differences, the ends of the walk, the ends of a fresh handle)."""
    ran = []
    with J.Session(lib, "A") as s:
        for k, (kind, arg) in enumerate(plan):
            if kind == "upload":
                s.upload(arg)
            else:
                s.run(arg)
                ran.append((k, s.key, arg))
        s.run(end)
        ran.append((len(plan), s.key, end))
        results = s.collect()
        after = ends(s)
        last_key = s.key
    lines = []
    for (k, key, job), got in zip(ran, results):
        lines += [f"[{what}, step {k}, scene {key}] {line}" for line in J.differences(got, fresh(key, job), job)]
    with J.Session(lib, last_key) as s:
        s.run(end)
        s.collect()
        alone = ends(s)
    return lines, after, alone


_walks = {}


def walked(lib, fresh, seed):
    if seed not in _walks:
        plan, end = walk_plan(seed)
        _walks[seed] = run_walk(lib, fresh, plan, end, f"walk seed {seed}")
    return _walks[seed]


def test_walk_plans_mix_everything():
    kinds = {"upload": 0, "refused": 0, "dirtier": 0, "plain": 0}
    for seed in WALK_SEEDS:
        plan, _ = walk_plan(seed)
        assert len(plan) == WALK_STEPS
        for kind, arg in plan:
            kinds[kind if kind != "job" else ("dirtier" if arg.dirtier else "plain")] += 1
    assert len(WALK_SEEDS) >= 8 and all(n >= 8 for n in kinds.values()), kinds


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_walk(hiplib, fresh, seed):
    lines, _, _ = walked(hiplib, fresh, seed)
    fail_with(lines, f"walk seed {seed}")


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_ends_of_a_walk(hiplib, fresh, seed):
    """The trees and build records after a walk are those of a handle that only ran the last upload and the last renders."""
    _, after, alone = walked(hiplib, fresh, seed)
    assert sorted(after) == sorted(alone)
    bad = [k for k in after if after[k] != alone[k]]
    for k in bad:
        print(f"walk seed {seed}: {k}: {str(after[k])[:200]} != {str(alone[k])[:200]}")
    assert not bad, f"walk seed {seed}: {bad}"
    for rt in ("f64", "f32"):
        assert after[f"export_render_bvh {rt}"][0] == A.CR_OK and after[f"frame_build_info {rt}"][1]["n_wrappers"] > 0


# ------------------------------------------------------------------ named sequences (regressions found by the walks go here)
NAMED = {
    # a frame tree, an edit, the same frame again: the frame tree must not be the one from before the edit
    "rebuild-edit-rebuild": (("job", J.BY_NAME["refits"]), ("job", J.BY_NAME["updates"]), ("job", J.BY_NAME["refits"]), ("job", J.PLAIN_CHECK)),
    # every flag word set, then every family at the same size and smaller
    "nan-then-every-family": (("job", J.BY_NAME["nan-frames"]),) + tuple(("job", j) for j in J.PLAIN),
    # the largest buffers of every kind, another scene, the table
    "grown-then-uploaded": (("job", J.BY_NAME["more-pixels"]), ("job", J.BY_NAME["more-frames"]), ("upload", "B")) + tuple(("job", j) for j in J.PLAIN),
}


@pytest.mark.parametrize("name", list(NAMED))
def test_named_sequence(hiplib, fresh, name):
    lines, after, alone = run_walk(hiplib, fresh, list(NAMED[name]), END_JOBS[2], name)
    fail_with(lines, name)
    assert after == alone
