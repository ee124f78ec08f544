"""The job table of tests/history_jobs.py, checked on the CPU: it covers the 24 entry points, every dirtier is larger than the
plain jobs in the dimension it dirties, and -- with the oracle, tests/adaptive_model.py and tests/far_corpus.py -- every
dirtier reaches the state it is named for.  A table that stops reaching these states (a dirtier replaced by a plain job, a
tolerance at which no block or every block stops) fails here, without a GPU, and does not pass quietly on one."""
import copy

import numpy as np
import pytest

import adaptive_model as M
import far_corpus
import history_jobs as J
from crucible_amd import _abi as A

FLAG = np.uint64(1 << 63)


def calls(job, **want):
    return [s for s in job.steps if isinstance(s, J.Call) and all(getattr(s, k) == v for k, v in want.items())]


def scene_for(call, frame=None):
    sc = copy.copy(J.base_scene("A"))
    sc.scene_cam = J.camera_of(sc, call)
    if frame is not None:
        sc.scene_cam.frame = frame
    return sc


def oracle_frame(oracles, call, frame=None, **kw):
    return oracles[call.rt].render_image(scene_for(call, frame), seed=J.SEED, **kw)


def pass_words(oracles, call, frame=None):
    """The per-pass fixed-point words of the frame of an adaptive call, from the oracle's relaxed sample shards."""
    P = call.pass_samples
    return np.stack([oracle_frame(oracles, call, frame, sum_order=J.RELAX, output_sum=J.FIXED, sample_begin=p * P, sample_count=P)[0]
                     for p in range(call.n_samples // P)])


def stopped_blocks(oracles, call):
    """(blocks stopped early, blocks) of every frame of an adaptive call, by the model."""
    out = []
    for frame in (call.frames if call.shape == "frames" else (None,)):
        words = pass_words(oracles, call, frame)
        if call.shape == "region":
            x0, y0, w, h = call.region
            words = words[:, y0:y0 + h, x0:x0 + w]
        counts, _, _ = M.adaptive(words, call.pass_samples, call.min_samples, call.n_samples, J.BLOCK, call.tolerance, J.NP_REAL[call.rt])
        rects = M.blocks_of(words.shape[2], words.shape[1], J.BLOCK)
        out.append((sum(1 for x0, y0, _, _ in rects if counts[y0, x0] < call.n_samples), len(rects)))
    return out


# ------------------------------------------------------------------ the states, by dirtier
def more_pixels(job, oracles):
    plain = max(c.extent()[1] * c.extent()[2] for j in J.PLAIN for c in calls(j))
    for family in ("render", "aov", "adaptive", "counts"):
        assert calls(job, family=family, shape="one"), family
    for c in calls(job):
        assert c.extent()[1] * c.extent()[2] > plain and c.size[0] <= 96


def more_frames(job, oracles):
    plain = max(c.extent()[0] for j in J.PLAIN for c in calls(j))
    for family in ("render", "aov", "adaptive", "counts"):
        assert calls(job, family=family, shape="frames"), family
    for c in calls(job):
        assert c.shape == "frames" and c.extent()[0] > plain


def more_samples(job, oracles):
    for family, most in (("render", 16), ("aov", 16), ("adaptive", 32), ("counts", 16)):
        plain = max(c.n_samples for j in J.PLAIN for c in calls(j, family=family))
        mine = calls(job, family=family)
        assert mine and all(plain < c.n_samples <= most for c in mine), family
    for c in calls(job, family="adaptive"):
        for stopped, blocks in stopped_blocks(oracles, c):
            assert 0 < stopped < blocks, (c, stopped, blocks)


def nan_frames(job, oracles):
    for rt in (J.F32, J.F64):
        for family in ("render", "aov", "adaptive"):
            assert calls(job, family=family, rt=rt, nan_camera=True), (family, rt)
        assert calls(job, family="render", rt=rt, host=True, output_sum=J.FIXED)
    assert all(c.nan_camera and c.size == (J.W, J.H) for c in calls(job))
    for c in calls(job, family="render", shape="one", host=True):
        _, st = oracle_frame(oracles, replace_sum(c))
        assert st["nan_pixels"] == J.W * J.H
        words, _ = oracle_frame(oracles, c, sum_order=J.RELAX, output_sum=J.FIXED)
        assert ((words & FLAG) != 0).all()          # bit 63 of every word of the buffer


def replace_sum(call):
    from dataclasses import replace
    return replace(call, output_sum=0)


def reference_order(job, oracles):
    ref, relaxed = calls(job, order=J.REFERENCE), calls(job, order=None)
    assert ref and relaxed and all(c.family == "render" and c.shape == "one" for c in ref + relaxed)
    assert {c.rt for c in ref} == {J.F32, J.F64}
    for c in ref:      # the two orders are two computations: some last bits differ
        a, _ = oracle_frame(oracles, c, sum_order=J.REFERENCE)
        b, _ = oracle_frame(oracles, c, sum_order=J.RELAX)
        assert not np.array_equal(a, b) and not np.isnan(a).any()


def adaptive_mixed(job, oracles):
    for shape in ("one", "frames", "region"):
        assert calls(job, family="adaptive", shape=shape, host=True) and calls(job, family="adaptive", shape=shape, host=False), shape
    for c in calls(job):
        assert c.family == "adaptive"
        for stopped, blocks in stopped_blocks(oracles, c):
            assert 0 < stopped < blocks, (c, stopped, blocks)


def count_plane_steps(job, oracles):
    assert {c.shape for c in calls(job)} == {"one", "frames", "region"}
    for c in calls(job):
        assert c.family == "counts" and c.counts == "steps"
        n, w, h = c.extent()
        plane = J.count_plane(c.counts, (n, h, w), c.n_samples)
        assert plane.dtype == np.int32 and plane.shape == (n, h, w) and plane.min() == 0 and plane.max() == c.n_samples
        for f in range(n):
            rows = plane[f].tolist()
            # 0, 1 and `samples` side by side in one row, somewhere in every frame
            assert any(row[x:x + 3] == [0, 1, c.n_samples] for row in rows for x in range(w - 2)), f


def refits(job, oracles):
    for rt in (J.F32, J.F64):
        mine = calls(job, rt=rt)
        rebuilt = [c.frame for c in mine if c.refit == "rebuild"]
        assert len(set(rebuilt)) >= 2                                      # two different frames ...
        assert any(a == b for a, b in zip(rebuilt, rebuilt[1:]))           # ... and the same frame twice in a row
        assert any(c.refit is True for c in mine)
        # the last frame tree of the precision is frame 0's under the short exposure: CR_REFIT_REBUILD's reuse test sees the
        # same first ray time and another last one when a plain job asks for frame 0 at the full exposure
        last = [c for c in mine if c.refit == "rebuild"][-1]
        assert (last.frame, last.shutter) == (0, J.SHORT_SHUTTER) and J.SHORT_SHUTTER < J.base_scene("A").scene_cam.shutter_angle
        for shutter in (None, J.SHORT_SHUTTER):
            assert any(c.refit == "rebuild" and c.frame == 0 and c.shutter == shutter and c.rt == rt for j in J.PLAIN for c in calls(j)), shutter
    sc = J.base_scene("A")
    assert sc.bvh_mode == A.CR_BVH_SAH and sc.flatten().desc.n_keys > 0    # what CR_REFIT_REBUILD needs; boxes that move
    c = calls(job, refit="rebuild")[0]
    a, _ = oracle_frame(oracles, c, frame=0)
    b, _ = oracle_frame(oracles, c, frame=2)
    assert not np.array_equal(a, b)
    short, _ = oracle_frame(oracles, calls(job, shutter=J.SHORT_SHUTTER)[0])
    assert not np.array_equal(a, short)       # another exposure, another frame


def far_boxes(job, oracles):
    ups = [s for s in job.steps if isinstance(s, J.Upload)]
    assert [u.name for u in ups] == ["edge_out", "far", "near", None]
    plane = far_corpus.largest_plane("edge_out")
    with np.errstate(over="ignore"):
        assert np.isfinite(plane) and plane > far_corpus.FLT_MAX and np.isinf(np.float32(plane))
    flat = J.other_scene("edge_out", 0).flatten()
    assert max(max(flat.prims[i].v) for i in range(flat.desc.n_prims)) == plane
    assert calls(job, scene="edge_out", rt=J.F64) and calls(job, scene="edge_out", rt=J.F32)
    # the hostile edit: a sphere whose f32 box is inf - inf, rendered in f32 after it
    k = next(i for i, s in enumerate(job.steps) if isinstance(s, J.HostileUpdate))
    assert job.steps[k].rebuild and any(isinstance(s, J.Call) and s.rt == J.F32 and s.scene == "near" for s in job.steps[k + 1:])
    _, rows, _ = far_corpus.hostile_edit(J.other_scene("near", A.CR_BVH_SAH).flatten())
    with np.errstate(invalid="ignore", over="ignore"):
        lo = rows[:, 0].astype(np.float32) - rows[:, 3].astype(np.float32)
    assert np.isnan(lo).any() and np.isfinite(rows[:, :4]).all()


def updates(job, oracles):
    ups = [s for s in job.steps if isinstance(s, J.Update)]
    assert [(u.rebuild, u.restore) for u in ups] == [(False, False), (False, True), (True, False), (True, True)]
    steps = list(job.steps)
    for u in ups[0::2]:     # a render between the edit and the edit that restores the coordinates
        k = steps.index(u)
        assert isinstance(steps[k + 1], J.Call)
    flat = J.base_scene("A").flatten()
    original = J.um.prim_arrays(flat)[2]
    idx, rows = J.um.seeded_edit(flat, ups[0].seed)
    assert len(idx) >= 2 and not np.array_equal(rows[:, :3], original[idx][:, :3])


def uploads(job, oracles):
    ups = [s for s in job.steps if isinstance(s, J.Upload)]
    assert ups[-1].name is None
    assert {u.mode for u in ups[:-1]} == set(J.TREE_MODES)
    described = {}
    for u in ups[:-1]:
        flat = J.other_scene(u.name, u.mode).flatten()
        kinds = {flat.prims[i].kind for i in range(flat.desc.n_prims)}
        described[u.name] = (bool(kinds & {A.CR_PRIM_LIST, A.CR_PRIM_BVH}), flat.desc.n_images > 0)
    assert {lists for lists, _ in described.values()} == {True, False}
    assert {images for _, images in described.values()} == {True, False}
    for k, s in enumerate(job.steps[:-1]):
        if isinstance(s, J.Upload):
            assert isinstance(job.steps[k + 1], J.Call) and job.steps[k + 1].scene == s.name


def queued(job, oracles):
    singles = calls(job, shape="one")
    assert len(singles) == 9 and all(not c.host and not c.wants_stats() for c in singles)      # two laps of the four-slot ring plus one
    assert len({c.cam_keys for c in singles}) == 9 and None not in {c.cam_keys for c in singles}
    images = [oracle_frame(oracles, c, sum_order=J.RELAX)[0].tobytes() for c in singles if c.rt == J.F32]
    assert len(set(images)) == len(images)                                                     # nine key sets, nine frames
    batches = calls(job, shape="frames")
    assert len(batches) == 3 and len({len(c.frames) for c in batches}) == 3 and all(not c.host for c in batches)
    assert list(job.steps[:9]) == singles and list(job.steps[9:]) == batches                   # back to back


def refusals(job, oracles):
    import json
    with open(J.refusal_gen.PATH) as f:
        golden = json.load(f)["refusals"]
    mine = {f"{s.entry}/{n}" for s in job.steps for n in J.refusal_gen.case_names(*J.refusal_gen.ENTRIES[s.entry][:2])}
    assert mine == set(golden) and all(golden[k]["status"] != A.CR_OK for k in mine)


STATES = {"more-pixels": more_pixels, "more-frames": more_frames, "more-samples": more_samples, "nan-frames": nan_frames,
          "reference-order": reference_order, "adaptive-mixed": adaptive_mixed, "count-plane-steps": count_plane_steps, "refits": refits,
          "far-boxes": far_boxes, "updates": updates, "uploads": uploads, "queued": queued, "refusals": refusals}


def test_every_dirtier_has_a_state():
    assert [j.name for j in J.DIRTIERS] == list(STATES) and all(j.dirtier for j in J.DIRTIERS) and not any(j.dirtier for j in J.PLAIN)


@pytest.mark.parametrize("name", list(STATES))
def test_dirtier_reaches_the_state_it_is_named_for(oracles, name):
    STATES[name](J.BY_NAME[name], oracles)


@pytest.mark.parametrize("name", list(STATES))
def test_a_plain_job_in_a_dirtiers_place_is_noticed(oracles, name):
    """What the check above is worth: the plain render in the dirtier's place does not reach the state."""
    with pytest.raises((AssertionError, StopIteration, IndexError)):
        STATES[name](J.PLAIN_CHECK, oracles)


def test_the_table_covers_the_entry_points():
    entries = J.entry_points(J.PLAIN)
    assert len(entries) == 24 and entries <= set(J.refusal_gen.ENTRIES) | {e for e in entries if "_aov_counts" in e}
    assert len([e for e in entries if e.endswith("_host")]) == 12 and len([e for e in entries if e.endswith("_device")]) == 12
    for family in ("render", "aov", "adaptive", "counts"):
        for host in (True, False):
            assert {c.rt for j in J.PLAIN for c in calls(j, family=family, shape="one", host=host)} == {J.F32, J.F64}, (family, host)
    for j in J.TABLE:
        for c in calls(j):
            assert c.size[0] <= 96 and c.n_samples <= (32 if c.family == "adaptive" else 16), (j.name, c)
            if not c.host and c.family != "adaptive":
                assert not c.wants_stats(), (j.name, c)          # asynchronous: no stats, no synchronise
    assert J.PIPELINE_DIRTIERS and J.RENDER_DIRTIERS and all(j.render_family_only for j in J.RENDER_JOBS + J.RENDER_DIRTIERS + J.PIPELINE_DIRTIERS)
    assert any(c.order == J.REFERENCE for j in J.PIPELINE_JOBS for c in calls(j))


@pytest.mark.parametrize("rt", [J.F64, J.F32], ids=["f64", "f32"])
def test_a_plain_frame_is_a_picture(oracles, rt):
    """No NaN and not constant: a stale NaN bit or a frame that was never written would show against it."""
    for job in J.PLAIN:
        for c in calls(job, family="render", shape="one", rt=rt, output_sum=0):
            img, st = oracle_frame(oracles, c, sum_order=J.RELAX)
            assert st["nan_pixels"] == 0 and not np.isnan(img).any()
            assert len(np.unique(img.reshape(-1, 3), axis=0)) > J.W * J.H // 4
