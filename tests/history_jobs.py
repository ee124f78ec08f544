"""The job table of tests/test_gpu_history.py, tests/test_gpu_handle_memory.py and tests/test_history_jobs_host.py.

A job is a short fixed list of steps on a fixed small scene: render calls with fixed arguments (a `Call`), uploads,
cr_update_primitives edits and refused calls.  Running it on a handle returns, step by step, everything the step hands back
as bytes: the output planes, the count plane, samples and the four work counters of CrStats, passes / blocks /
blocks_stopped of CrAdaptiveStats, the status and the text of cr_last_error.  Times are left out.  A device-form call
writes into torch tensors of its own and is not followed by a synchronise: `Session.collect()` reads them when the
sequence has ended.

PLAIN has one job per entry point and precision: the 24 cr_render_* calls (render, guide layers, adaptive, guide layers
at a count plane; frame, batch, region; host and device), the frame shape of every family in f32 and f64.  DIRTIERS are
built to leave the most behind on a handle (handle.hpp: grow-only buffers reused at smaller sizes, the camera-key and
frame-time rings, the cached trees and flags, the NaN bits inside the accumulators); each is larger than every plain job
in the dimension it dirties.  tests/test_history_jobs_host.py asserts on the CPU, with the oracle and the models, that each
dirtier reaches the state it is named for.

The scenes: "A" is scenes.moving_scene under CR_BVH_SAH (keyed primitives that leave their boxes, no list elements, so
refits, frame trees and edits all apply), "B" is scenes.scaled_scene under CR_BVH_SAH_ORDERED built on the device.  Every
job runs on either; a job that uploads something else ends by uploading the session's scene again."""
import copy
import ctypes as C
import importlib.util
import os
from dataclasses import dataclass, replace

import numpy as np

import far_corpus
import scenes
import update_model as um
from crucible_amd import _abi as A
from crucible_amd.scene import LERP, WORLD

F32, F64 = A.CR_REAL_F32, A.CR_REAL_F64
RELAX, REFERENCE, FIXED = A.CR_SUM_RELAXED, A.CR_SUM_REFERENCE_ORDER, A.CR_OUTPUT_FIXED_SUM
SEED = 0x4157
W, H = 37, 29                      # no multiple of the 4 x 4 tile or of the 8-pixel block: edge tiles and edge blocks are partial
SAMPLES, AD_SAMPLES = 6, 16        # of a plain job: a render or guide call, an adaptive call
BIG_W, BIG_H = 96, 75              # the dirtiers: more pixels ...
MANY_FRAMES = (2, 0, 1, 3, 1)      # ... more frames (a plain batch has two) ...
MANY_SAMPLES, AD_MANY_SAMPLES = 16, 32   # ... and more samples than any plain job
FRAMES = (1, 2)
REGION = (0, 8, 32, 16)            # its origin on a multiple of the block
BLOCK = 8
SHORT_SHUTTER = 90.0              # a quarter of the scenes' exposure
# The noise target of every adaptive job.  Chosen once, with the oracle's words and tests/adaptive_model.py, so that on scene A
# some blocks stop early and some run to the maximum in every shape, at 16 and at 32 samples, in f32 and f64
# (tests/test_history_jobs_host.py asserts it).
TOLERANCE = 0.08
MANY_TOLERANCE = 0.03            # ... of the call with 32 samples, whose means are quieter
COUNTERS = ("samples", "segments", "node_tests", "prim_tests", "texel_fetches")
NP_REAL = {F32: np.float32, F64: np.float64}
TAG = {F32: "f32", F64: "f64"}
DEVICE = A.CR_BVH_BUILD_DEVICE
TREE_MODES = (A.CR_BVH_REFERENCE, A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED, A.CR_BVH_LBVH, A.CR_BVH_SAH | DEVICE, A.CR_BVH_SAH_ORDERED | DEVICE)


def _refusal_generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_entry_refusals.py")
    spec = importlib.util.spec_from_file_location("make_entry_refusals", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


refusal_gen = _refusal_generator()


# ------------------------------------------------------------------ scenes
def base_scene(key):
    """The scene a session renders, sized and in its tree mode."""
    if key == "A":
        sc = scenes.moving_scene(samples=SAMPLES, frame=1)
        sc.bvh_mode = A.CR_BVH_SAH
    else:
        assert key == "B", key
        sc = scenes.scaled_scene(samples=SAMPLES, frame=1)
        sc.bvh_mode = A.CR_BVH_SAH_ORDERED | DEVICE
    sc.scene_cam.image_width, sc.scene_cam.image_height = W, H
    return sc


def other_scene(name, mode):
    """A scene a dirtier uploads in the session scene's place."""
    if name == "lists":            # list elements, no images
        sc = scenes.list_scene(samples=2, frame=1)
    elif name == "images":         # image textures and a spherical sky, no list elements
        sc = scenes.mixed_scene(samples=2, animate=True)
    elif name == "plain":          # neither
        sc = scenes.few_spheres(7, samples=2)
    elif name == "near":
        sc = far_corpus.static_scene("near")
    else:
        sc = far_corpus.static_scene(name)
    sc.bvh_mode = mode
    if name in ("lists", "images", "plain"):
        sc.scene_cam.image_width, sc.scene_cam.image_height = 41, 23
    return sc


# ------------------------------------------------------------------ steps
@dataclass(frozen=True)
class Call:
    """One cr_render_* call.  `scene`: None renders the session's scene with its camera; a name renders other_scene(name)
    (which an Upload step has put on the handle) with that scene's camera."""
    family: str                    # "render", "aov", "adaptive", "counts"
    shape: str                     # "one", "frames", "region"
    host: bool
    rt: int = F64
    order: int = None              # None: relaxed sums for renders and adaptive calls, CR_SUM_DEFAULT for guide calls
    size: tuple = (W, H)
    samples: int = None            # None: SAMPLES, AD_SAMPLES for an adaptive call
    frame: int = 1
    frames: tuple = FRAMES
    region: tuple = REGION
    layers: int = A.CR_AOV_ALL
    refit: object = False          # False, True, "rebuild"
    shutter: float = None          # the shutter angle; None: the scene's (360 degrees: frame f draws ray times in [f, f + 1])
    output_sum: int = 0
    shard: tuple = None            # (sample_begin, sample_count)
    min_samples: int = 4
    pass_samples: int = 2
    tolerance: float = TOLERANCE
    counts: str = "random"         # the count plane of a "counts" call: count_plane's kinds
    nan_camera: bool = False       # look_from == look_at: every pixel is NaN
    cam_keys: int = None           # camera_keys' set
    scene: str = None
    stats: bool = None             # None: the host forms and the adaptive calls ask for stats, the other device forms do not (and stay asynchronous)

    @property
    def entry(self):
        return ("cr_render" + {"render": "", "aov": "_aov", "adaptive": "_adaptive", "counts": "_aov_counts"}[self.family]
                + {"one": "", "frames": "_frames", "region": "_region"}[self.shape] + ("_host" if self.host else "_device"))

    @property
    def n_samples(self):
        return self.samples if self.samples is not None else (AD_SAMPLES if self.family == "adaptive" else SAMPLES)

    @property
    def sum_order(self):
        if self.order is not None:
            return self.order
        return RELAX if self.family in ("render", "adaptive") else A.CR_SUM_DEFAULT

    @property
    def guide(self):
        return self.family in ("aov", "counts")

    def extent(self):
        """(frames, width, height) of the output."""
        w, h = (self.region[2], self.region[3]) if self.shape == "region" else self.size
        return (len(self.frames) if self.shape == "frames" else 1), w, h

    def channels(self):
        if not self.guide:
            return 3
        return sum(c for _, bit, c in A.AOV_LAYERS if self.layers & bit)

    def out_dtype(self):
        return np.uint64 if self.output_sum == FIXED else NP_REAL[self.rt]

    def wants_stats(self):
        return self.stats if self.stats is not None else (self.host or self.family == "adaptive")


@dataclass(frozen=True)
class Upload:
    """cr_upload_scene of other_scene(name, mode); name None: the session's own scene again."""
    name: str = None
    mode: int = 0


@dataclass(frozen=True)
class Update:
    """cr_update_primitives of the session's scene: update_model.seeded_edit's rows, or (restore) the uploaded coordinates
    of the same primitives."""
    rebuild: bool
    restore: bool = False
    seed: int = um.EDIT_SEED


@dataclass(frozen=True)
class HostileUpdate:
    """far_corpus.hostile_edit on the uploaded "near" scene: a sphere whose f32 box is inf - inf (DevScene::nan_planes)."""
    rebuild: bool = True


@dataclass(frozen=True)
class Refusals:
    """Every refusal tests/golden/entry_refusals.json records for one entry point, replayed on the session's scene."""
    entry: str


@dataclass(frozen=True)
class Job:
    name: str
    steps: tuple
    dirtier: bool = False

    @property
    def render_family_only(self):
        return all(isinstance(s, Call) and s.family == "render" and s.scene is None for s in self.steps)


def camera_keys(cam, k):
    """Camera-key set k: look_from and look_at travel to their own points during frame 1."""
    cam.look_from_tl.translate_point((0.4 * k - 1.5, 3.0 + 0.15 * k, 9.0 - 0.2 * k), 1.25 + 0.05 * k, LERP, WORLD)
    cam.look_at_tl.translate_point((0.1 * k, 0.7, 0.05 * k), 1.5, LERP, WORLD)


def camera_of(sc, call):
    """The camera of `call` on the scene `sc` (a copy: the scene's own stays as it is)."""
    cam = copy.deepcopy(sc.scene_cam)
    if call.scene is None:
        cam.image_width, cam.image_height = call.size
        cam.set_samples(call.n_samples)
        cam.frame = call.frame
    cam.refit_boxes = call.refit
    if call.shutter is not None:
        cam.shutter_angle = float(call.shutter)
    if call.nan_camera:
        cam.look_from((1.0, 2.0, 3.0))
        cam.look_at((1.0, 2.0, 3.0))
    if call.cam_keys is not None:
        camera_keys(cam, call.cam_keys)
    return cam


def count_plane(kind, shape, samples):
    """The (frames, h, w) int32 plane of a guide call at a count plane.  "steps": 0, 1 and `samples` (and a value between)
    in neighbouring pixels, shifted from row to row and frame to frame; "random": seeded values in [0, samples]."""
    n, h, w = shape
    if kind == "steps":
        f, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
        return np.array([0, 1, samples, samples // 2], dtype=np.int32)[(x + y + f) % 4]
    assert kind == "random", kind
    return np.random.RandomState(n * 7919 + h * 31 + w).randint(0, samples + 1, size=shape).astype(np.int32)


# ------------------------------------------------------------------ the table
def _frame_jobs():
    """Every entry point once, the frame shape of each family in both precisions and both forms."""
    jobs = []
    for family in ("render", "aov", "adaptive", "counts"):
        for shape in ("one", "frames", "region"):
            for host in (True, False):
                reals = (F64, F32) if shape == "one" else ((F64,) if host else (F32,))
                for rt in reals:
                    call = Call(family, shape, host, rt)
                    jobs.append(Job(f"{call.entry[3:]}-{TAG[rt]}", (call,)))
    return jobs


PLAIN = tuple(_frame_jobs()) + (
    Job("render_host-f64-shard-fixed", (Call("render", "one", True, F64, shard=(2, 3), output_sum=FIXED),)),
    Job("render_aov_host-f32-albedo-depth", (Call("aov", "one", True, F32, layers=A.CR_AOV_ALBEDO | A.CR_AOV_DEPTH),)),
    Job("render_host-f32-frame0", (Call("render", "one", True, F32, frame=0),)),
    # frame trees of frame 0 over two exposures: the same first ray time, another last one
    Job("render_host-f64-rebuild", (Call("render", "one", True, F64, frame=0, refit="rebuild"),)),
    Job("render_host-f32-rebuild", (Call("render", "one", True, F32, frame=0, refit="rebuild"),)),
    Job("render_host-f64-rebuild-short", (Call("render", "one", True, F64, frame=0, refit="rebuild", shutter=SHORT_SHUTTER),)),
    Job("render_host-f32-rebuild-short", (Call("render", "one", True, F32, frame=0, refit="rebuild", shutter=SHORT_SHUTTER),)),
)


def _nan_frames():
    """look_from == look_at through the relaxed render, the guide layers and the adaptive call, at the largest plain size:
    bit 63 of every fixed-point word and every flag word of the buffers stay set behind it.  The host render asks for the
    fixed-point words (the mean of such a frame is refused with CR_ERR_NAN once it has been copied out: the adaptive host
    form shows that)."""
    steps = []
    for rt in (F64, F32):
        steps += [Call("render", "one", True, rt, nan_camera=True, output_sum=FIXED),
                  Call("render", "one", False, rt, nan_camera=True),
                  Call("render", "frames", True, rt, nan_camera=True, output_sum=FIXED),
                  Call("aov", "one", True, rt, nan_camera=True),
                  Call("aov", "frames", False, rt, nan_camera=True),
                  Call("adaptive", "one", True, rt, nan_camera=True),
                  Call("adaptive", "frames", False, rt, nan_camera=True),
                  Call("counts", "one", True, rt, nan_camera=True, counts="steps")]
    return tuple(steps)


def _uploads():
    """Another scene in each tree mode -- with list elements, with images, with neither --, rendered in both precisions so
    that both trees are built, then the session's scene again."""
    steps = []
    for k, mode in enumerate(TREE_MODES):
        name = ("lists", "images", "plain")[k % 3]
        steps += [Upload(name, mode), Call("render", "one", True, (F64, F32)[k % 2], REFERENCE, scene=name),
                  Call("aov", "one", False, (F32, F64)[k % 2], scene=name)]
    steps += [Upload("images", A.CR_BVH_REFERENCE), Call("render", "one", True, F32, scene="images"), Upload()]
    return tuple(steps)


def _refusals():
    return tuple(Refusals(e) for e in refusal_gen.ENTRIES)


DIRTIERS = (
    Job("more-pixels", tuple(Call(f, "one", host, rt, size=(BIG_W, BIG_H), samples=2 if f != "adaptive" else 8, counts="steps")
                             for f in ("render", "aov", "adaptive", "counts") for host, rt in ((True, F64), (False, F32))), True),
    Job("more-frames", tuple(Call(f, "frames", host, rt, frames=MANY_FRAMES) for f in ("render", "aov", "adaptive", "counts")
                             for host, rt in ((True, F32), (False, F64))), True),
    Job("more-samples", (Call("render", "one", True, F64, samples=MANY_SAMPLES), Call("render", "one", False, F32, samples=MANY_SAMPLES),
                         Call("aov", "one", True, F64, samples=MANY_SAMPLES), Call("render", "one", True, F32, REFERENCE, samples=MANY_SAMPLES),
                         Call("adaptive", "one", True, F64, samples=AD_MANY_SAMPLES, min_samples=8, pass_samples=4, tolerance=MANY_TOLERANCE),
                         Call("counts", "one", False, F32, samples=MANY_SAMPLES, counts="steps")), True),
    Job("nan-frames", _nan_frames(), True),
    # the reference order fills sample_buf and sg_acc, which the relaxed renders beside it do without
    Job("reference-order", (Call("render", "one", True, F64, REFERENCE, samples=MANY_SAMPLES), Call("render", "one", True, F64),
                            Call("render", "one", False, F32, REFERENCE, samples=MANY_SAMPLES), Call("render", "one", True, F32)), True),
    Job("adaptive-mixed", (Call("adaptive", "one", True, F64), Call("adaptive", "region", True, F64), Call("adaptive", "frames", True, F64),
                           Call("adaptive", "one", False, F32), Call("adaptive", "region", False, F32), Call("adaptive", "frames", False, F32)), True),
    Job("count-plane-steps", (Call("counts", "one", True, F64, counts="steps"), Call("counts", "frames", False, F64, counts="steps"),
                              Call("counts", "region", True, F32, counts="steps"), Call("counts", "one", False, F32, counts="steps")), True),
    # refitted boxes and frame trees: two different frames, then the same frame twice (the frame tree is reused), then the
    # same frame under a shorter exposure (the same first ray time: a frame tree the next full exposure must not reuse)
    Job("refits", tuple(Call(f, "one", host, rt, frame=frame, refit=refit, shutter=shutter) for rt in (F64, F32)
                        for f, host, frame, refit, shutter in (("render", True, 0, True, None), ("render", True, 2, "rebuild", None), ("aov", True, 0, "rebuild", None),
                                                               ("render", False, 0, "rebuild", None), ("render", True, 0, "rebuild", None), ("render", True, 2, True, None),
                                                               ("render", True, 0, "rebuild", SHORT_SHUTTER))), True),
    # boxes beyond the f32 range (screen_overflow set, screen_usable cleared) and an f32 tree with a NaN plane
    Job("far-boxes", (Upload("edge_out", A.CR_BVH_REFERENCE), Call("render", "one", True, F64, scene="edge_out"), Call("render", "one", True, F32, scene="edge_out"),
                      Call("aov", "one", True, F64, scene="edge_out"),
                      Upload("far", A.CR_BVH_SAH), Call("render", "one", True, F64, REFERENCE, scene="far"),
                      Upload("near", A.CR_BVH_SAH), Call("render", "one", True, F32, scene="near"), HostileUpdate(True),
                      Call("render", "one", True, F32, scene="near"), Call("render", "one", True, F64, scene="near"), Upload()), True),
    Job("updates", (Call("render", "one", True, F64), Call("render", "one", True, F32),
                    Update(False), Call("render", "one", True, F64), Call("render", "one", False, F32), Update(False, restore=True),
                    Update(True), Call("render", "one", True, F32), Call("aov", "one", True, F64), Update(True, restore=True)), True),
    Job("uploads", _uploads(), True),
    # two laps of the four-slot camera-key ring plus one; then the frame-times ring: three batches of different lengths
    Job("queued", tuple(Call("render", "one", False, (F64, F32)[k % 2], cam_keys=k) for k in range(9))
        + (Call("render", "frames", False, F64, frames=(0, 1, 2, 3)), Call("render", "frames", False, F64, frames=(3,)),
           Call("aov", "frames", False, F32, frames=(2, 1, 0))), True),
    Job("refusals", _refusals(), True),
)

TABLE = PLAIN + DIRTIERS
BY_NAME = {j.name: j for j in TABLE}
assert len(BY_NAME) == len(TABLE)
PLAIN_CHECK = BY_NAME["render_host-f64"]    # the plain job a refused call is followed by


def render_only(job, order=None):
    """The job's render-family calls on the session's scene; order=REFERENCE: its whole-frame renders alone, in the
    reference order (what the wavefront and LDS-queue pipelines implement; fixed-point words become sums in reals)."""
    steps = [s for s in job.steps if isinstance(s, Call) and s.family == "render" and s.scene is None]
    if order == REFERENCE:
        steps = [replace(s, order=REFERENCE, output_sum=1 if s.output_sum == FIXED else s.output_sum) for s in steps if s.shape == "one"]
    return Job(job.name + ("-render" if order is None else "-reference"), tuple(steps), job.dirtier)


def _unique(jobs):
    seen, out = set(), []
    for j in jobs:
        if j.steps and j.steps not in seen:
            seen.add(j.steps)
            out.append(j)
    return tuple(out)


_RENDER_DIRTIERS = ("more-pixels", "more-frames", "more-samples", "nan-frames", "reference-order", "refits", "queued")
# the render family alone, as the megakernel runs it under a small work counter ...
RENDER_JOBS = _unique([j for j in PLAIN if j.render_family_only] + [render_only(j, REFERENCE) for j in PLAIN if j.render_family_only])
RENDER_DIRTIERS = _unique(render_only(BY_NAME[n]) for n in _RENDER_DIRTIERS)
# ... and as the cross-check pipelines run it: reference-order frames (the relaxed jobs stay in the list: their refusal is a result too)
PIPELINE_JOBS = RENDER_JOBS
PIPELINE_DIRTIERS = _unique(render_only(BY_NAME[n], REFERENCE) for n in _RENDER_DIRTIERS)
BY_NAME.update({j.name: j for j in RENDER_JOBS + RENDER_DIRTIERS + PIPELINE_DIRTIERS})
SMALL_WORK_COUNTER = 6000          # CRUCIBLE_WORK_COUNTER_MAX: a 37 x 29 frame's 80 tiles x 64 items fit once: every four samples are a launch


def entry_points(jobs):
    return {s.entry for j in jobs for s in j.steps if isinstance(s, Call)}


# ------------------------------------------------------------------ running jobs on a handle
class Session:
    """One handle with one of the base scenes on it.  run(job) makes the job's calls; collect() synchronises once and
    returns every job's results in order: per step a dict with "rc" and "msg", and for a call that ran its "out", "counts"
    and "stats" (None where the call has none)."""

    def __init__(self, lib, key="A", upload=True):
        self.lib, self.key = lib, key
        self.sc = base_scene(key)
        self.flat = self.sc.flatten()
        self.original = um.prim_arrays(self.flat)[2].copy()
        h = C.c_void_p()
        rc = lib.cr_create(0, C.byref(h))
        if rc != A.CR_OK:
            raise RuntimeError("cr_create: " + (lib.cr_last_error(None) or b"").decode())
        self.h = h
        self.others = {}
        self.current = None            # the other scene on the handle, None: the session's own
        self.pending = []
        self.keep = []
        if upload:
            self.upload(self.key)

    def close(self):
        if self.h:
            self.lib.cr_destroy(self.h)
            self.h = None
        self.keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def message(self):
        return (self.lib.cr_last_error(self.h) or b"").decode()

    def upload(self, key):
        """Another base scene takes the session over."""
        if key != self.key:
            self.key, self.sc = key, base_scene(key)
            self.flat = self.sc.flatten()
            self.original = um.prim_arrays(self.flat)[2].copy()
        self.current = None
        rc = self.lib.cr_upload_scene(self.h, C.byref(self.flat.desc))
        if rc != A.CR_OK:
            raise RuntimeError("cr_upload_scene: " + self.message())

    # -- steps
    def _upload_step(self, step):
        if step.name is None:
            flat, self.current = self.flat, None
        else:
            sc = other_scene(step.name, step.mode)
            flat = sc.flatten()
            self.others[step.name] = (sc, flat)
            self.current = step.name
        rc = self.lib.cr_upload_scene(self.h, C.byref(flat.desc))
        return {"rc": rc, "msg": self.message() if rc != A.CR_OK else ""}

    def _update(self, idx, rows, rebuild):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        rc = self.lib.cr_update_primitives(self.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), rows.ctypes.data_as(C.POINTER(C.c_double)), len(idx),
                                           A.CR_UPDATE_REBUILD if rebuild else A.CR_UPDATE_REFIT)
        return {"rc": rc, "msg": self.message() if rc != A.CR_OK else ""}

    def _update_step(self, step):
        idx, rows = um.seeded_edit(self.flat, step.seed)
        if step.restore:
            kind = um.prim_arrays(self.flat)[0]
            rows = self.original[idx].copy()
            rows[kind[idx] == A.CR_PRIM_SPHERE, 4:] = np.nan
        return self._update(idx, rows, step.rebuild)

    def _hostile_step(self, step):
        idx, rows, _ = far_corpus.hostile_edit(self.others["near"][1])
        return self._update(idx, rows, step.rebuild)

    def _refusal_step(self, step):
        import torch
        gen = refusal_gen
        family, shape, host = gen.ENTRIES[step.entry]
        cam = copy.deepcopy(self.sc.scene_cam)
        cam.image_width, cam.image_height = gen.W, gen.H
        cam.set_samples(gen.SAMPLES)
        if host:
            out, counts = np.zeros(gen.OUT_BYTES, dtype=np.uint8), np.zeros(2 * gen.W * gen.H, dtype=np.int32)
            ptrs = out.ctypes.data, counts.ctypes.data
        else:
            out = torch.empty(gen.OUT_BYTES, dtype=torch.uint8, device="cuda")
            counts = torch.empty(2 * gen.W * gen.H, dtype=torch.int32, device="cuda")
            ptrs = out.data_ptr(), counts.data_ptr()
        self.keep += [out, counts]
        answers = {}
        for name in gen.case_names(family, shape):
            call = gen.Call(cam)
            for f in name.split("+"):
                call.fault(f)
            rc = call.run(self.lib, self.h, step.entry, ptrs[0], ptrs[1], None)
            answers[f"{step.entry}/{name}"] = {"status": rc, "message": self.message()}
        return {"rc": A.CR_OK, "msg": "", "refusals": answers}

    def _call_step(self, call):
        import torch
        sc = self.sc if call.scene is None else self.others[call.scene][0]
        assert call.scene == self.current, (call.scene, self.current)
        cam = camera_of(sc, call)
        if call.scene is not None:
            call = replace(call, size=(cam.image_width, cam.image_height), samples=cam.samples)
        n, w, h = call.extent()
        cd = cam.desc()
        begin, count = call.shard if call.shard else (0, None)
        p = cam.params(SEED, call.rt, begin, count, call.output_sum, call.sum_order)
        n_out = n * w * h * call.channels()
        want_counts = call.family == "adaptive"
        plane = count_plane(call.counts, (n, h, w), call.n_samples) if call.family == "counts" else None
        if call.host:
            out = np.zeros(n_out, dtype=call.out_dtype())
            counts = np.zeros(n * w * h, dtype=np.int32) if want_counts else None
            out_ptr, counts_ptr = C.c_void_p(out.ctypes.data), (C.c_void_p(counts.ctypes.data) if want_counts else None)
            plane_ptr = C.c_void_p(plane.ctypes.data) if plane is not None else None
        else:
            # torch.empty launches nothing: no fill kernel of torch's stream can land after the handle's stream has written
            out = torch.empty(n_out * np.dtype(call.out_dtype()).itemsize, dtype=torch.uint8, device="cuda")
            counts = torch.empty(n * w * h, dtype=torch.int32, device="cuda") if want_counts else None
            out_ptr, counts_ptr = C.c_void_p(out.data_ptr()), (C.c_void_p(counts.data_ptr()) if want_counts else None)
            plane_ptr = None
            if plane is not None:
                d_plane = torch.from_numpy(plane).to("cuda")
                torch.cuda.current_stream().synchronize()   # torch's copy, on torch's stream: the handle's stream is not waited for
                self.keep.append(d_plane)
                plane_ptr = C.c_void_p(d_plane.data_ptr())
        st = (A.CrAdaptiveStats() if call.family == "adaptive" else A.CrStats()) if call.wants_stats() else None
        args = [self.h, C.byref(cd), C.byref(p)]
        keep = [cd, p, plane]
        if call.guide:
            args.append(call.layers)
        if call.family == "adaptive":
            ap = A.CrAdaptiveParams(call.min_samples, call.pass_samples, 3, 0, call.tolerance)
            keep.append(ap)
            args.append(C.byref(ap))
        if call.shape == "frames":
            fr = (C.c_int32 * len(call.frames))(*call.frames)
            keep.append(fr)
            args += [fr, len(call.frames)]
        if call.shape == "region":
            reg = A.CrRegion(*call.region)
            keep.append(reg)
            args.append(C.byref(reg))
        if call.family == "counts":
            args.append(plane_ptr)
        args.append(out_ptr)
        if call.family == "adaptive":
            args.append(counts_ptr)
        args.append(C.byref(st) if st is not None else None)
        rc = getattr(self.lib, call.entry)(*args)
        self.keep.append(keep)
        res = {"rc": rc, "msg": self.message() if rc != A.CR_OK else "", "out": None, "counts": None, "stats": None}
        if rc in (A.CR_OK, A.CR_ERR_NAN):    # CR_ERR_NAN: a host form's pixel check, after everything has been copied out
            res["out"], res["counts"] = out, counts
            if st is not None:
                render = st.render if call.family == "adaptive" else st
                res["stats"] = tuple(int(getattr(render, c)) for c in COUNTERS)
                if call.family == "adaptive":
                    res["stats"] += (int(st.passes), int(st.blocks), int(st.blocks_stopped))
        return res

    def run(self, job):
        steps = []
        for step in job.steps:
            if isinstance(step, Call):
                steps.append(self._call_step(step))
            elif isinstance(step, Upload):
                steps.append(self._upload_step(step))
            elif isinstance(step, Update):
                steps.append(self._update_step(step))
            elif isinstance(step, HostileUpdate):
                steps.append(self._hostile_step(step))
            else:
                steps.append(self._refusal_step(step))
        self.pending.append(steps)
        return steps

    def collect(self):
        """Every run() since the last collect(), the device outputs read after one synchronise of the handle's stream."""
        rc = self.lib.cr_synchronize(self.h)
        if rc != A.CR_OK:
            raise RuntimeError("cr_synchronize: " + self.message())
        done = []
        for steps in self.pending:
            for res in steps:
                for k in ("out", "counts"):
                    v = res.get(k)
                    if v is not None and not isinstance(v, (bytes, np.ndarray)):
                        v = v.cpu().numpy()
                    if isinstance(v, np.ndarray):
                        res[k] = v.tobytes()
            done.append(steps)
        self.pending, self.keep = [], []
        return done


def differences(got, want, job):
    """What differs between two results of `job`, as a list of lines (empty: the same bytes everywhere)."""
    lines = []
    assert len(got) == len(want) == len(job.steps)
    for k, (g, w, step) in enumerate(zip(got, want, job.steps)):
        for key in sorted(set(g) | set(w)):
            a, b = g.get(key), w.get(key)
            if a == b:
                continue
            what = f"{job.name} step {k} ({getattr(step, 'entry', type(step).__name__)}) {key}"
            if isinstance(a, bytes) and isinstance(b, bytes) and len(a) == len(b):
                x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
                bad = np.nonzero(x != y)[0]
                lines.append(f"{what}: {len(bad)} of {len(a)} bytes differ, the first at byte {int(bad[0])}, the last at byte {int(bad[-1])}")
            elif key == "refusals":
                lines += [f"{what} {n}: {a.get(n)} != {b.get(n)}" for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
            else:
                lines.append(f"{what}: {a!r} != {b!r}"[:400])
    return lines


def output_array(res, call, key="out"):
    """A collected result's output as an array: (frames, h, w, channels) for a render or an adaptive call, the flat buffer
    of a guide call; key="counts": (frames, h, w) int32."""
    n, w, h = call.extent()
    if key == "counts":
        return np.frombuffer(res["counts"], dtype=np.int32).reshape(n, h, w)
    a = np.frombuffer(res["out"], dtype=call.out_dtype())
    return a if call.guide else a.reshape(n, h, w, 3)
