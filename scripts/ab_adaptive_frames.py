"""What a batch does for adaptive passes (profiles/experiments/adaptive_frames.txt).  One JSON line on stdout.
  python scripts/ab_adaptive_frames.py [--frames 48] [--spp 64] [--pass-samples 8] [--min-samples 16] [--block 16]
                                       [--tolerances 0.02,0.01] [--batches 4,8,16] [--reps 5]
first_movie's shape (the teapot orbit movie's keyed camera at 400x225, depth 5), f64, relaxed sums, frames 0 .. F-1:
  A  one cr_render_adaptive_host call per frame (the existing entry point, never the batch call with one frame),
  B  cr_render_adaptive_frames_host with each of --batches frames per call,
alternated A, B4, B8, B16, A, ... `--reps` times in one process on one handle after a warm-up of every mode.  Per mode and
tolerance: wall ms per frame (the host calls, copies back included) of every repeat, kernel ms and judge ms per frame, the
passes (launches of the render kernel) over all frames, the share of the fixed count's samples taken.  Every frame and count
plane of every mode must hash to mode A's.  Context: the fixed-count cr_render_host per frame and cr_render_frames_host
batched, at --spp."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import procedural_sky, teapot_orbit_movie  # noqa: E402
from crucible_amd.renderer import LIB_PATH, Renderer  # noqa: E402

SEED = 0xC0FFEE
KW = dict(seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)


def adaptive_all(r, cam, n_frames, per_call, akw):
    """Frames 0 .. n_frames-1 to the noise target, per_call frames per call (0: the single-frame entry point).  The frames are
    hashed after the clock stops."""
    kept, tot = [], {"kernel_ms": 0.0, "judge_ms": 0.0, "passes": 0, "samples": 0}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f0 in range(0, n_frames, max(1, per_call)):
        if per_call == 0:
            cam.frame = f0
            img, counts, st = r.render_adaptive(cam, **akw, **KW)
            img, counts = img[None], counts[None]
        else:
            img, counts, st = r.render_adaptive_frames(cam, list(range(f0, min(n_frames, f0 + per_call))), **akw, **KW)
        tot["kernel_ms"] += st["render"]["kernel_ms"]; tot["judge_ms"] += st["judge_ms"]
        tot["passes"] += st["passes"]; tot["samples"] += st["render"]["samples"]
        kept.append((img, counts))
    tot["wall_ms"] = (time.perf_counter() - t0) * 1e3
    tot["md5"] = hashlib.md5(b"".join(i.tobytes() for i, _ in kept) + b"".join(c.tobytes() for _, c in kept)).hexdigest()   # all frames, then all count planes
    return tot


def fixed_all(r, cam, n_frames, per_call):
    kernel_ms = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f0 in range(0, n_frames, max(1, per_call)):
        if per_call == 0:
            cam.frame = f0
            _, st = r.render(cam, **KW)
        else:
            _, st = r.render_frames(cam, list(range(f0, min(n_frames, f0 + per_call))), **KW)
        kernel_ms += st["kernel_ms"]
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": kernel_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--pass-samples", type=int, default=8)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--tolerances", default="0.02,0.01")
    ap.add_argument("--batches", default="4,8,16")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sc = teapot_orbit_movie(1, image_width=400, samples=a.spp, sky=procedural_sky())
    cam = sc.scene_cam
    cam.set_max_depth(5)
    F = a.frames
    modes = [0] + [int(b) for b in a.batches.split(",")]
    fixed_samples = cam.image_width * cam.image_height * a.spp * F
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        out = {"lib": LIB_PATH, "device": torch.cuda.get_device_name(0),
               "shape": f"teapot orbit movie {cam.image_width}x{cam.image_height}, at most {a.spp} spp, depth {cam.max_depth}, {F} frames, f64, relaxed",
               "pass_samples": a.pass_samples, "min_samples": a.min_samples, "block": a.block, "reps": a.reps, "adaptive": [], "fixed": {}}
        for tol in (float(t) for t in a.tolerances.split(",")):
            akw = dict(tolerance=tol, min_samples=a.min_samples, pass_samples=a.pass_samples, block=a.block)
            for m in modes:   # warm-up: tree build, buffers grown, first launches of every mode
                adaptive_all(r, cam, min(F, max(2, m)), m, akw)
            runs = {m: [] for m in modes}
            for _ in range(a.reps):
                for m in modes:   # alternated
                    runs[m].append(adaptive_all(r, cam, F, m, akw))
            ref = runs[0][0]["md5"]
            rec = {"tolerance": tol, "modes": {}}
            for m in modes:
                walls = [x["wall_ms"] / F for x in runs[m]]
                rec["modes"]["per-frame" if m == 0 else str(m)] = {
                    "wall_ms_per_frame": walls, "wall_ms_per_frame_median": statistics.median(walls),
                    "kernel_ms_per_frame_median": statistics.median(x["kernel_ms"] / F for x in runs[m]),
                    "judge_ms_per_frame_median": statistics.median(x["judge_ms"] / F for x in runs[m]),
                    "passes": runs[m][0]["passes"], "samples_taken": runs[m][0]["samples"], "share_of_fixed": runs[m][0]["samples"] / fixed_samples,
                    "equal_to_per_frame": all(x["md5"] == ref for x in runs[m])}
            base = rec["modes"]["per-frame"]["wall_ms_per_frame_median"]
            for m in modes[1:]:
                rec["modes"][str(m)]["wall_speedup"] = base / rec["modes"][str(m)]["wall_ms_per_frame_median"]
            out["adaptive"].append(rec)
        fmodes = [0, max(modes)]
        for m in fmodes:
            fixed_all(r, cam, min(F, max(2, m)), m)
        fruns = {m: [] for m in fmodes}
        for _ in range(a.reps):
            for m in fmodes:
                fruns[m].append(fixed_all(r, cam, F, m))
        for m in fmodes:
            out["fixed"]["per-frame" if m == 0 else str(m)] = {"wall_ms_per_frame": [x["wall_ms"] / F for x in fruns[m]],
                                                              "kernel_ms_per_frame_median": statistics.median(x["kernel_ms"] / F for x in fruns[m])}
        print(json.dumps(out), flush=True)
    finally:
        r.close()


if __name__ == "__main__":
    main()
