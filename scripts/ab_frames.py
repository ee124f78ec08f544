"""A/B of cr_render_frames_host against one frame per call: the teapot orbit movie's camera (keyed camera, the CAMK
kernels), f64, relaxed sums, the frames 0 .. F-1 rendered with frames_per_launch 1, 8 and F, alternated, `--reps` times
each.  Per mode: wall time per frame (the host call, copy back included, as render_movie makes it) and the summed
kernel_ms.  Every frame of every mode must hash to the one-frame-per-call frame.
  small: first_movie's shape (demo_movies.rs:13-16): 400x225 @ 50 spp, depth 5, F = --frames (>= 48)
  large: BASELINE configs[4]'s frame, 1920x1080 @ 512 spp, its own depth, F = --large-frames (1 and F per launch)
usage: python scripts/ab_frames.py [--out profiles/experiments/frames_per_launch.json] [--frames 48] [--reps 5]
       python scripts/ab_frames.py --trace-one-launch N   (under rocprofv3 --kernel-trace --stats: the small shape's
                                                           F frames at N frames per launch, nothing else)
       python scripts/ab_frames.py --count-dispatches KERNEL_STATS_CSV   (pathtrace_kernel dispatches in a rocprofv3 run)"""
import argparse
import csv
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
from crucible_amd.renderer import Renderer  # noqa: E402

SEED = 0xC0FFEE


def shape(name, sky):
    if name == "small":
        sc = teapot_orbit_movie(1, image_width=400, samples=50, sky=sky)
        sc.scene_cam.set_max_depth(5)
    else:
        sc = teapot_orbit_movie(1, image_width=1920, samples=512, sky=sky)
    return sc


def render_all(r, sc, n_frames, fpl):
    """Frames 0 .. n_frames-1 at fpl frames per call: (wall s, kernel ms, per-frame md5s).  The frames are hashed after
    the clock stops."""
    cam, kept, kernel_ms = sc.scene_cam, [], 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f0 in range(0, n_frames, fpl):
        frames = list(range(f0, min(n_frames, f0 + fpl)))
        if fpl == 1:
            cam.frame = f0
            img, st = r.render(cam, seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)
            imgs = img[None]
        else:
            imgs, st = r.render_frames(cam, frames, seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)
        kernel_ms += st["kernel_ms"]
        kept.append(imgs)
    wall = time.perf_counter() - t0
    return wall, kernel_ms, [hashlib.md5(im.tobytes()).hexdigest() for imgs in kept for im in imgs]


def ab(r, sky, name, n_frames, modes, reps):
    sc = shape(name, sky)
    r.upload_scene(sc.flatten())
    cam = sc.scene_cam
    samples = cam.image_width * cam.image_height * cam.samples * n_frames
    render_all(r, sc, min(n_frames, 2), 1)   # warm-up: scene build, first launches
    runs = {m: [] for m in modes}
    ref = None
    for rep in range(reps):
        for m in modes:   # alternated
            wall, kms, hashes = render_all(r, sc, n_frames, m)
            if ref is None:
                ref = hashes
            runs[m].append({"wall_s": wall, "kernel_ms": kms, "images_equal": hashes == ref})
            print(f"{name} rep {rep} fpl {m:3d}: {wall / n_frames * 1e3:8.3f} ms/frame wall, {kms / n_frames:8.3f} ms/frame kernel, "
                  f"{samples / (kms * 1e3):7.0f} Msamples/s kernel, equal {hashes == ref}", flush=True)
    out = {"shape": f"teapot orbit movie {cam.image_width}x{cam.image_height} @ {cam.samples} spp, depth {cam.max_depth}, "
                    f"{n_frames} frames, f64, relaxed", "frames": n_frames, "modes": {}}
    for m in modes:
        walls = [x["wall_s"] for x in runs[m]]
        kms = [x["kernel_ms"] for x in runs[m]]
        out["modes"][str(m)] = {"runs": runs[m], "wall_ms_per_frame_median": statistics.median(walls) / n_frames * 1e3,
                                "wall_ms_per_frame_min": min(walls) / n_frames * 1e3,
                                "kernel_ms_per_frame_median": statistics.median(kms) / n_frames,
                                "msamples_per_s_kernel_median": samples / (statistics.median(kms) * 1e3),
                                "images_equal": all(x["images_equal"] for x in runs[m])}
    base = out["modes"][str(modes[0])]
    for m in modes[1:]:
        o = out["modes"][str(m)]
        o["wall_speedup_vs_1"] = base["wall_ms_per_frame_median"] / o["wall_ms_per_frame_median"]
        o["kernel_speedup_vs_1"] = base["kernel_ms_per_frame_median"] / o["kernel_ms_per_frame_median"]
    return out


def count_dispatches(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    return sum(int(r["Calls"]) for r in rows if "pathtrace_kernel" in r["Name"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "experiments", "frames_per_launch.json"))
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--large-frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-one-launch", type=int, default=0)
    ap.add_argument("--count-dispatches", default="")
    a = ap.parse_args()
    if a.count_dispatches:
        print(count_dispatches(a.count_dispatches))
        return
    sky = procedural_sky()
    r = Renderer(0)
    try:
        if a.trace_one_launch:
            sc = shape("small", sky)
            r.upload_scene(sc.flatten())
            render_all(r, sc, a.frames, a.trace_one_launch)
            return
        rec = {"tool": "scripts/ab_frames.py", "device": torch.cuda.get_device_name(0),
               "small": ab(r, sky, "small", a.frames, [1, 8, a.frames], a.reps),
               "large": ab(r, sky, "large", a.large_frames, [1, a.large_frames], 2)}
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
