"""The guide layers of a movie's frames, one cr_render_aov_device call per frame against cr_render_aov_frames_device at 8
frames per launch and at all frames in one launch: all four layers, f32 and f64, HIP events (CrStats.kernel_ms, summed over
the calls) and wall clock (the calls queued without stats, then one synchronize), best of `--reps` after a warm-up.
  movie:  first_movie's shape, 400x225 @ 50 spp, the teapot orbit camera of scripts/ab_frames.py, --frames frames (48)
  large:  the same movie at 1920x1080 @ 64 spp, 8 frames: 8 single calls against one launch
  single: cr_render_aov_device alone on book1 1920x1080 @ 64 spp and on the 400x225 @ 50 spp book1 frame (the cases of
          scripts/aov_pass.py), to compare two builds
One JSON line per case.  With --loop-only nothing of the batch interface is touched: point CRUCIBLE_HIP_LIB at the
library of a build from before it for the yardstick, and alternate the two builds in one session.
usage: python scripts/aov_frames.py [--loop-only] [--frames 48] [--reps 5] [--tag NAME]"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)

from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene, procedural_sky, teapot_orbit_movie  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

SEED = 0xC0FFEE
REALS = ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64"))


def run(r, cam, buf, rt, frames, fpl, stats):
    """The frames at fpl per call into buf, frame after frame: (wall s, summed kernel ms or None)"""
    stride = cam.image_width * cam.image_height * 8
    kernel_ms = 0.0
    r.synchronize()
    t0 = time.perf_counter()
    for f0 in range(0, len(frames), fpl):
        ptr = buf.data_ptr() + f0 * stride * buf.element_size()
        if fpl == 1:
            cam.frame = frames[f0]
            st = r.render_aov_device(cam, ptr, seed=SEED, real_type=rt, want_stats=stats)
        else:
            st = r.render_aov_frames_device(cam, frames[f0:f0 + fpl], ptr, seed=SEED, real_type=rt, want_stats=stats)
        if stats:
            kernel_ms += st["kernel_ms"]
    r.synchronize()
    return time.perf_counter() - t0, kernel_ms if stats else None


def movie_case(r, sc, name, n_frames, modes, reps, tag):
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    frames = list(range(n_frames))
    n = cam.image_width * cam.image_height * 8
    for rt, real in REALS:
        buf = torch.empty(n * n_frames, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
        ref = None
        for fpl in modes:
            run(r, cam, buf, rt, frames, fpl, True)   # warm-up: tree, code objects, the handle's buffers
            walls, kernels = [], []
            for _ in range(reps):
                walls.append(run(r, cam, buf, rt, frames, fpl, False)[0])
                kernels.append(run(r, cam, buf, rt, frames, fpl, True)[1])
            digest = hashlib.md5(buf.cpu().numpy().tobytes()).hexdigest()
            ref = ref or digest
            print(json.dumps({"build": tag, "case": name, "real": real, "width": cam.image_width, "height": cam.image_height,
                              "samples": cam.samples, "frames": n_frames, "frames_per_launch": fpl,
                              "kernel_ms_per_frame_min": min(kernels) / n_frames, "kernel_ms_per_frame_max": max(kernels) / n_frames,
                              "wall_ms_per_frame_min": min(walls) / n_frames * 1e3, "wall_ms_per_frame_max": max(walls) / n_frames * 1e3,
                              "equal_to_first_mode": digest == ref, "md5": digest}), flush=True)


def single_cases(r, reps, tag):
    for name, width, samples in (("book1_1080p_64spp", 1920, 64), ("movie_frame_400x225_50spp", 400, 50)):
        sc = book1_end_scene(1, scene_seed=1, image_width=width, samples=samples)
        cam = sc.scene_cam
        r.upload_scene(sc.flatten())
        n = cam.image_width * cam.image_height * 8
        for rt, real in REALS:
            buf = torch.empty(n, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
            ms = [r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True)["kernel_ms"] for _ in range(reps + 1)][1:]
            print(json.dumps({"build": tag, "case": "single " + name, "real": real, "width": cam.image_width, "height": cam.image_height,
                              "samples": samples, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.loop_only:   # a build from before the batch interface does not export its calls
        for name in ("cr_render_aov_frames_device", "cr_render_aov_frames_host"):
            A.SYMBOLS.pop(name, None)
    tag = a.tag or ("loop-only" if a.loop_only else "this")
    sky = procedural_sky()
    r = Renderer(0)
    try:
        single_cases(r, a.reps, tag)
        small = teapot_orbit_movie(1, image_width=400, samples=50, sky=sky)
        movie_case(r, small, "movie", a.frames, [1] if a.loop_only else [1, 8, a.frames], a.reps, tag)
        large = teapot_orbit_movie(1, image_width=1920, samples=64, sky=sky)
        movie_case(r, large, "large", 8, [1] if a.loop_only else [1, 8], a.reps, tag)
    finally:
        r.close()


if __name__ == "__main__":
    main()
