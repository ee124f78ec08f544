"""A/B of cr_render_views_device against one cr_render_device per view, f64, relaxed sums, the teapot scene with its image sky:
  orbit: first_movie's shape (demo_movies.rs:13-16) 400x225 @ 50 spp, depth 5 -- 48 views of a zooming orbit: static
         cameras on a circle around the teapot, vfov 20 .. 30 degrees (a path and a zoom sampled on the host)
  cube:  the six faces of a cube map, 512x512 @ 50 spp, depth 5, vfov 90 degrees from a point beside the teapot
Modes, `--reps` times each, one JSON line per shape and mode:
  views         all views in one cr_render_views_device call with stats: wall and the call's kernel_ms
  single        one cr_render_device call with stats per view: wall and the summed kernel_ms (each call synchronises)
  single-async  one cr_render_device call without stats per view, one synchronise at the end: wall only
The single modes use nothing that the parent of the views calls lacks, so the same script measures a build without them:
  python scripts/ab_views.py --modes single,single-async     (in that build's tree)
  python scripts/ab_views.py --modes views,single,single-async
Every mode hashes its views after the clock stops; the hashes of all modes (and of both builds) must agree.
Results: profiles/experiments/views_per_launch.txt."""
import argparse
import copy
import hashlib
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import load_teapot, procedural_sky  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

SEED = 0xC0FFEE
KW = dict(seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)


def orbit(sky, n=48):
    sc = load_teapot(1, image_width=400, samples=50, sky=sky)
    cam = sc.scene_cam
    cam.set_max_depth(5)
    cams = []
    for k in range(n):
        c = copy.deepcopy(cam)
        a = 2.0 * math.pi * k / n
        c.look_from((13.0 * math.sin(a), 10.0, -13.0 * math.cos(a)))
        c.set_vfov(20.0 + 10.0 * k / (n - 1))
        cams.append(c)
    return sc, cams


def cube(sky):
    sc = load_teapot(1, image_width=512, samples=50, sky=sky)
    cam = sc.scene_cam
    cam.set_max_depth(5)
    cam.aspect_ratio, cam.image_height = 1.0, 512
    cam.set_vfov(90.0)
    eye = (4.0, 3.0, 4.0)
    cams = []
    for d, up in (((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))):
        c = copy.deepcopy(cam)
        c.look_from(eye)
        c.look_at(tuple(e + x for e, x in zip(eye, d)))
        c.set_vup(up)
        cams.append(c)
    return sc, cams


def run(r, cams, mode, out):
    """One pass over the views: (wall s, kernel ms or None)."""
    n = len(cams)
    view = out[0].numel() * out.element_size()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if mode == "views":
        kms = r.render_views_device(cams, out.data_ptr(), None, want_stats=True, **KW)["kernel_ms"]
    elif mode == "single":
        kms = sum(r.render_device(cams[k], out.data_ptr() + k * view, want_stats=True, **KW)["kernel_ms"] for k in range(n))
    else:
        for k in range(n):
            r.render_device(cams[k], out.data_ptr() + k * view, **KW)
        r.synchronize()
        kms = None
    return time.perf_counter() - t0, kms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="views,single,single-async")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="orbit,cube")
    a = ap.parse_args()
    sky = procedural_sky()
    r = Renderer(0)
    try:
        for shape in a.shapes.split(","):
            sc, cams = orbit(sky) if shape == "orbit" else cube(sky)
            r.upload_scene(sc.flatten())
            cam = cams[0]
            out = torch.zeros((len(cams), cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda:0")
            run(r, cams[:2], "single", out)   # warm-up: scene build, first launches
            modes = a.modes.split(",")
            runs = {m: [] for m in modes}
            hashes = {}
            for rep in range(a.reps):
                for m in modes:   # alternated
                    out.zero_()
                    runs[m].append(run(r, cams, m, out))
                    hashes[m] = hashlib.md5(out.cpu().numpy().tobytes()).hexdigest()
            for m in modes:
                walls = [w for w, _ in runs[m]]
                kms = [k for _, k in runs[m] if k is not None]
                print(json.dumps({"shape": shape, "mode": m, "views": len(cams), "size": f"{cam.image_width}x{cam.image_height}", "spp": cam.samples,
                                  "device": torch.cuda.get_device_name(0), "reps": a.reps,
                                  "wall_ms_per_view_median": statistics.median(walls) / len(cams) * 1e3, "wall_ms_per_view_min": min(walls) / len(cams) * 1e3,
                                  "kernel_ms_per_view_median": statistics.median(kms) / len(cams) if kms else None, "md5": hashes[m]}), flush=True)
    finally:
        r.close()


if __name__ == "__main__":
    main()
