"""What adaptive sampling saves (profiles/experiments/adaptive_sampling.txt).  One JSON line on stdout.
  python scripts/ab_adaptive.py [--width 1920] [--spp 512] [--pass-samples 16] [--min-samples 64] [--block 16]
                                [--tolerances 0.02,0.01,0.005] [--reps 2] [--real f64]
book1 at the given size: the fixed-count relaxed render (cr_render_host; wall and kernel ms of every repeat), then
cr_render_adaptive_host per tolerance -- wall ms, kernel ms (the passes'), judge ms, passes, blocks stopped, total samples
taken, and the largest and the mean absolute difference from the fixed-count frame (linear colour).  Everything in one
process on one handle, the fixed render repeated after the adaptive ones, so the figures share a session."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene  # noqa: E402
from crucible_amd.renderer import LIB_PATH, Renderer  # noqa: E402

SEED = 0xC0FFEE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--pass-samples", type=int, default=16)
    ap.add_argument("--min-samples", type=int, default=64)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--tolerances", default="0.02,0.01,0.005")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--real", choices=["f32", "f64"], default="f64")
    a = ap.parse_args()
    rt = A.CR_REAL_F64 if a.real == "f64" else A.CR_REAL_F32
    sc = book1_end_scene(1, scene_seed=1, image_width=a.width, samples=a.spp)
    cam = sc.scene_cam
    kw = dict(seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        r.render(cam, **kw)   # warm-up: tree build, first launch

        def fixed():
            t0 = time.perf_counter()
            img, st = r.render(cam, **kw)
            return img, {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["kernel_ms"]}

        ref, first = fixed()
        out = {"lib": LIB_PATH, "frame": f"book1 {cam.image_width}x{cam.image_height} @ {a.spp} spp, {a.real}, relaxed",
               "pass_samples": a.pass_samples, "min_samples": a.min_samples, "block": a.block, "fixed": [first], "adaptive": []}
        ref64 = ref.astype(np.float64)
        for tol in (float(t) for t in a.tolerances.split(",")):
            runs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                img, counts, st = r.render_adaptive(cam, tolerance=tol, min_samples=a.min_samples, pass_samples=a.pass_samples,
                                                    block=a.block, **kw)
                runs.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["render"]["kernel_ms"], "judge_ms": st["judge_ms"]})
            diff = np.abs(img.astype(np.float64) - ref64)
            out["adaptive"].append({"tolerance": tol, "runs": runs, "passes": st["passes"], "blocks": st["blocks"],
                                    "blocks_stopped": st["blocks_stopped"], "samples_taken": st["render"]["samples"],
                                    "samples_fixed": cam.image_width * cam.image_height * a.spp,
                                    "mean_count": float(counts.mean()), "max_abs_diff": float(diff.max()), "mean_abs_diff": float(diff.mean())})
            out["fixed"].append(fixed()[1])
        print(json.dumps(out), flush=True)
    finally:
        r.close()


if __name__ == "__main__":
    main()
