"""What an adaptive region costs against its alternatives (profiles/experiments/adaptive_region.txt).  One
JSON line on stdout.
  python scripts/ab_adaptive_region.py [--width 1920] [--spp 512] [--pass-samples 16] [--min-samples 64] [--block 16]
                                       [--tolerance 0.01] [--patch 256] [--grid 4] [--reps 5] [--real f64]
book1 at the given size, everything in one process on one handle, every mode warmed once and then alternated `reps` times:
  patch      cr_render_adaptive_region_host of one aligned patch x patch region near the frame's centre (the editor's re-render)
  fixed      cr_render_region_host of the same pixels at the full sample count
  whole      cr_render_adaptive_host of the whole frame
  tiled      the whole frame as grid x grid aligned regions through Renderer.render_tiled(adaptive=...)
Wall ms of every repeat, the calls' kernel and judge ms, passes, blocks, samples; and whether the patch and the tiled frame
are the whole-frame call's pixels and counts, as the alignment promises."""
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
    ap.add_argument("--tolerance", type=float, default=0.01)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--real", choices=["f32", "f64"], default="f64")
    a = ap.parse_args()
    rt = A.CR_REAL_F64 if a.real == "f64" else A.CR_REAL_F32
    sc = book1_end_scene(1, scene_seed=1, image_width=a.width, samples=a.spp)
    cam = sc.scene_cam
    W, H = cam.image_width, cam.image_height
    kw = dict(seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
    akw = dict(tolerance=a.tolerance, min_samples=a.min_samples, pass_samples=a.pass_samples, block=a.block)
    if a.patch % a.block or a.patch > min(W, H):
        sys.exit("--patch must be a multiple of --block and fit the frame")
    # the patch: aligned, near the centre; the tiles: the smallest multiple of the block that covers the frame in `grid` steps
    patch = ((W - a.patch) // 2 // a.block * a.block, (H - a.patch) // 2 // a.block * a.block, a.patch, a.patch)
    tile = tuple(-(-(-(-n // a.grid)) // a.block) * a.block for n in (W, H))
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        r.render(cam, **kw)   # warm-up: tree build, first launch

        def timed(fn):
            t0 = time.perf_counter()
            res = fn()
            return (time.perf_counter() - t0) * 1e3, res

        modes = {
            "patch": lambda: r.render_adaptive_region(cam, patch, **akw, **kw),
            "fixed": lambda: r.render_region(cam, patch, **kw),
            "whole": lambda: r.render_adaptive(cam, **akw, **kw),
            "tiled": lambda: r.render_tiled(cam, tile, adaptive=akw, **kw),
        }
        for fn in modes.values():
            fn()
        runs = {name: [] for name in modes}
        last = {}
        for _ in range(a.reps):
            for name, fn in modes.items():
                ms, last[name] = timed(fn)
                st = last[name][-1]
                rs = st["render"] if "render" in st else st
                runs[name].append({"wall_ms": ms, "kernel_ms": rs["kernel_ms"], "judge_ms": st.get("judge_ms", 0.0)})
        x0, y0, w, h = patch
        whole_img, whole_counts, whole_st = last["whole"]
        out = {"lib": LIB_PATH, "frame": f"book1 {W}x{H} @ {a.spp} spp max, {a.real}, relaxed", **akw, "patch": patch, "tile": tile,
               "tiles": -(-W // tile[0]) * -(-H // tile[1]), "reps": a.reps, "runs": runs}
        for name in ("patch", "whole", "tiled"):
            st = last[name][-1]
            out[name] = {"passes": st["passes"], "blocks": st["blocks"], "blocks_stopped": st["blocks_stopped"],
                         "samples_taken": st["render"]["samples"]}
        out["fixed"] = {"samples_taken": last["fixed"][1]["samples"]}
        out["patch_equals_whole"] = bool(np.array_equal(last["patch"][0], whole_img[y0:y0 + h, x0:x0 + w]) and
                                         np.array_equal(last["patch"][1], whole_counts[y0:y0 + h, x0:x0 + w]))
        out["tiled_equals_whole"] = bool(np.array_equal(last["tiled"][0], whole_img) and np.array_equal(last["tiled"][1], whole_counts))
        out["tiled_counters_equal_whole"] = all(last["tiled"][2]["render"][k] == whole_st["render"][k]
                                                for k in ("samples", "segments", "node_tests", "prim_tests", "texel_fetches"))
        out["median_wall_ms"] = {name: float(np.median([x["wall_ms"] for x in v])) for name, v in runs.items()}
        out["range_wall_ms"] = {name: [min(x["wall_ms"] for x in v), max(x["wall_ms"] for x in v)] for name, v in runs.items()}
        print(json.dumps(out), flush=True)
    finally:
        r.close()


if __name__ == "__main__":
    main()
