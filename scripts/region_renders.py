"""Measurements for region renders (profiles/experiments/region_renders.txt).  One JSON line per run on stdout.
  python scripts/region_renders.py frames [--reps 3]
      the kernels that carry the region's offsets, on whole frames: the teapot orbit movie (keyed camera, CAMK kernels,
      f64, relaxed) at scripts/ab_frames.py's small shape with 1 and 48 frames per launch, and one 1920x1080 @ 512 frame;
      kernel ms of every repeat and one md5 over all frames.  Run it once per build in alternation (a copy of this script in a
      checkout of the other commit, e.g. the parent's: its Python table must match its library): equal md5s, and a difference inside the spread of one library's
      own repeats, is "no loss".
  python scripts/region_renders.py guides [--reps 5]
      the f32 guide kernels of cr_render_aov_frames_* that walk on screening records, one per residency and kind: the
      teapot orbit (camera keys only) with the tree's top in LDS and in global memory, book1 with a keyed ground sphere
      (keyed primitives) in LDS, with its top in LDS and in global memory; 8 frames of 400x225 @ 50 spp per call, kernel
      ms per repeat and one md5 per configuration.  Run once per library in alternation, as `frames`.
  python scripts/region_renders.py cost [--reps 3]
      what a region costs: book1 1920x1080 @ 512 spp, f64, relaxed -- the whole frame (static kernel), the whole frame as
      one region (CAMK kernel), one 480x270 region, and the 16 such regions that tile the frame."""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene, procedural_sky  # noqa: E402
from crucible_amd.renderer import LIB_PATH, Renderer  # noqa: E402
from ab_frames import render_all, shape  # noqa: E402

SEED = 0xC0FFEE
KW = dict(seed=SEED, real_type=A.CR_REAL_F64, sum_order=A.CR_SUM_RELAXED)


def frames(r, reps):
    sky = procedural_sky()
    md5 = hashlib.md5()
    out = {"lib": LIB_PATH, "small_kernel_ms_per_frame": {}, "large_kernel_ms": []}
    sc = shape("small", sky)
    r.upload_scene(sc.flatten())
    render_all(r, sc, 2, 1)   # warm-up
    for fpl in (1, 48):
        runs = []
        for _ in range(reps):
            _, kms, hashes = render_all(r, sc, 48, fpl)
            runs.append(kms / 48)
        md5.update("".join(hashes).encode())
        out["small_kernel_ms_per_frame"][str(fpl)] = runs
    sc = shape("large", sky)
    r.upload_scene(sc.flatten())
    for k in range(reps + 1):
        img, st = r.render(sc.scene_cam, **KW)
        if k:
            out["large_kernel_ms"].append(st["kernel_ms"])
    md5.update(img.tobytes())
    out["md5"] = md5.hexdigest()
    return out


def guides(reps):
    from crucible_amd.scene import LERP, LOCAL
    out = {"lib": LIB_PATH, "configs": {}}
    sky = procedural_sky()
    for name, keyed, env in (("top-camera", False, {}), ("global-camera", False, {"CRUCIBLE_LDS_TOP_KB": "0"}),
                             ("lds-keyed", True, {}), ("top-keyed", True, {"CRUCIBLE_LDS_LIMIT": "0"}),
                             ("global-keyed", True, {"CRUCIBLE_LDS_LIMIT": "0", "CRUCIBLE_LDS_TOP_KB": "0"})):
        if keyed:
            sc = book1_end_scene(1, scene_seed=1, image_width=400, samples=50)
            sc.translate_point((0.0, 0.01, 0.0), 1.0, LERP, LOCAL, "ground")
        else:
            sc = shape("small", sky)
        os.environ.update(env)
        r = Renderer(0)
        for k in env:
            del os.environ[k]
        try:
            r.upload_scene(sc.flatten())
            runs, md5 = [], hashlib.md5()
            for k in range(reps + 1):
                planes, st = r.render_aov_frames(sc.scene_cam, list(range(8)), seed=SEED, real_type=A.CR_REAL_F32)
                if k:
                    runs.append(st["kernel_ms"])
            for fr in planes:
                for n in sorted(fr):
                    md5.update(fr[n].tobytes())
            out["configs"][name] = {"scene_in_lds": st["scene_in_lds"], "kernel_ms": runs, "md5": md5.hexdigest()}
        finally:
            r.close()
    return out


def cost(r, reps):
    sc = book1_end_scene(1, scene_seed=1, image_width=1920, samples=512)
    cam = sc.scene_cam
    W, H = cam.image_width, cam.image_height
    r.upload_scene(sc.flatten())
    buf = torch.empty((H, W, 3), dtype=torch.float64, device="cuda:0")
    part = torch.empty((H // 4, W // 4, 3), dtype=torch.float64, device="cuda:0")
    tiles = [(x0, y0, W // 4, H // 4) for y0 in range(0, H, H // 4) for x0 in range(0, W, W // 4)]
    r.render_device(cam, buf.data_ptr(), want_stats=True, **KW)   # warm-up: tree build, first launch
    r.render_region_device(cam, tiles[0], part.data_ptr(), want_stats=True, **KW)
    full, whole, one, sixteen = [], [], [], []
    for _ in range(reps):   # alternated
        full.append(r.render_device(cam, buf.data_ptr(), want_stats=True, **KW)["kernel_ms"])
        whole.append(r.render_region_device(cam, (0, 0, W, H), buf.data_ptr(), want_stats=True, **KW)["kernel_ms"])
        per = [r.render_region_device(cam, t, part.data_ptr(), want_stats=True, **KW)["kernel_ms"] for t in tiles]
        one.append(per[5])   # an inner tile
        sixteen.append(sum(per))
    med = statistics.median
    return {"lib": LIB_PATH, "frame": f"book1 {W}x{H} @ {cam.samples} spp, f64, relaxed", "region": f"{W // 4}x{H // 4}",
            "full_frame_kernel_ms": full, "whole_frame_as_region_kernel_ms": whole, "one_region_kernel_ms": one,
            "sixteen_regions_kernel_ms": sixteen, "last_per_region_kernel_ms": per,
            "one_region_over_a_sixteenth": med(one) / (med(full) / 16), "sixteen_over_full": med(sixteen) / med(full)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["frames", "guides", "cost"])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.what == "guides":
        print(json.dumps(guides(a.reps)), flush=True)
        return
    r = Renderer(0)
    try:
        print(json.dumps((frames if a.what == "frames" else cost)(r, a.reps)), flush=True)
    finally:
        r.close()


if __name__ == "__main__":
    main()
