"""Kernel time of the guide pass at a count plane (cr_render_aov_counts_device, all four layers) over the counts of an
adaptive frame, beside two yardsticks taken from ANOTHER build's library: (a) cr_render_aov_device at the maximum sample
count -- the only guide pass there was, which casts other primary rays than the adaptive pixels used -- and (b) the same
call at samples = ceil(mean count), a lower mark.  Kernel events (CrStats.kernel_ms), best of 5 after a warm-up, f32 and
f64; every row also carries the five repetitions' spread (max - min).  Cases: book1 1920x1080 with a maximum of 512 at
tolerance 0.02 and 0.01 (passes of 16, blocks of 16), the 400x225 movie frame with a maximum of 64, the scaled teapot at
400x225 with a maximum of 64 (keyed primitives: the ANIM kernels, the tree's top window in LDS), and the overhead
check: a plane that is 64 everywhere against the plain pass at 64 spp.  One JSON line per row.

usage: CRUCIBLE_HIP_LIB=<the parent build's library> python scripts/aov_counts.py --yardstick     rows (a), (b), plain
       python scripts/aov_counts.py                                                                the counts pass
The counts are those of cr_render_adaptive_host, which both builds have and compute bit for bit alike; the yardstick run
binds no cr_render_aov_counts_* symbol.  units_at_16_waves_per_cu / empty_units_at_16_waves_per_cu restate aov_launch's
sizing on the host under the assumption its name states (one 1024-thread workgroup per CU, in both precisions; what
pick_block chose is not visible through the ABI): the units whose first sample group lies beyond their tile's largest
count.  A host restatement, not a device counter."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene, scaled_teapot  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

yardstick = "--yardstick" in sys.argv
if yardstick:   # the parent's library does not export the calls under test
    for name in [n for n in A.SYMBOLS if n.startswith("cr_render_aov_counts_")]:
        A.SYMBOLS.pop(name)
CASES = (("book1_1080p_max512_tol0.02", 1920, 512, 0.02), ("book1_1080p_max512_tol0.01", 1920, 512, 0.01), ("movie_frame_400x225_max64_tol0.02", 400, 64, 0.02),
         ("scaled_teapot_400x225_max64_tol0.02", 400, 64, 0.02))


def best_of_5(call):
    ms = [call()["kernel_ms"] for _ in range(6)][1:]
    return {"ms": min(ms), "spread_ms": max(ms) - min(ms)}


def empty_units(counts, samples, n_cus):
    """(units of the launch, those with nothing to do) by aov_launch's rule: tiles of 4 x 4 pixels, groups of 4 samples"""
    h, w = counts.shape
    th, tw = -(-h // 4), -(-w // 4)
    pad = np.zeros((th * 4, tw * 4), dtype=np.int64)
    pad[:h, :w] = np.clip(counts, 0, samples)
    tile_max = pad.reshape(th, 4, tw, 4).max(axis=(1, 3)).reshape(-1)
    groups, tiles, resident = (samples + 3) // 4, th * tw, n_cus * 16
    ug = min(groups, max(1, tiles * groups // (8 * resident)))
    chunks = -(-groups // ug)
    need = (tile_max + 3) // 4                                   # groups a tile still runs
    ran = np.minimum(chunks, -(-need // ug))                     # its units with a first group below that
    return int(tiles * chunks), int((chunks - ran).sum())


r = Renderer(0)
n_cus = torch.cuda.get_device_properties(0).multi_processor_count
for name, width, samples, tol in CASES:
    teapot = name.startswith("scaled_teapot")
    sc = scaled_teapot(1, image_width=width, samples=samples) if teapot else book1_end_scene(1, scene_seed=1, image_width=width, samples=samples)
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    n = cam.image_width * cam.image_height
    for rt, tag in ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64")):
        _, counts, ast = r.render_adaptive(cam, seed=1, real_type=rt, tolerance=tol, min_samples=64 if samples > 64 else 32, pass_samples=16, block=16,
                                           sum_order=A.CR_SUM_RELAXED)
        total, mean = int(counts.sum(dtype=np.int64)), float(counts.mean())
        buf = torch.empty(n * 8, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
        row = {"case": name, "real": tag, "width": cam.image_width, "height": cam.image_height, "max_samples": samples, "tolerance": tol,
               "sum_counts": total, "mean_count": mean, "distinct_counts": [int(v) for v in np.unique(counts)]}
        if yardstick:
            row["a_plain_at_max"] = best_of_5(lambda: r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
            cam.set_samples(int(math.ceil(mean)))
            row["b_plain_at_ceil_mean"] = dict(best_of_5(lambda: r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True)), samples=cam.samples)
            cam.set_samples(samples)
        else:
            d_counts = torch.from_numpy(counts).to("cuda:0")
            row["counts_pass"] = best_of_5(lambda: r.render_aov_counts_device(cam, d_counts.data_ptr(), buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
            row["units_at_16_waves_per_cu"], row["empty_units_at_16_waves_per_cu"] = empty_units(counts, samples, n_cus)
            row["scene_in_lds"] = r.render_aov_counts_device(cam, d_counts.data_ptr(), buf.data_ptr(), seed=1, real_type=rt, want_stats=True)["scene_in_lds"]
            if teapot:   # the ANIM kernels' own overhead: the maximum everywhere against (a)
                d_full = torch.full((n,), samples, dtype=torch.int32, device="cuda:0")
                row["counts_pass_uniform_max"] = best_of_5(lambda: r.render_aov_counts_device(cam, d_full.data_ptr(), buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
        print(json.dumps(row), flush=True)
# the overhead of the count plane where it saves nothing: 64 everywhere against the plain pass at 64 spp
sc = book1_end_scene(1, scene_seed=1, image_width=1920, samples=64)
cam = sc.scene_cam
r.upload_scene(sc.flatten())
n = cam.image_width * cam.image_height
for rt, tag in ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64")):
    buf = torch.empty(n * 8, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    row = {"case": "book1_1080p_uniform_64", "real": tag}
    if yardstick:
        row["plain_64spp"] = best_of_5(lambda: r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
    else:
        d_counts = torch.full((n,), 64, dtype=torch.int32, device="cuda:0")
        row["counts_pass_uniform_64"] = best_of_5(lambda: r.render_aov_counts_device(cam, d_counts.data_ptr(), buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
        row["plain_64spp_this_build"] = best_of_5(lambda: r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True))
    print(json.dumps(row), flush=True)
r.close()
