"""Kernel time of the guide pass (cr_render_aov_device, all four layers) beside its yardstick, cr_render_device at
max_depth = 1 under CR_SUM_RELAXED: the same primary rays, walked by the megakernel.  Kernel events (CrStats.kernel_ms),
best of 5 after a warm-up, on book1 1920x1080 @ 64 spp and the 400x225 @ 50 spp movie frame, f32 and f64.  One JSON line
per case.  With CRUCIBLE_HIP_LIB set to another build's library the `render_ms` column is that build's yardstick.
usage: python scripts/aov_pass.py [--only-render]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

only_render = "--only-render" in sys.argv
if only_render:   # a build from before the guide pass does not export its calls
    for name in ("cr_render_aov_device", "cr_render_aov_host", "cr_write_pfm"):
        A.SYMBOLS.pop(name, None)
r = Renderer(0)
for name, width, samples in (("book1_1080p_64spp", 1920, 64), ("movie_frame_400x225_50spp", 400, 50)):
    sc = book1_end_scene(1, scene_seed=1, image_width=width, samples=samples)
    cam = sc.scene_cam
    r.upload_scene(sc.flatten())
    n = cam.image_width * cam.image_height
    for rt, tag in ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64")):
        buf = torch.empty(n * 8, dtype=torch.float64 if rt == A.CR_REAL_F64 else torch.float32, device="cuda:0")
        depth = cam.max_depth
        cam.set_max_depth(1)
        ms_r = [r.render_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True, sum_order=A.CR_SUM_RELAXED)["kernel_ms"] for _ in range(6)][1:]
        cam.set_max_depth(depth)
        row = {"case": name, "real": tag, "width": cam.image_width, "height": cam.image_height, "samples": samples, "render_depth1_ms": min(ms_r)}
        if not only_render:
            st = [r.render_aov_device(cam, buf.data_ptr(), seed=1, real_type=rt, want_stats=True) for _ in range(6)][1:]
            row["aov_ms"] = min(s["kernel_ms"] for s in st)
            row["ratio"] = row["aov_ms"] / row["render_depth1_ms"]
            row["scene_in_lds"] = st[0]["scene_in_lds"]
        print(json.dumps(row), flush=True)
r.close()
