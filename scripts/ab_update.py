"""What cr_update_primitives costs and what it leaves behind, against the only way there was before it: another
cr_upload_scene.  Scenes: book1 and the 1M-sphere field, in f64 and f32, reference topology (the headline's).
  (a) re-upload: cr_upload_scene + the first render's build, the handle's own `upload_ms` (what every edit cost so far);
  (b) CR_UPDATE_REFIT of every small sphere and of 1 % of them: wall time around the call + cr_synchronize, best of 5
      after a warm-up call;
  (c) tree drift: Msamples/s (kernel time) of a headline-shaped render -- 1920 wide, `--spp` samples -- after the same
      edit applied with REFIT (the old topology, refitted boxes) and with REBUILD (a fresh tree), for small and large
      displacements; the REBUILD's own cost (upload_ms of the render that rebuilds) goes with it.
Every ratio is against (a) or REBUILD measured in the same run.  The REFIT and REBUILD frames are compared pixel by pixel
(box-grazing rays may differ, nothing else).
usage: python scripts/ab_update.py [--out profiles/experiments/update_primitives.txt] [--scenes book1,million] [--spp 64]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene, million_spheres  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

SEED = 0xC0FFEE
PRIM = np.dtype([("kind", "<i4"), ("material", "<i4"), ("flags", "<i4"), ("key_first", "<i4"), ("key_count", "<i4"),
                 ("_pad", "<i4"), ("v", "<f8", 9)])


def prim_view(flat):
    return np.frombuffer(flat.prims, dtype=PRIM, count=flat.desc.n_prims)


def small_spheres(flat):
    p = prim_view(flat)
    return np.nonzero((p["kind"] == A.CR_PRIM_SPHERE) & (p["v"][:, 3] < 0.5))[0].astype(np.int32)


def moved_rows(flat, idx, reach, seed):
    """The spheres `idx` pushed by up to `reach` along x and z (they stay on the ground)."""
    rs = np.random.RandomState(seed)
    rows = prim_view(flat)["v"][idx].copy()
    rows[:, 0] += rs.uniform(-reach, reach, len(idx))
    rows[:, 2] += rs.uniform(-reach, reach, len(idx))
    return rows


def timed_update(r, idx, rows, rebuild=False):
    r.synchronize()
    t0 = time.perf_counter()
    r.update_primitives(idx, rows, rebuild=rebuild)
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rate(r, cam, rt, reps=3):
    """(best Msamples/s by kernel time, the frame, upload_ms the first of the renders reports)."""
    best, img, up = 0.0, None, None
    for _ in range(reps):
        img, st = r.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
        up = st["upload_ms"] if up is None else up
        best = max(best, st["samples"] / (st["kernel_ms"] * 1e3))
    return best, img, up


def one(name, build, rt, tag, spp, say):
    sc = build()
    cam = sc.scene_cam
    flat = sc.flatten()
    original = prim_view(flat)["v"].copy()
    idx = small_spheres(flat)
    probe = build.probe()
    r = Renderer(0)
    try:
        # (a) the parent's way
        ups = []
        for _ in range(3):
            r.upload_scene(flat)
            _, st = r.render(probe.scene_cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
            ups.append(st["upload_ms"])
        reupload = min(ups)
        say(f"{name} {tag}: {flat.desc.n_prims} primitives, {st['bvh_entries']} wrappers; (a) re-upload + build, best of 3: {reupload:9.2f} ms")
        # (b) REFIT of every small sphere / of 1 %
        one_pct = idx[:: 100] if len(idx) >= 100 else idx[:1]
        for what, sel in (("all small spheres", idx), ("1 % of them", one_pct)):
            rows = moved_rows(flat, sel, 0.05, 1)
            timed_update(r, sel, rows)
            ms = min(timed_update(r, sel, moved_rows(flat, sel, 0.05, 2 + k)) for k in range(5))
            say(f"{name} {tag}: (b) REFIT of {what} ({len(sel)} rows), best of 5: {ms:9.3f} ms = re-upload / {reupload / ms:6.1f}")
        # (c) drift
        for reach in (0.25, 2.0, 20.0):
            rows = moved_rows(flat, idx, reach, 11)
            r.upload_scene(flat)                       # the tree of the unedited scene
            r.render(probe.scene_cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)
            timed_update(r, idx, rows)
            fit, img_fit, built_ms = rate(r, cam, rt)
            timed_update(r, idx, rows, rebuild=True)
            new, img_new, rebuilt_ms = rate(r, cam, rt)
            rebuild_ms = rebuilt_ms - built_ms         # upload_ms accumulates the handle's builds since the upload
            same = (img_fit == img_new).all(axis=2).mean()
            say(f"{name} {tag}: (c) every small sphere moved by up to {reach:5.2f}: REFIT {fit:8.1f} Msamples/s, REBUILD {new:8.1f} "
                f"Msamples/s (REFIT / REBUILD = {fit / new:5.3f}; rebuild {rebuild_ms:8.2f} ms; pixels equal {same:.5f})")
        prim_view(flat)["v"][:] = original
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "experiments", "update_primitives.txt"))
    ap.add_argument("--scenes", default="book1,million")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def book1():
        return book1_end_scene(1, scene_seed=1, image_width=a.width, samples=a.spp)
    book1.probe = lambda: book1_end_scene(1, scene_seed=1, image_width=32, samples=1)

    def million():
        return million_spheres(1, scene_seed=1, image_width=a.width, samples=max(1, a.spp // 2))
    million.probe = lambda: million_spheres(1, scene_seed=1, half_extent=2, image_width=32, samples=1)

    builds = {"book1": book1, "million": million}
    say(f"scripts/ab_update.py on {torch.cuda.get_device_name(0)}: {a.width} wide, book1 at {a.spp} spp, million at {max(1, a.spp // 2)} spp, "
        "relaxed sums, CR_BVH_REFERENCE")
    for name in a.scenes.split(","):
        for rt, tag in ((A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")):
            one(name, builds[name], rt, tag, a.spp, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
