"""What cr_update_materials and cr_update_image cost, against the only way there was before them: cr_upload_scene of the
edited description plus the first render's build.  Per case, in f64 and f32: the wall time of the edit up to the end of the
next cr_render_host (a host clock around work that ends in the render's synchronise) at `--width` x width*9/16 pixels and
`--spp` samples, the two ways alternating on one handle each, best of `--reps` after a warm-up pair, with the spread (worst)
beside it.  The two frames are compared byte for byte every repetition.
  book1    one material edited; all spheres reassigned
  teapot   with its 2048 x 1024 environment map: one material edited; the whole map replaced (cr_update_image against
           re-uploading it)
  million  the 1M-sphere field: one material edited
usage: python scripts/ab_update_materials.py [--out profiles/experiments/update_materials.txt] [--scenes book1,teapot,million]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime: torch first, see crucible_amd.renderer.load_library)
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.demo_builder import book1_end_scene, load_teapot, million_spheres, procedural_sky  # noqa: E402
from crucible_amd.renderer import Renderer  # noqa: E402

SEED = 0xC0FFEE
PRIM = np.dtype([("kind", "<i4"), ("material", "<i4"), ("flags", "<i4"), ("key_first", "<i4"), ("key_count", "<i4"),
                 ("_pad", "<i4"), ("v", "<f8", 9)])


def prim_view(flat):
    return np.frombuffer(flat.prims, dtype=PRIM, count=flat.desc.n_prims)


def first_metal(flat):
    return next(i for i in range(flat.desc.n_materials) if flat.materials[i].kind == A.CR_MAT_METAL)


class MaterialEdit:
    """One metal's fuzz and albedo: a different value every repetition, written into the description both ways share"""
    what = "one material edited"

    def __init__(self, flat):
        self.flat, self.i = flat, first_metal(flat)

    def step(self, k):
        m = self.flat.materials[self.i]
        m.param = 0.05 + 0.01 * (k % 7)
        m.albedo[0] = 0.3 + 0.05 * (k % 5)

    def in_place(self, r):
        r.update_materials(self.flat.materials)


class Reassign:
    """Every sphere's material rotated by k through the table"""
    what = "all spheres reassigned"

    def __init__(self, flat):
        self.flat = flat
        p = prim_view(flat)
        self.idx = np.nonzero(p["kind"] == A.CR_PRIM_SPHERE)[0].astype(np.int32)
        self.original = p["material"][self.idx].copy()

    def step(self, k):
        prim_view(self.flat)["material"][self.idx] = np.roll(self.original, k + 1)

    def in_place(self, r):
        r.update_materials(assign=(self.idx, prim_view(self.flat)["material"][self.idx]))


class Repaint:
    """The whole environment map replaced by itself rolled k columns (a video environment advancing a frame)"""
    what = "the whole 2048 x 1024 map replaced"

    def __init__(self, flat):
        self.flat, self.image = flat, flat.desc.sky_image
        self.original = flat._image_arrays[self.image].copy()

    def step(self, k):
        self.flat._image_arrays[self.image][:] = np.roll(self.original, 17 * (k + 1), axis=1)

    def in_place(self, r):
        r.update_image(self.image, self.flat._image_arrays[self.image])


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def one(name, sc, edit_type, rt, tag, reps, say):
    flat, cam = sc.flatten(), sc.scene_cam
    edit = edit_type(flat)
    render = lambda r: r.render(cam, seed=SEED, real_type=rt, sum_order=A.CR_SUM_RELAXED)[0].tobytes()
    old, new = Renderer(0), Renderer(0)
    try:
        for r in (old, new):
            r.upload_scene(flat)
            render(r)
        t_old, t_new = [], []
        for k in range(reps + 1):                       # the first pair warms both ways up
            edit.step(k)
            ms_old, a = timed(lambda: (old.upload_scene(flat), render(old))[1])
            ms_new, b = timed(lambda: (edit.in_place(new), render(new))[1])
            assert a == b, (name, tag, edit.what, k)    # faster and different is not faster
            if k:
                t_old.append(ms_old)
                t_new.append(ms_new)
        say(f"{name:8s} {tag}  {edit.what:38s}  upload + build + render: best {min(t_old):9.2f} ms (worst {max(t_old):9.2f})   "
            f"edit in place + render: best {min(t_new):8.2f} ms (worst {max(t_new):8.2f})   ratio of bests {min(t_old) / min(t_new):7.1f}   frames equal")
    finally:
        old.close()
        new.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "experiments", "update_materials.txt"))
    ap.add_argument("--scenes", default="book1,teapot,million")
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    say(f"scripts/ab_update_materials.py on {torch.cuda.get_device_name(0)}; parent commit {os.environ.get('CRUCIBLE_COMMIT') or commit or 'unknown'} plus this change")
    say("command: python " + " ".join(sys.argv))
    say(f"{a.width} x {a.width * 9 // 16} pixels, {a.spp} spp, relaxed sums, CR_BVH_REFERENCE; wall ms of the edit up to the end of the next cr_render_host, "
        f"the two ways alternating, best of {a.reps} after a warm-up pair")
    cases = {"book1": (lambda: book1_end_scene(1, scene_seed=1, image_width=a.width, samples=a.spp), (MaterialEdit, Reassign)),
             "teapot": (lambda: load_teapot(1, image_width=a.width, samples=a.spp, sky=procedural_sky()), (MaterialEdit, Repaint)),
             "million": (lambda: million_spheres(1, scene_seed=1, image_width=a.width, samples=a.spp), (MaterialEdit,))}
    for name in a.scenes.split(","):
        build, edits = cases[name]
        sc = build()
        for edit_type in edits:
            for rt, tag in ((A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")):
                one(name, sc, edit_type, rt, tag, a.reps, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
