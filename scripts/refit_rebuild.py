"""refit_boxes = CR_REFIT_REBUILD against refit_boxes = 1 at a late frame, where keyed primitives are far from where the
uploaded scene's tree was built -> profiles/experiments/refit_rebuild.txt.

    python scripts/refit_rebuild.py [--parent-lib PATH] [--out FILE] [--scenes movie,swarm10k,swarm1m]

Scenes: `movie` is first_movie's frame shape (400 x 225 at 50 spp, depth 5) over a swarm of 2000 keyed spheres; `swarm10k`
and `swarm1m` are 10^4 and 10^6 keyed spheres in two clusters that exchange places (480 x 270 at 16 spp, depth 6), each
rendered at the frame where every sphere has arrived.  Every (library, scene) pair runs in a child process of its own.
Per scene and precision, best of 5 after a warm-up: the parent library's refit_boxes = 1 kernel time and node_tests
(--parent-lib names a library built from the parent commit); this library's, which must be the same work; the rebuild
render's; and the frame build's tree_ms / total_ms (cr_frame_build_info) with the host and with the device builder.  A
frame build is forced each time by alternating two frames.  Times come from one session on one device; compare rows of one
run only."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5
LATE = 4          # every sphere starts in frame 0 .. 3 and travels for one frame
SHAPES = {"movie": (2000, 400, 50, 5), "swarm10k": (10 ** 4, 480, 16, 6), "swarm1m": (10 ** 6, 480, 16, 6)}


def swarm_flat(n, width, samples, depth, mode):
    """The description of the swarm, written straight into the ABI records (a million add_element calls would take minutes):
    sphere i waits until frame i % 4 (a zero NERP key), then one LERP translate key takes it to the other cluster."""
    from crucible_amd import _abi as A
    from crucible_amd.scene import FlatScene, Lambertian, Scene, Sphere
    sc = Scene.new_image(16.0 / 9.0, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    side = max(1.5, 0.12 * n ** (1.0 / 3.0))           # the clusters grow with n: about the same density at every size
    cam.look_from((0.0, 2.0 * side, 7.0 * side))
    cam.look_at((0.0, 0.5 * side, 0.0))
    cam.set_vfov(38.0)
    cam.frame = LATE
    sc.add_element(Sphere.new((0.0, -1000.0, 0.0), 1000.0, Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)), "ground")
    sc.add_element(Sphere.new((0.0, 0.5, 0.0), 0.5, Lambertian.new_from_color((0.8, 0.3, 0.2), 1.0)), "red")
    sc.add_element(Sphere.new((0.0, 0.5, 1.5), 0.5, Lambertian.new_from_color((0.2, 0.3, 0.8), 1.0)), "blue")
    sc.bvh_mode = mode
    seed = sc.flatten()                                  # three spheres: the materials and textures of the swarm
    rs = np.random.RandomState(11)
    cx = np.where(np.arange(n) % 2 == 0, -3.0 * side, 3.0 * side)
    place = lambda c: np.stack([c + rs.uniform(-side, side, n), rs.uniform(0.3, 2.0 * side, n), rs.uniform(-side, side, n)], axis=1)
    start, target = place(cx), place(-cx)
    radius = rs.uniform(0.12, 0.22, n)
    prims = [seed.prims[i] for i in range(3)]
    keys = []
    for i in range(n):
        wait = i % 4
        first = len(keys)
        for ch in range(3):
            if wait:
                keys.append(A.CrKeyframe(ch, A.CR_KEY_NERP, 0.0, float(wait), 0.0, 0.0))
            keys.append(A.CrKeyframe(ch, A.CR_KEY_LERP, float(wait), float(wait + 1), float(target[i, ch] - start[i, ch]), 0.0))
        v = (C.c_double * 9)(start[i, 0], start[i, 1], start[i, 2], radius[i])
        prims.append(A.CrPrimitive(A.CR_PRIM_SPHERE, 1 + i % 2, 0, first, len(keys) - first, 0, v))
    flat = FlatScene(prims, [seed.materials[i] for i in range(seed.desc.n_materials)], [seed.textures[i] for i in range(seed.desc.n_textures)],
                     [], keys, seed.desc.sky_kind, seed.desc.sky_image)
    flat.desc.bvh_mode = mode
    return flat, cam


def best(r, cam, rt, refit, rebuild_each_time=False):
    """Best kernel time of REPS renders after a warm-up, node_tests, and the best frame build (tree_ms, total_ms)."""
    ms, tree, total, nodes = [], [], [], None
    for rep in range(REPS + 1):
        if rebuild_each_time:                            # another interval drops the frame tree: the next render builds again
            cam.frame = LATE + 1
            cam.refit_boxes = refit
            r.render(cam, seed=1, real_type=rt, sample_begin=0, sample_count=1)
            cam.frame = LATE
        cam.refit_boxes = refit
        _, st = r.render(cam, seed=1, real_type=rt)
        if rep:
            ms.append(st["kernel_ms"])
            nodes = st["node_tests"]
            if refit == "rebuild":
                info = r.frame_build_info(rt)
                tree.append(info["tree_ms"])
                total.append(info["total_ms"])
    return min(ms), nodes, (min(tree) if tree else None), (min(total) if total else None)


def child(name):
    from crucible_amd import _abi as A
    lib_path = os.environ.get("CRUCIBLE_HIP_LIB")
    parent = bool(lib_path) and not hasattr(C.CDLL(lib_path), "cr_frame_build_info")
    if parent:
        for sym in ("cr_frame_build_info", "cr_export_render_bvh"):
            A.SYMBOLS.pop(sym)
    from crucible_amd.renderer import Renderer
    n, width, samples, depth = SHAPES[name]
    r = Renderer(0)
    for rt, rname in ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64")):
        for builder, mode in (("host", A.CR_BVH_SAH_ORDERED), ("device", A.CR_BVH_SAH_ORDERED | A.CR_BVH_BUILD_DEVICE)):
            if parent and builder == "device":
                continue
            flat, cam = swarm_flat(n, width, samples, depth, mode)
            r.upload_scene(flat)
            ms, nodes, _, _ = best(r, cam, rt, True)
            row = {"scene": name, "primitives": n + 3, "real": rname, "builder": builder, "refit_kernel_ms": ms, "refit_node_tests": nodes}
            if not parent:
                ms, nodes, tree, total = best(r, cam, rt, "rebuild", rebuild_each_time=True)
                info = r.frame_build_info(rt)
                row.update(rebuild_kernel_ms=ms, rebuild_node_tests=nodes, frame_tree_ms=tree, frame_total_ms=total,
                           built_on_device=info["built_on_device"], device_rounds=info["device_rounds"],
                           saved_ms_per_frame=row["refit_kernel_ms"] - ms)
            print(json.dumps(row), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "experiments", "refit_rebuild.txt"))
    ap.add_argument("--scenes", default="movie,swarm10k,swarm1m")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    rows = []
    for name in a.scenes.split(","):
        for which, lib in (("parent", a.parent_lib), ("this", None)):
            if which == "parent" and not lib:
                continue
            env = dict(os.environ)
            env.pop("CRUCIBLE_HIP_LIB", None)
            if lib:
                env["CRUCIBLE_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True, timeout=1100)
            if out.returncode != 0:
                print(f"{which} {name}: child failed ({out.returncode})\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}", file=sys.stderr)
                return 1
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), library=which))
                    print(rows[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("# scripts/refit_rebuild.py: refit_boxes = 1 against CR_REFIT_REBUILD at frame %d, best of %d after a warm-up; times in ms.\n" % (LATE, REPS))
        f.write("# library: parent = built from the parent commit (refit only), this = this tree.  frame_tree_ms / frame_total_ms: cr_frame_build_info.\n")
        f.write("# Break-even: a frame build pays for itself when frame_total_ms < saved_ms_per_frame.\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
