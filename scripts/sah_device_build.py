"""Build times of the CR_BVH_SAH_ORDERED tree: the host builder, the device builder (CR_BVH_BUILD_DEVICE) and the LBVH,
per scene and precision, best of 5 after a warm-up -> profiles/experiments/sah_device_build.txt.

    python scripts/sah_device_build.py [--parent-lib PATH] [--out FILE] [--scenes book1,teapot,s70k,s1m]

Every (library, scene) pair runs in a child process of its own.  tree_ms and total_ms are read from the laps
CRUCIBLE_BUILD_TIMING prints, which both libraries print alike: tree = the lap "tree" minus the lap before it, total = the
last lap.  --parent-lib names a library built from the parent commit: its host build is the yardstick of the acceptance
bar (device tree_ms at 10^6 primitives at most half of it, in the same session).  The child also renders one small frame
per mode, so the file shows the render rate with and without the flag (the same tree on the same kernels)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5
DEVICE = 0x100


def make_scene(name):
    from crucible_amd.demo_builder import book1_end_scene, load_teapot, million_spheres
    if name == "book1":
        return book1_end_scene(1, scene_seed=2, image_width=480, samples=16)
    if name == "teapot":
        return load_teapot(1, image_width=480, samples=16)
    if name == "s70k":
        return million_spheres(1, half_extent=132, image_width=480, samples=16)
    if name == "s1m":
        return million_spheres(1, image_width=480, samples=16)
    raise ValueError(name)


def child(scene_name, thresholds):
    """Prints one JSON line per (real, mode, threshold)."""
    import ctypes as C
    from crucible_amd import _abi as A
    lib_path = os.environ.get("CRUCIBLE_HIP_LIB")
    has_flag = True
    if lib_path:
        has_flag = hasattr(C.CDLL(lib_path), "cr_build_info")
        if not has_flag:
            A.SYMBOLS.pop("cr_build_info")
    from crucible_amd.renderer import Renderer
    laps = tempfile.TemporaryFile(mode="w+b")
    os.dup2(laps.fileno(), 2)                       # the library's [build] laps
    os.environ["CRUCIBLE_BUILD_TIMING"] = "1"
    sc = make_scene(scene_name)
    r = Renderer(0)
    modes = [("host", A.CR_BVH_SAH_ORDERED, None)]
    if has_flag:
        modes += [("device", A.CR_BVH_SAH_ORDERED | DEVICE, t) for t in thresholds] + [("lbvh", A.CR_BVH_LBVH, None)]
    n_prims = None
    for rt, rname in ((A.CR_REAL_F32, "f32"), (A.CR_REAL_F64, "f64")):
        for label, mode, small in modes:
            if small is None:
                os.environ.pop("CRUCIBLE_SAH_SMALL", None)
            else:
                os.environ["CRUCIBLE_SAH_SMALL"] = str(small)
            sc.bvh_mode = mode
            flat = sc.flatten()
            tree, total = [], []
            n = C.c_int32()
            for rep in range(REPS + 1):
                r.upload_scene(flat)
                laps.seek(0)
                laps.truncate()
                r._check(r.lib.cr_export_bvh(r.h, rt, None, None, None, 0, C.byref(n)))
                laps.seek(0)
                got = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[build\] (.+?)\s+([0-9.]+) ms", laps.read().decode())}
                if rep:
                    tree.append(got["tree"] - got["primitive records and boxes"])
                    total.append(got["uploads and boxes"])
            row = {"scene": scene_name, "real": rname, "builder": label, "wrappers": n.value, "tree_ms": min(tree), "total_ms": min(total)}
            if has_flag:
                info = r.build_info(rt)
                row.update(small_threshold=info["small_threshold"], device_rounds=info["device_rounds"],
                           large_nodes=info["large_nodes"], small_subtrees=info["small_subtrees"])
            if label in ("host", "device") and small is None:
                img, st = r.render(sc.scene_cam, seed=1, real_type=rt)
                img, st = r.render(sc.scene_cam, seed=1, real_type=rt)
                row.update(render_msamples_per_s=st["samples"] / st["kernel_ms"] / 1e3, node_tests=st["node_tests"])
            print(json.dumps(row), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "experiments", "sah_device_build.txt"))
    ap.add_argument("--scenes", default="book1,teapot,s70k,s1m")
    ap.add_argument("--thresholds", default="64,128,512,1024")
    ap.add_argument("--child")
    a = ap.parse_args()
    thresholds = [None] + [int(t) for t in a.thresholds.split(",") if t]
    if a.child:
        return child(a.child, thresholds)
    rows = []
    for name in a.scenes.split(","):
        for which, lib in (("parent", a.parent_lib), ("this", None)):
            if which == "parent" and not lib:
                continue
            env = dict(os.environ)
            env.pop("CRUCIBLE_HIP_LIB", None)
            if lib:
                env["CRUCIBLE_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--thresholds", a.thresholds], env=env,
                                 capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(f"{which} {name}: child failed ({out.returncode})\n{out.stdout[-2000:]}", file=sys.stderr)
                return 1
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), library=which))
                    print(rows[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("# scripts/sah_device_build.py: CR_BVH_SAH_ORDERED build times in ms, best of %d after a warm-up (tree = topology and order;\n" % REPS)
        f.write("# total = the whole build with uploads and boxes).  library: parent = built from the parent commit, this = this tree.\n")
        f.write("# small_threshold without a CRUCIBLE_SAH_SMALL override is the default.\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
