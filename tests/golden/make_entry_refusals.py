"""Records what the eighteen cr_render_* entry points answer to bad and good calls (tests/golden/entry_refusals.json).

Every case goes through ctypes into libcrucible_hip.so on one small scene, scenes.moving_scene at 37 x 29 pixels with 16
samples: the refusals of every entry point (status and the whole text of cr_last_error), double faults that pin the
order of the checks, a handle without a scene, one good call through each of the nine host forms (status, SHA-256 of the
output and count bytes, the integer fields of the stats; CR_REAL_F64 with relaxed sums, so the bytes depend on the code
alone) and one frame with NaN pixels (scenes.nan_window_scene(0)) through the four calls that check pixels.  A refused
call launches nothing; the device forms are handed real device buffers all the same.

tests/test_gpu_entry_refusals.py replays record() against the built library and compares everything with the file.

    python tests/golden/make_entry_refusals.py            # needs the GPU; refuses to overwrite the file
    python tests/golden/make_entry_refusals.py --force    # ... unless asked
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from crucible_amd import _abi as A  # noqa: E402
import scenes  # noqa: E402

PATH = os.path.join(HERE, "entry_refusals.json")
SEED = 0xC0FFEE
W, H, SAMPLES = 37, 29, 16
FRAMES = [1, 2]
REGION = (8, 8, 24, 16)                # inside the frame, its origin on a multiple of every block side
ADAPTIVE = (4, 2, 3, 0, 0.05)          # min_samples, pass_samples, block_log2, _reserved, tolerance
OUT_BYTES = 2 * W * H * 8 * 8          # two frames of eight f64 channels: the largest output of any call here

# name -> (family, shape, host form)
ENTRIES = {
    "cr_render_device": ("render", "one", False), "cr_render_host": ("render", "one", True),
    "cr_render_frames_device": ("render", "frames", False), "cr_render_frames_host": ("render", "frames", True),
    "cr_render_region_device": ("render", "region", False), "cr_render_region_host": ("render", "region", True),
    "cr_render_aov_device": ("aov", "one", False), "cr_render_aov_host": ("aov", "one", True),
    "cr_render_aov_frames_device": ("aov", "frames", False), "cr_render_aov_frames_host": ("aov", "frames", True),
    "cr_render_aov_region_device": ("aov", "region", False), "cr_render_aov_region_host": ("aov", "region", True),
    "cr_render_adaptive_device": ("adaptive", "one", False), "cr_render_adaptive_host": ("adaptive", "one", True),
    "cr_render_adaptive_frames_device": ("adaptive", "frames", False), "cr_render_adaptive_frames_host": ("adaptive", "frames", True),
    "cr_render_adaptive_region_device": ("adaptive", "region", False), "cr_render_adaptive_region_host": ("adaptive", "region", True),
}
DOUBLE_FAULTS = ("null_output+samples_0", "frames_null+null_output", "frames_null+block_log2_2", "layers_0+null_output",
                 "region_outside+sum_reference")


def needs_relaxed(family, shape):
    return family == "adaptive" or (family == "render" and shape != "one")


def applies(case, family, shape):
    """Whether `case` (one fault's name) is a case of this family and shape."""
    if case in ("frames_null", "n_frames_0", "n_frames_-1"):
        return shape == "frames"
    if case in ("region_null", "region_outside"):
        return shape == "region"
    if case in ("layers_0", "layers_unknown_bit"):
        return family == "aov"
    if case in ("ap_null", "block_log2_2", "pass_samples_0", "min_samples_above", "tolerance_nan"):
        return family == "adaptive"
    if case == "sum_reference":
        return needs_relaxed(family, shape)
    if case == "fixed_sum":
        return family != "render"
    return True


SINGLE_FAULTS = ("null_camera", "null_params", "null_output", "frames_null", "n_frames_0", "n_frames_-1", "region_null",
                 "region_outside", "layers_0", "layers_unknown_bit", "ap_null", "block_log2_2", "pass_samples_0", "min_samples_above",
                 "tolerance_nan", "samples_0", "sample_range", "real_type_7", "sum_reference", "fixed_sum")


def case_names(family, shape):
    out = [c for c in SINGLE_FAULTS if applies(c, family, shape)]
    out += [d for d in DOUBLE_FAULTS if all(applies(c, family, shape) for c in d.split("+"))]
    return out


class Call:
    """The arguments of one call, good until a fault is applied."""

    def __init__(self, cam, real_type=A.CR_REAL_F64):
        self.cd = cam.desc()
        self.p = cam.params(SEED, real_type, 0, None, False, A.CR_SUM_RELAXED)
        self.cam_null = self.p_null = self.out_null = self.frames_null = self.region_null = self.ap_null = False
        self.layers = A.CR_AOV_ALL
        self.frames = list(FRAMES)
        self.n_frames = None               # None: len(frames)
        self.region = REGION
        self.ap = list(ADAPTIVE)

    def fault(self, name):
        p = self.p
        if name == "null_camera": self.cam_null = True
        elif name == "null_params": self.p_null = True
        elif name == "null_output": self.out_null = True
        elif name == "frames_null": self.frames_null = True
        elif name == "n_frames_0": self.n_frames = 0
        elif name == "n_frames_-1": self.n_frames = -1
        elif name == "region_null": self.region_null = True
        elif name == "region_outside": self.region = (W - 10, 4, 11, 8)
        elif name == "layers_0": self.layers = 0
        elif name == "layers_unknown_bit": self.layers = A.CR_AOV_ALBEDO | 16
        elif name == "ap_null": self.ap_null = True
        elif name == "block_log2_2": self.ap[2] = 2
        elif name == "pass_samples_0": self.ap[1] = 0
        elif name == "min_samples_above": self.ap[0] = 2 * SAMPLES
        elif name == "tolerance_nan": self.ap[4] = float("nan")
        elif name == "samples_0": p.samples = 0
        elif name == "sample_range": p.sample_begin, p.sample_count = SAMPLES // 2, SAMPLES
        elif name == "real_type_7": p.real_type = 7
        elif name == "sum_reference": p.sum_order = A.CR_SUM_REFERENCE_ORDER
        elif name == "fixed_sum": p.output_sum = A.CR_OUTPUT_FIXED_SUM
        else: raise KeyError(name)
        return self

    def run(self, lib, h, entry, out, counts, stats):
        """Status of `entry` with these arguments; out / counts: addresses in the memory the entry's form writes."""
        family, shape, _ = ENTRIES[entry]
        args = [h, None if self.cam_null else C.byref(self.cd), None if self.p_null else C.byref(self.p)]
        keep = []
        if family == "aov":
            args.append(self.layers)
        if family == "adaptive":
            keep.append(A.CrAdaptiveParams(*self.ap))
            args.append(None if self.ap_null else C.byref(keep[-1]))
        if shape == "frames":
            keep.append((C.c_int32 * len(self.frames))(*self.frames))
            args += [None if self.frames_null else keep[-1], len(self.frames) if self.n_frames is None else self.n_frames]
        if shape == "region":
            keep.append(A.CrRegion(*self.region))
            args.append(None if self.region_null else C.byref(keep[-1]))
        args.append(None if self.out_null else C.c_void_p(out))
        if family == "adaptive":
            args.append(C.c_void_p(counts) if counts else None)
        args.append(C.byref(stats) if stats is not None else None)
        return getattr(lib, entry)(*args)


def message(lib, h):
    return (lib.cr_last_error(h) or b"").decode()


def int_fields(st):
    d = st.as_dict()
    if "render" in d:
        d.update({"render." + k: v for k, v in d.pop("render").items()})
    return {k: int(v) for k, v in d.items() if not k.endswith("_ms")}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def out_shape(family, shape):
    """(frames, pixels per frame, channels per pixel) of a good call's output."""
    pix = REGION[2] * REGION[3] if shape == "region" else W * H
    return (len(FRAMES) if shape == "frames" else 1), pix, (8 if family == "aov" else 3)


def create(lib):
    h = C.c_void_p()
    rc = lib.cr_create(0, C.byref(h))
    if rc != A.CR_OK:
        raise RuntimeError("cr_create: " + (lib.cr_last_error(None) or b"").decode())
    return h


def upload(lib, h, sc):
    flat = sc.flatten()
    if lib.cr_upload_scene(h, C.byref(flat.desc)) != A.CR_OK:
        raise RuntimeError("cr_upload_scene: " + message(lib, h))


def record(lib):
    """Every case against `lib`, in the layout of entry_refusals.json."""
    import torch
    d_out = torch.zeros(OUT_BYTES, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(2 * W * H, dtype=torch.int32, device="cuda")
    h_out = np.zeros(OUT_BYTES, dtype=np.uint8)
    h_counts = np.zeros(2 * W * H, dtype=np.int32)

    def buffers(entry):
        return (h_out.ctypes.data, h_counts.ctypes.data) if ENTRIES[entry][2] else (d_out.data_ptr(), d_counts.data_ptr())

    def scene():
        sc = scenes.moving_scene(samples=SAMPLES, frame=1)
        sc.scene_cam.image_width, sc.scene_cam.image_height = W, H
        return sc

    doc = {"scene": f"scenes.moving_scene(samples={SAMPLES}, frame=1) at {W}x{H}", "refusals": {}, "no_scene": {}, "good": {}, "nan": {}}
    h, bare = create(lib), create(lib)
    try:
        sc = scene()
        upload(lib, h, sc)
        for entry, (family, shape, _) in ENTRIES.items():
            out, counts = buffers(entry)
            for name in case_names(family, shape):
                call = Call(sc.scene_cam)
                for f in name.split("+"):
                    call.fault(f)
                rc = call.run(lib, h, entry, out, counts, None)
                doc["refusals"][f"{entry}/{name}"] = {"status": rc, "message": message(lib, h)}
            rc = Call(sc.scene_cam).run(lib, bare, entry, out, counts, None)
            doc["no_scene"][entry] = {"status": rc, "message": message(lib, bare)}
        for entry, (family, shape, host) in ENTRIES.items():
            if not host:
                continue
            n, pix, ch = out_shape(family, shape)
            h_out[:] = 0
            h_counts[:] = 0
            st = A.CrAdaptiveStats() if family == "adaptive" else A.CrStats()
            rc = Call(sc.scene_cam).run(lib, h, entry, h_out.ctypes.data, h_counts.ctypes.data, st)
            rec = {"status": rc, "output_sha256": sha(h_out[:n * pix * ch * 8]), "stats": int_fields(st)}
            if family == "adaptive":
                rec["counts_sha256"] = sha(h_counts[:n * pix])
            doc["good"][entry] = rec
        nan_sc = scenes.nan_window_scene(0)
        upload(lib, h, nan_sc)
        for entry in ("cr_render_host", "cr_render_frames_host", "cr_render_adaptive_host", "cr_render_adaptive_frames_host"):
            family = ENTRIES[entry][0]
            call = Call(nan_sc.scene_cam)
            call.frames = [1, 0]
            st = A.CrAdaptiveStats() if family == "adaptive" else A.CrStats()
            rc = call.run(lib, h, entry, h_out.ctypes.data, h_counts.ctypes.data, st)
            doc["nan"][entry] = {"status": rc, "message": message(lib, h),
                                 "nan_pixels": int(st.render.nan_pixels if family == "adaptive" else st.nan_pixels)}
        torch.cuda.synchronize()
    finally:
        lib.cr_destroy(h)
        lib.cr_destroy(bare)
    return doc


if __name__ == "__main__":
    if os.path.exists(PATH) and "--force" not in sys.argv[1:]:
        sys.exit(f"{PATH} exists: it is written once, by the library the refactor starts from (--force overwrites it)")
    from crucible_amd.renderer import load_library
    doc = record(load_library())
    bad = [k for k, v in list(doc["refusals"].items()) + list(doc["no_scene"].items()) if v["status"] == A.CR_OK]
    bad += [k for k, v in doc["good"].items() if v["status"] != A.CR_OK] + [k for k, v in doc["nan"].items() if v["status"] != A.CR_ERR_NAN]
    if bad:
        sys.exit("not what the case is about: " + ", ".join(bad))
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {PATH}: {len(doc['refusals'])} refusals, {len(doc['no_scene'])} calls without a scene, "
          f"{len(doc['good'])} good calls, {len(doc['nan'])} NaN frames")
