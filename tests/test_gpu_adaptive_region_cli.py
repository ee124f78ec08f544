"""crucible_render --adaptive tol,min,pass,block --region x0,y0,w,h --sample-map: the CLI writes the region that
Renderer.render_adaptive_region returns for the same scene (the P6 payload is its quantised bytes) and the samples each of its
pixels took as a region-sized <frame>.samples.pfm; --timing names the region, the passes, the region's blocks, the blocks
stopped and the samples taken.  --aov stays refused next to --adaptive."""
import json
import os
import subprocess

import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene
from crucible_amd.renderer import quantize_rgb8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")

pytestmark = pytest.mark.gpu

BASE = ["--world", "1", "--width", "64", "--samples", "16", "--sum-order", "relaxed", "--format", "p6"]
TOL, MIN, PASS, BLOCK = 0.05, 4, 2, 8
REGION = (5, 3, 43, 29)   # of the 64 x 36 frame: unaligned, partial blocks at its right and bottom edge


def read_p6(path):
    magic, size, maxval, data = open(path, "rb").read().split(b"\n", 3)
    assert magic == b"P6" and maxval == b"255"
    w, h = (int(x) for x in size.split())
    return np.frombuffer(data, dtype=np.uint8).reshape(h, w, 3)


def read_pfm(path):
    magic, size, scale, data = open(path, "rb").read().split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"Pf" and scale == b"-1.0"
    return np.frombuffer(data, dtype="<f4").reshape(h, w)[::-1]   # top to bottom


def test_cli_writes_the_adaptive_region_and_its_sample_map(renderer, tmp_path):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    stem = str(tmp_path / "frame")
    region = ",".join(str(v) for v in REGION)
    out = subprocess.check_output([CLI, "--file", stem, "--adaptive", f"{TOL},{MIN},{PASS},{BLOCK}", "--region", region, "--sample-map",
                                   "--timing"] + BASE, cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300)
    assert sorted(os.listdir(tmp_path)) == ["frame.ppm", "frame.samples.pfm"]
    sc = book1_end_scene(1, scene_seed=1, image_width=64, samples=16)
    assert (sc.scene_cam.image_width, sc.scene_cam.image_height) == (64, 36)
    renderer.upload_scene(sc.flatten())
    img, counts, st = renderer.render_adaptive_region(sc.scene_cam, REGION, seed=0xC0FFEE, real_type=A.CR_REAL_F32, tolerance=TOL,
                                                      min_samples=MIN, pass_samples=PASS, block=BLOCK, sum_order=A.CR_SUM_RELAXED)
    assert len(np.unique(counts)) >= 2   # the region is an adaptive one
    got_img = read_p6(stem + ".ppm")
    assert got_img.shape == (29, 43, 3) and got_img.tobytes() == quantize_rgb8(img).tobytes()
    got = read_pfm(stem + ".samples.pfm")
    assert got.shape == counts.shape == (29, 43) and np.array_equal(got, counts.astype(np.float32))
    line = json.loads(out.decode().strip().splitlines()[-1])
    assert line["adaptive"] == f"{TOL},{MIN},{PASS},{BLOCK}" and line["region"] == region
    assert (line["passes"], line["blocks"], line["blocks_stopped"]) == (st["passes"], st["blocks"], st["blocks_stopped"])
    assert line["blocks"] == 6 * 4
    assert line["samples_taken"] == st["render"]["samples"] == int(counts.sum())
    bad = subprocess.run([CLI, "--file", stem, "--adaptive", f"{TOL},{MIN},{PASS},{BLOCK}", "--region", region, "--aov", "albedo"] + BASE,
                         cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--aov" in bad.stderr
    bad = subprocess.run([CLI, "--file", stem, "--adaptive", f"{TOL},{MIN},{PASS},{BLOCK}", "--region", "40,3,43,29"] + BASE,
                         cwd=ROOT, capture_output=True, text=True)   # reaches outside the frame: the library refuses it
    assert bad.returncode == 1 and "outside the frame" in bad.stderr
