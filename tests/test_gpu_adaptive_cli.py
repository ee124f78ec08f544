"""crucible_render --adaptive tol,min,pass,block --sample-map: the CLI writes the frame that Renderer.render_adaptive returns for
the same scene (the P6 payload is its quantised bytes) and the samples each pixel took as <frame>.samples.pfm; --timing
names the passes, the blocks stopped and the samples taken."""
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


def test_cli_writes_the_adaptive_frame_and_the_sample_map(renderer, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    stem = str(tmp_path / "frame")
    out = subprocess.check_output([CLI, "--file", stem, "--adaptive", f"{TOL},{MIN},{PASS},{BLOCK}", "--sample-map", "--timing"] + BASE,
                                  cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300)
    assert sorted(os.listdir(tmp_path)) == ["frame.ppm", "frame.samples.pfm"]
    sc = book1_end_scene(1, scene_seed=1, image_width=64, samples=16)
    renderer.upload_scene(sc.flatten())
    img, counts, st = renderer.render_adaptive(sc.scene_cam, seed=0xC0FFEE, real_type=A.CR_REAL_F32, tolerance=TOL, min_samples=MIN,
                                               pass_samples=PASS, block=BLOCK, sum_order=A.CR_SUM_RELAXED)
    assert len(np.unique(counts)) >= 2   # the frame is an adaptive one
    assert read_p6(stem + ".ppm").tobytes() == quantize_rgb8(img).tobytes()
    got = read_pfm(stem + ".samples.pfm")
    assert got.shape == counts.shape and np.array_equal(got, counts.astype(np.float32))
    line = json.loads(out.decode().strip().splitlines()[-1])
    assert line["adaptive"] == f"{TOL},{MIN},{PASS},{BLOCK}"
    assert (line["passes"], line["blocks"], line["blocks_stopped"]) == (st["passes"], st["blocks"], st["blocks_stopped"])
    assert line["samples_taken"] == st["render"]["samples"] == int(counts.sum())
    bad = subprocess.run([CLI, "--file", stem, "--adaptive", "x"] + BASE, cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--adaptive" in bad.stderr
    bad = subprocess.run([CLI, "--file", stem, "--sample-map"] + BASE, cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--sample-map" in bad.stderr
