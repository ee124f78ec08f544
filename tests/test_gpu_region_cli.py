"""crucible_render --region x0,y0,w,h: the CLI writes the region as a w x h file whose pixel payload is the crop of the
full frame's file, and with --aov the region's .pfm planes, the crops of the full planes (rows bottom to top)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")

pytestmark = pytest.mark.gpu

REGION = (5, 3, 13, 9)
BASE = ["--world", "1", "--width", "64", "--samples", "4", "--sum-order", "relaxed", "--format", "p6"]


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


def test_cli_writes_the_region(hiplib, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    x0, y0, w, h = REGION
    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    subprocess.check_call([CLI, "--file", full, "--aov", "depth"] + BASE, cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300)
    out = subprocess.check_output([CLI, "--file", part, "--aov", "depth", "--region", "5,3,13,9", "--timing"] + BASE, cwd=ROOT,
                                  stderr=subprocess.DEVNULL, timeout=300)
    assert sorted(os.listdir(tmp_path)) == ["full.depth.pfm", "full.ppm", "part.depth.pfm", "part.ppm"]
    whole, region = read_p6(full + ".ppm"), read_p6(part + ".ppm")
    assert region.shape == (h, w, 3)
    assert region.tobytes() == np.ascontiguousarray(whole[y0:y0 + h, x0:x0 + w]).tobytes()
    depth, rdepth = read_pfm(full + ".depth.pfm"), read_pfm(part + ".depth.pfm")
    assert rdepth.shape == (h, w)
    assert rdepth.tobytes() == np.ascontiguousarray(depth[y0:y0 + h, x0:x0 + w]).tobytes()
    assert json.loads(out.decode().strip().splitlines()[-1])["region"] == "5,3,13,9"
    bad = subprocess.run([CLI, "--file", part, "--region", "5,3,13"] + BASE, cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--region" in bad.stderr
