"""crucible_render --aov albedo,depth: the CLI writes <file>.albedo.pfm and <file>.depth.pfm next to the frame -- the
planes Renderer.render_aov returns for the mirrored scene, rounded to f32, rows bottom to top -- and the frame file
itself is the one a run without the flag writes, byte for byte."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")

pytestmark = pytest.mark.gpu


def read_pfm(path):
    magic, size, scale, data = open(path, "rb").read().split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert scale == b"-1.0"
    ch = {b"PF": 3, b"Pf": 1}[magic]
    a = np.frombuffer(data, dtype="<f4").reshape((h, w, 3) if ch == 3 else (h, w))
    return a[::-1]   # top to bottom


def test_cli_writes_the_guide_layers(hiplib, renderer, tmp_path):
    from crucible_amd.demo_builder import book1_end_scene
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    base = ["--world", "1", "--width", "32", "--samples", "4", "--real", "f64", "--seed", "77"]
    plain, guided = str(tmp_path / "plain"), str(tmp_path / "guided")
    subprocess.check_call([CLI, "--file", plain] + base, cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300)
    subprocess.check_call([CLI, "--file", guided, "--aov", "albedo,depth"] + base, cwd=ROOT, stderr=subprocess.DEVNULL, timeout=300)
    assert filecmp.cmp(plain + ".ppm", guided + ".ppm", shallow=False)
    assert sorted(os.listdir(tmp_path)) == ["guided.albedo.pfm", "guided.depth.pfm", "guided.ppm", "plain.ppm"]
    sc = book1_end_scene(1, scene_seed=1, image_width=32, samples=4)
    renderer.upload_scene(sc.flatten())
    want, _ = renderer.render_aov(sc.scene_cam, ("albedo", "depth"), seed=77, real_type=A.CR_REAL_F64)
    for name in ("albedo", "depth"):
        got = read_pfm(f"{guided}.{name}.pfm")
        assert got.shape == want[name].shape
        assert got.tobytes() == want[name].astype(np.float32).tobytes(), name
    bad = subprocess.run([CLI, "--file", plain, "--aov", "albedo,colour"] + base, cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--aov" in bad.stderr
