"""crucible_render --movie --adaptive ... --frames-per-launch N --sample-map: the frames of a batch come from one
cr_render_adaptive_frames_host call, and the .ppm and .samples.pfm files are those of N = 1, byte for byte.  The Python
mirror's Scene.render_movie writes the same files, batched or not, and falls back to one call per frame when the library
refuses the batch -- refit boxes over keyed primitives, which the CLI's own movie (a camera walk over static spheres) cannot
reach, so that case runs through the Python mirror on a scene with keyed primitives."""
import filecmp
import json
import os
import subprocess

import pytest

import scenes
from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")
FRAMES = 5
ADAPTIVE = "0.03,4,2,8"   # tolerance, min_samples, pass_samples, block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hiplib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    return CLI


def movie(cli, stem, fpl):
    """(artifacts directory, its file names, the --timing line)"""
    r = subprocess.run([cli, "--file", stem, "--world", "1", "--movie", "--seconds", "1", "--rate", str(FRAMES), "--width", "48", "--samples", "16",
                        "--real", "f32", "--seed", "77", "--sum-order", "relaxed", "--adaptive", ADAPTIVE, "--sample-map",
                        "--frames-per-launch", str(fpl), "--timing"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    art = os.path.join(stem, "artifacts")
    return art, sorted(os.listdir(art)), json.loads(r.stdout.strip().splitlines()[-1])


def same_files(a, b):
    (da, na), (db, nb) = a, b
    assert na == nb
    for n in na:
        assert filecmp.cmp(os.path.join(da, n), os.path.join(db, n), shallow=False), n


def read_pfm_values(path):
    import numpy as np
    _, _, _, data = open(path, "rb").read().split(b"\n", 3)
    return np.frombuffer(data, dtype="<f4")


def test_cli_batches_the_adaptive_frames_of_a_movie(cli, tmp_path):
    import numpy as np
    art1, names1, line1 = movie(cli, str(tmp_path / "one"), 1)
    assert names1 == sorted([f"image{k}.ppm" for k in range(FRAMES)] + [f"image{k}.samples.pfm" for k in range(FRAMES)])
    art3, names3, line3 = movie(cli, str(tmp_path / "three"), 3)   # frames 0..2, then frames 3, 4
    same_files((art1, names1), (art3, names3))
    # the frames are adaptive ones, and not one frame written five times
    assert len(np.unique(read_pfm_values(os.path.join(art1, "image0.samples.pfm")))) >= 2
    assert not filecmp.cmp(os.path.join(art1, "image0.ppm"), os.path.join(art1, "image4.ppm"), shallow=False)
    # --timing reports the last call's stats: the one frame 4, the two frames 3 and 4
    taken = [int(read_pfm_values(os.path.join(art1, f"image{k}.samples.pfm")).sum()) for k in range(FRAMES)]
    assert line1["samples_taken"] == taken[4] and line3["samples_taken"] == taken[3] + taken[4]
    assert line3["blocks"] == 2 * line1["blocks"]


def py_movie(monkeypatch, sc, stem, fpl, frames=FRAMES):
    monkeypatch.setenv("CRUCIBLE_SUM_ORDER", "relaxed")   # Scene.render_movie renders in its handle's default order
    sc.duration, sc.frame_rate, sc.scene_cam.frame_rate = 1.0, frames, float(frames)
    sc.seed, sc.real_type = 77, A.CR_REAL_F32
    sc.frames_per_launch, sc.sample_map = fpl, True
    tol, mn, ps, block = ADAPTIVE.split(",")
    sc.set_adaptive(float(tol), int(mn), int(ps), int(block))
    sc.render_movie(stem)
    return os.path.join(stem, "artifacts"), sorted(os.listdir(os.path.join(stem, "artifacts")))


def test_python_movie_writes_the_same_files(cli, tmp_path, monkeypatch):
    from crucible_amd.demo_builder import book1_end_scene
    from crucible_amd.scene import LERP, WORLD
    art, names, _ = movie(cli, str(tmp_path / "cpp"), 3)

    def walk():
        sc = book1_end_scene(1, scene_seed=1, image_width=48, samples=16)   # main.cpp's movie: the book1 camera walk
        sc.scene_cam.set_max_depth(5)
        sc.cam_translate_point((3.0, 2.0, 13.0), 1.0, LERP, WORLD, "from")
        return sc

    same_files((art, names), py_movie(monkeypatch, walk(), str(tmp_path / "py_three"), 3))
    same_files((art, names), py_movie(monkeypatch, walk(), str(tmp_path / "py_one"), 1))


def test_python_movie_falls_back_when_the_library_refuses_the_batch(tmp_path, monkeypatch):
    """Refit boxes over keyed primitives: the library refuses the batch (boxes are per frame), render_movie renders one frame per
    call from then on, and the files are those of the frame-by-frame movie."""
    from crucible_amd.renderer import Renderer
    calls = []
    real = Renderer.render_adaptive_frames

    def spy(self, *a, **kw):
        calls.append(len(a[1]))
        return real(self, *a, **kw)

    monkeypatch.setattr(Renderer, "render_adaptive_frames", spy)

    def moving(refit):
        sc = scenes.moving_scene(width=48, samples=16)
        sc.scene_cam.refit_boxes = refit
        return sc

    one = py_movie(monkeypatch, moving(True), str(tmp_path / "refit_one"), 1, frames=4)
    assert calls == []
    three = py_movie(monkeypatch, moving(True), str(tmp_path / "refit_three"), 3, frames=4)
    assert calls == [3]   # refused once, then never asked again
    same_files(one, three)
    assert one[1] == sorted([f"image{k}.ppm" for k in range(4)] + [f"image{k}.samples.pfm" for k in range(4)])
    # without the refit the batches go through: frames 0..2, then frame 3
    calls.clear()
    py_movie(monkeypatch, moving(False), str(tmp_path / "plain_three"), 3, frames=4)
    assert calls == [3, 1]
