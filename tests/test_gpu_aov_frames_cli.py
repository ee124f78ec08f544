"""crucible_render --movie --aov ... --frames-per-launch N: the guide layers of a batch of frames come from one
cr_render_aov_frames_host call, and the files are those of N = 1, byte for byte.  The suite runs with
CRUCIBLE_SUM_ORDER=reference, under which the library refuses the batch of beauty frames (the CLI then renders those one
per call) and still batches the guide layers, which do not depend on the sum order.  The Python mirror's
Scene.render_movie writes the same files."""
import filecmp
import json
import os
import subprocess

import pytest

from crucible_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")
LAYERS = ("albedo", "normal", "depth", "coverage")
FRAMES = 4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hiplib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    return CLI


def movie(cli, stem, fpl):
    """(artifacts directory, its file names, guide calls the run made)"""
    r = subprocess.run([cli, "--file", stem, "--world", "1", "--movie", "--seconds", "1", "--rate", str(FRAMES), "--width", "32", "--samples", "2",
                        "--real", "f32", "--seed", "77", "--aov", ",".join(LAYERS), "--frames-per-launch", str(fpl), "--timing"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    art = os.path.join(stem, "artifacts")
    return art, sorted(os.listdir(art)), json.loads(r.stdout.strip().splitlines()[-1])["guide_calls"]


def same_files(a, b):
    (da, na), (db, nb) = a, b
    assert na == nb
    for n in na:
        assert filecmp.cmp(os.path.join(da, n), os.path.join(db, n), shallow=False), n


def test_cli_batches_the_guide_layers_of_a_movie(cli, tmp_path):
    art1, names1, calls1 = movie(cli, str(tmp_path / "one"), 1)
    assert names1 == sorted([f"image{k}.ppm" for k in range(FRAMES)] + [f"image{k}.{n}.pfm" for k in range(FRAMES) for n in LAYERS])
    assert calls1 == FRAMES
    art3, names3, calls3 = movie(cli, str(tmp_path / "three"), 3)
    assert calls3 == 2   # frames 0..2, then frame 3
    same_files((art1, names1), (art3, names3))
    # the frames are not one frame written four times
    assert not filecmp.cmp(os.path.join(art1, "image0.albedo.pfm"), os.path.join(art1, "image3.albedo.pfm"), shallow=False)


def test_python_movie_writes_the_same_guide_layers(cli, tmp_path):
    from crucible_amd.demo_builder import book1_end_scene
    from crucible_amd.scene import LERP, WORLD
    art, names, _ = movie(cli, str(tmp_path / "cpp"), 3)

    def py_movie(stem, fpl, layers):
        sc = book1_end_scene(1, scene_seed=1, image_width=32, samples=2)   # main.cpp's movie: the book1 camera walk
        sc.duration, sc.frame_rate, sc.scene_cam.frame_rate = 1.0, FRAMES, float(FRAMES)
        sc.scene_cam.set_max_depth(5)
        sc.cam_translate_point((3.0, 2.0, 13.0), 1.0, LERP, WORLD, "from")
        sc.seed, sc.real_type = 77, A.CR_REAL_F32
        sc.frames_per_launch, sc.aov_layers = fpl, layers
        sc.render_movie(stem)
        return os.path.join(stem, "artifacts"), sorted(os.listdir(os.path.join(stem, "artifacts")))

    same_files((art, names), py_movie(str(tmp_path / "py_three"), 3, LAYERS))
    same_files((art, names), py_movie(str(tmp_path / "py_one"), 1, A.CR_AOV_ALL))   # a mask, one frame per call
