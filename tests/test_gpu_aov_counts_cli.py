"""crucible_render --adaptive ... --adaptive-aov albedo,depth --sample-map: the guide files of an adaptive frame, of a region
and of a movie's batches hold the planes Renderer.render_aov_counts* computes over the adaptive call's counts (a .pfm stores
its rows bottom to top).  The Python mirror's Scene writes the same files with set_adaptive(..., guide_at_counts=True), and
with the default False the files of the plain guide pass at the maximum sample count, as before."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer, write_pfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")
ADAPTIVE = "0.03,4,2,8"   # tolerance, min_samples, pass_samples, block
AD = dict(tolerance=0.03, min_samples=4, pass_samples=2, block=8)
LAYERS = ("albedo", "depth")
SEED, WIDTH, SAMPLES = 77, 48, 16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hiplib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    return CLI


def run_cli(cli, stem, *extra):
    r = subprocess.run([cli, "--file", stem, "--world", "1", "--width", str(WIDTH), "--samples", str(SAMPLES), "--real", "f32", "--seed", str(SEED),
                        "--sum-order", "relaxed", "--adaptive", ADAPTIVE, "--adaptive-aov", ",".join(LAYERS), "--sample-map", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def read_pfm(path):
    """(H, W) or (H, W, 3) float32, rows top to bottom"""
    kind, size, _, data = open(path, "rb").read().split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    a = np.frombuffer(data, dtype="<f4").reshape((h, w, 3) if kind == b"PF" else (h, w))
    return a[::-1]


def book1():
    from crucible_amd.demo_builder import book1_end_scene
    return book1_end_scene(1, scene_seed=1, image_width=WIDTH, samples=SAMPLES)


def walk():
    from crucible_amd.scene import LERP, WORLD
    sc = book1()   # main.cpp's movie: the book1 camera walk
    sc.scene_cam.set_max_depth(5)
    sc.cam_translate_point((3.0, 2.0, 13.0), 1.0, LERP, WORLD, "from")
    sc.duration, sc.frame_rate, sc.scene_cam.frame_rate = 1.0, 3, 3.0
    return sc


def check_files(stem, planes, counts):
    """<stem>.<layer>.pfm hold `planes`, <stem>.samples.pfm holds `counts`; no other guide file"""
    for n in LAYERS:
        assert read_pfm(f"{stem}.{n}.pfm").tobytes() == planes[n].tobytes(), (stem, n)
    assert np.array_equal(read_pfm(stem + ".samples.pfm"), counts.astype(np.float32))
    assert not os.path.exists(stem + ".normal.pfm") and not os.path.exists(stem + ".coverage.pfm")


@pytest.fixture()
def relaxed(monkeypatch):
    monkeypatch.setenv("CRUCIBLE_SUM_ORDER", "relaxed")   # the adaptive calls need it; a handle reads it when it is created


def test_a_frame_and_a_region(cli, tmp_path, relaxed):
    sc = book1()
    cam = sc.scene_cam
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        _, counts, _ = r.render_adaptive(cam, seed=SEED, real_type=A.CR_REAL_F32, **AD)
        assert len(np.unique(counts)) >= 2
        planes, _ = r.render_aov_counts(cam, counts, LAYERS, seed=SEED, real_type=A.CR_REAL_F32)
        plain, _ = r.render_aov(cam, LAYERS, seed=SEED, real_type=A.CR_REAL_F32)
        assert planes["albedo"].tobytes() != plain["albedo"].tobytes()   # the files below can tell the two passes apart
        reg = (5, 3, 29, 21)
        _, rcounts, _ = r.render_adaptive_region(cam, reg, seed=SEED, real_type=A.CR_REAL_F32, **AD)
        rplanes, _ = r.render_aov_counts_region(cam, reg, rcounts, LAYERS, seed=SEED, real_type=A.CR_REAL_F32)
    finally:
        r.close()
    stem = str(tmp_path / "frame")
    run_cli(cli, stem)
    check_files(stem, planes, counts)
    rstem = str(tmp_path / "region")
    run_cli(cli, rstem, "--region", ",".join(str(v) for v in reg))
    check_files(rstem, rplanes, rcounts)
    # the Python Scene: the same files with the switch, the plain guide pass's without it
    for at_counts, want in ((True, planes), (False, plain)):
        py = book1()
        py.seed, py.real_type, py.aov_layers, py.sample_map = SEED, A.CR_REAL_F32, LAYERS, True
        py.set_adaptive(guide_at_counts=at_counts, **AD) if at_counts else py.set_adaptive(**AD)
        pstem = str(tmp_path / f"py_{at_counts}")
        py.render_image(pstem)
        for n in LAYERS:
            assert filecmp.cmp(f"{pstem}.{n}.pfm", f"{stem}.{n}.pfm", shallow=False) == at_counts, (at_counts, n)
            write_pfm(str(tmp_path / "want.pfm"), want[n])
            assert filecmp.cmp(f"{pstem}.{n}.pfm", str(tmp_path / "want.pfm"), shallow=False), (at_counts, n)
        assert filecmp.cmp(pstem + ".samples.pfm", stem + ".samples.pfm", shallow=False)
        assert filecmp.cmp(pstem + ".ppm", stem + ".ppm", shallow=False)


def test_a_movie_in_batches(cli, tmp_path, relaxed):
    stem = str(tmp_path / "movie")
    run_cli(cli, stem, "--movie", "--seconds", "1", "--rate", "3", "--frames-per-launch", "2")   # frames 0 and 1, then frame 2
    art = os.path.join(stem, "artifacts")
    names = sorted(os.listdir(art))
    assert names == sorted(f"image{k}{ext}" for k in range(3) for ext in (".ppm", ".samples.pfm", ".albedo.pfm", ".depth.pfm"))
    sc = walk()
    cam = sc.scene_cam
    r = Renderer(0)
    try:
        r.upload_scene(sc.flatten())
        _, counts, _ = r.render_adaptive_frames(cam, [0, 1, 2], seed=SEED, real_type=A.CR_REAL_F32, **AD)
        frames, _ = r.render_aov_counts_frames(cam, [0, 1, 2], counts, LAYERS, seed=SEED, real_type=A.CR_REAL_F32)
    finally:
        r.close()
    assert len(np.unique(counts)) >= 2 and frames[0]["depth"].tobytes() != frames[2]["depth"].tobytes()
    for k in range(3):
        check_files(os.path.join(art, f"image{k}"), frames[k], counts[k])
    # the Python Scene, batched and frame by frame: the same files
    for fpl in (2, 1):
        py = walk()
        py.seed, py.real_type, py.aov_layers, py.sample_map, py.frames_per_launch = SEED, A.CR_REAL_F32, LAYERS, True, fpl
        py.set_adaptive(guide_at_counts=True, **AD)
        pstem = str(tmp_path / f"py_movie_{fpl}")
        py.render_movie(pstem)
        assert sorted(os.listdir(os.path.join(pstem, "artifacts"))) == names
        for n in names:
            assert filecmp.cmp(os.path.join(pstem, "artifacts", n), os.path.join(art, n), shallow=False), (fpl, n)
