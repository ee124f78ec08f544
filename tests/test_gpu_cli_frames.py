"""crucible_render --frames-per-launch N: a movie rendered N frames per library call (cr_render_frames_host) writes the
files one frame per call writes, byte for byte -- batched under relaxed sums, and one frame per call after the library
refuses the batch under the reference order.  With two devices, the per-device threads pass their frames m, m + 2, ...
as strided lists."""
import filecmp
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crucible_amd", "host", "crucible_render")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hiplib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "crucible_amd", "host"), "all"])
    return CLI


def movie(cli, stem, order, fpl, gpus=1):
    subprocess.check_call([cli, "--file", stem, "--world", "1", "--movie", "--seconds", "6", "--rate", "1", "--width", "48",
                           "--samples", "4", "--real", "f64", "--sum-order", order, "--frames-per-launch", str(fpl),
                           "--gpus", str(gpus)], cwd=ROOT, stderr=subprocess.DEVNULL, timeout=600)
    art = os.path.join(stem, "artifacts")
    return art, sorted(os.listdir(art))


def same_files(a, b):
    (da, na), (db, nb) = a, b
    assert len(na) == 6 and na == nb
    for n in na:
        assert filecmp.cmp(os.path.join(da, n), os.path.join(db, n), shallow=False), n


@pytest.mark.parametrize("order", ["relaxed", "reference"])
def test_cli_frames_per_launch_writes_the_same_files(cli, tmp_path, order):
    import torch
    one = movie(cli, str(tmp_path / "one"), order, 1)
    same_files(one, movie(cli, str(tmp_path / "four"), order, 4))
    same_files(one, movie(cli, str(tmp_path / "all"), order, 6))
    if torch.cuda.device_count() >= 2:   # per-device threads: frames 0, 2, 4 and 1, 3, 5 as strided batches
        same_files(one, movie(cli, str(tmp_path / "two_gpus"), order, 4, gpus=2))
