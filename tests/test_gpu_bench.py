"""bench.py end to end on the device at a tiny size: a plain run prints the headline line without the `--full` keys and
dumps the frame it timed; `--full` adds them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_KEYS = {"f32_fast_mode", "reference_order", "opt_in_tree", "cpu_baseline", "cpu_baseline_faithful"}


def run_bench(*args, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--width", "96",
                        "--spp", "4", *args], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["unit"] == "Msamples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    return rec


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_oracle_frame(tmp_path, o64):
    from crucible_amd.demo_builder import book1_end_scene
    rec = run_bench("--dump-outputs", str(tmp_path))     # the session's parity mode reaches it through CRUCIBLE_SUM_ORDER
    assert not FULL_KEYS & rec.keys()
    assert rec["roofline"]["counters_per_launch"]["samples"] == 96 * 54 * 4
    ref, _ = o64.render_image(book1_end_scene(1, scene_seed=1, image_width=96, samples=4), seed=0xC0FFEE)
    assert np.array_equal(np.load(tmp_path / "image.npy"), ref)


@pytest.mark.gpu
def test_full_run_adds_the_extra_lines():
    env = {k: v for k, v in os.environ.items() if k != "CRUCIBLE_SUM_ORDER"}   # the library default, which has a reference_order line
    rec = run_bench("--full", env=env)
    assert FULL_KEYS <= rec.keys()
    assert rec["reference_order"]["counters_equal"] and rec["reference_order"]["max_abs_difference_of_the_measured_frame"] <= 1e-12
