"""The eighteen cr_render_* entry points answer as tests/golden/entry_refusals.json records: every refusal's status and
whole message (double faults pin the order of the checks), a handle without a scene, one good call per host form (the
output's and the counts' bytes, the integer stats) and a frame with NaN pixels through the calls that check them.  The
file was written once, by the library as it stood before the entry points were gathered behind one call descriptor
(tests/golden/make_entry_refusals.py has the cases); the replay launches nine 37 x 29 frames and the NaN frame's four."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_entry_refusals", os.path.join(GOLDEN, "make_entry_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()


@pytest.fixture(scope="module")
def want():
    with open(gen.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(hiplib):
    return gen.record(hiplib)


@pytest.mark.parametrize("section", ["refusals", "no_scene", "good", "nan"])
def test_entry_points_answer_as_recorded(want, got, section):
    assert sorted(got[section]) == sorted(want[section])
    diff = {k: (got[section][k], want[section][k]) for k in want[section] if got[section][k] != want[section][k]}
    for k, (g, w) in diff.items():
        print(f"{section} {k}:\n  got  {g}\n  want {w}")
    assert not diff, f"{len(diff)} of {len(want[section])} {section} cases differ: {sorted(diff)[:8]}"


def test_fixture_is_not_vacuous(want):
    from crucible_amd import _abi as A
    assert len(gen.ENTRIES) == 18
    refusals = want["refusals"]
    for entry, (family, shape, host) in gen.ENTRIES.items():
        names = gen.case_names(family, shape)
        assert {"null_camera", "null_params", "null_output", "samples_0", "sample_range", "real_type_7", "null_output+samples_0"} <= set(names)
        for name in names:
            assert refusals[f"{entry}/{name}"]["status"] != A.CR_OK, (entry, name)
        assert want["no_scene"][entry]["status"] == A.CR_ERR_NO_SCENE
        if host:
            assert want["good"][entry]["status"] == A.CR_OK and want["good"][entry]["stats"]["samples" if family != "adaptive" else "render.samples"] > 0
    for d in gen.DOUBLE_FAULTS:
        assert any(k.endswith("/" + d) for k in refusals), d
    for family in ("render", "aov", "adaptive"):
        texts = {v["message"] for k, v in refusals.items() if gen.ENTRIES[k.split("/")[0]][0] == family}
        assert len(texts) >= 2, family
    assert len(want["good"]) == 9 and len(want["nan"]) == 4
    for entry, rec in want["nan"].items():
        assert rec["status"] == A.CR_ERR_NAN and rec["nan_pixels"] > 0
        assert ("frame 0 (entry 1 of the batch)" in rec["message"]) == ("frames" in entry)
