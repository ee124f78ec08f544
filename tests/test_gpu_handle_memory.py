"""A handle gives its device memory back, and does not grow while the sizes of its calls stay the same.

Device memory is read with torch.cuda.mem_get_info (the whole card's free bytes), so three things blur the reading: the
runtime's own drift, other processes on a shared card, and the allocation granule -- a buffer of a few hundred bytes that is
never freed costs nothing visible until its granule fills.  Hence

  * the jobs of LARGE are sized so that the per-pixel buffers of a call (fx_acc, aov_acc, aov_flags, aov_counts, ad_acc,
    ad_counts, out_buf, sample_buf, sg_acc, att_stack, the wf_* buffers of the wavefront pipeline, a group's partial sums)
    are at least 2 MiB each: 1024 x 512 pixels at 2 samples, still milliseconds;
  * the tolerance is measured, not fixed: a control loop of the same length creates and destroys handles that run nothing, and
    the tolerance is twice its drift plus 16 MiB -- half of what the smallest tracked buffer (2 MiB) would lose over 16 cycles;
  * a loop that exceeds the tolerance is repeated, up to three times, and the test fails only if every repetition does: a
    real leak repeats exactly, a neighbour's allocation does not.

What this cannot see: a leak below one allocation granule per cycle (ad_ctrl, ad_block_n, ad_lists, times_dev,
update_stage, the screen_overflow word, events and pinned host slots), and a buffer that DevBuf::ensure frees and allocates
again at the same size on every call (no growth, only time).  tests/test_handle_lifetime_host.py covers the first by name.
The figures of one run are in profiles/experiments/handle_memory.txt."""
from dataclasses import replace

import numpy as np
import pytest

import history_jobs as J
from crucible_amd import _abi as A
from test_gpu_history import ENVS, open_session

pytestmark = pytest.mark.gpu

MIB = 1 << 20
BIG = (1024, 512)
CYCLES, WARM_CYCLES, TABLE_RUNS, REPEATS = 16, 2, 20, 3
SMALLEST_TRACKED = 2 * MIB
SLACK = CYCLES * SMALLEST_TRACKED // 2


def big(family, shape, host, rt, **kw):
    kw.setdefault("samples", 4 if family == "adaptive" else 2)
    if family == "adaptive":
        kw.update(min_samples=2, pass_samples=1)
    return J.Call(family, shape, host, rt, size=BIG, frames=(1, 2), region=(0, 0, 1024, 512), **kw)


LARGE = J.Job("large", (big("render", "one", True, J.F64), big("render", "one", True, J.F32, order=J.REFERENCE), big("render", "frames", False, J.F32),
                        big("aov", "one", True, J.F64), big("aov", "frames", False, J.F32), big("counts", "one", True, J.F64, counts="steps"),
                        big("adaptive", "one", True, J.F64), big("adaptive", "frames", True, J.F32), big("render", "region", True, J.F64),
                        J.Update(False), J.Update(True, restore=True), big("render", "one", True, J.F64, refit="rebuild")))
# the cross-check pipelines: reference-order frames, a quarter of the pixels (a wavefront slot carries a whole path state, so its buffers are far larger per pixel)
LARGE_REFERENCE = J.Job("large-reference", (replace(big("render", "one", True, J.F64, order=J.REFERENCE), size=(512, 256)),
                                            replace(big("render", "one", False, J.F32, order=J.REFERENCE), size=(512, 256))))


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def lost_over(loop, warm, n):
    """Free memory before minus after `n` rounds of `loop`, after `warm` rounds that are not counted."""
    for _ in range(warm):
        loop()
    before = free_bytes()
    for _ in range(n):
        loop()
    return before - free_bytes()


def settle(measure, control, what):
    """Up to REPEATS times: the control loop's drift, then the measured loop's loss.  Passes once a repetition stays within
    twice the control's drift plus SLACK; prints every figure."""
    figures = []
    for k in range(REPEATS):
        drift = control()
        lost = measure()
        tolerance = 2 * max(0, drift) + SLACK
        figures.append((drift, lost, tolerance))
        print(f"{what}: repetition {k}: control {drift / MIB:+.2f} MiB, measured {lost / MIB:+.2f} MiB, tolerance {tolerance / MIB:.2f} MiB")
        if lost <= tolerance:
            return figures
    raise AssertionError(f"{what}: device memory is not given back in any of {REPEATS} repetitions (control, lost, tolerance in bytes): {figures}")


def expect_ok(job, results):
    for step, res in zip(job.steps, results):
        assert res["rc"] == A.CR_OK, (job.name, step, res["rc"], res["msg"])


def test_the_large_job_reaches_two_mib_per_buffer():
    """The sizes behind the module's claim, from handle.hpp's own words per pixel."""
    pixels = BIG[0] * BIG[1]
    per_pixel = {"fx_acc": 3 * 8, "aov_acc": 8 * 8, "aov_flags": 4, "aov_counts": 4, "ad_acc": 2 * 3 * 8, "ad_counts": 4, "out_buf f32": 3 * 4, "sg_acc f32": 3 * 4}
    for name, b in per_pixel.items():
        assert pixels * b >= SMALLEST_TRACKED, name
    families = {(s.family, s.shape) for s in LARGE.steps if isinstance(s, J.Call)}
    assert {("render", "one"), ("render", "frames"), ("render", "region"), ("aov", "one"), ("counts", "one"), ("adaptive", "one"), ("adaptive", "frames")} <= families
    assert any(isinstance(s, J.Call) and s.sum_order == J.REFERENCE for s in LARGE.steps) and any(isinstance(s, J.Update) for s in LARGE.steps)


def test_no_growth_at_a_fixed_size(hiplib):
    """One handle: every job once as a warm-up (every buffer reaches its largest size), then the whole table 20 more times."""
    with J.Session(hiplib, "A") as s:
        def table():
            for job in J.TABLE + (LARGE,):
                s.run(job)
            return s.collect()

        expect_ok(LARGE, table()[-1])

        def control():
            def loop():
                with J.Session(hiplib, "A", upload=False):
                    pass
            return lost_over(loop, WARM_CYCLES, TABLE_RUNS)

        settle(lambda: lost_over(table, 0, TABLE_RUNS), control, "fixed size")


@pytest.mark.parametrize("env_name", [None, "wavefront", "queue"], ids=["mega", "wavefront", "queue"])
def test_everything_comes_back(hiplib, monkeypatch, env_name):
    """Create, upload, the jobs, destroy: 2 cycles to warm up, 16 measured."""
    jobs = (J.PLAIN + (LARGE,)) if env_name is None else (J.RENDER_JOBS + (LARGE_REFERENCE,))

    def cycle():
        with open_session(hiplib, "A", monkeypatch, ENVS.get(env_name)) as s:
            for job in jobs:
                s.run(job)
            expect_ok(jobs[-1], s.collect()[-1])

    def bare():
        with J.Session(hiplib, "A", upload=False):
            pass

    settle(lambda: lost_over(cycle, WARM_CYCLES, CYCLES), lambda: lost_over(bare, WARM_CYCLES, CYCLES), f"cycles ({env_name or 'mega'})")


def test_a_group_gives_everything_back(hiplib, monkeypatch):
    """Two members on one device: their handles, the partial sums, the flag and status buffers."""
    import ctypes as C
    monkeypatch.setenv("CRUCIBLE_GROUP_SAME_DEVICE", "1")
    sc = J.base_scene("A")
    flat = sc.flatten()
    cam = J.camera_of(sc, big("render", "one", True, J.F64))
    want = {}

    def group(render):
        ids = (C.c_int32 * 2)(0, 0)
        g = C.c_void_p()
        assert hiplib.cr_group_create(ids, 2, C.byref(g)) == A.CR_OK, hiplib.cr_group_last_error(None)
        try:
            if not render:
                return
            assert hiplib.cr_group_upload_scene(g, C.byref(flat.desc)) == A.CR_OK, hiplib.cr_group_last_error(g)
            for rt, order in ((J.F64, J.RELAX), (J.F32, J.REFERENCE)):
                cd, p = cam.desc(), cam.params(J.SEED, rt, sum_order=order)
                out = np.zeros((BIG[1], BIG[0], 3), dtype=J.NP_REAL[rt])
                st = A.CrGroupStats()
                rc = hiplib.cr_group_render_host(g, C.byref(cd), C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(st))
                assert rc == A.CR_OK and st.members == 2, hiplib.cr_group_last_error(g)
                assert want.setdefault((rt, order), out.tobytes()) == out.tobytes()      # and every cycle renders the same frame
        finally:
            hiplib.cr_group_destroy(g)

    settle(lambda: lost_over(lambda: group(True), WARM_CYCLES, CYCLES), lambda: lost_over(lambda: group(False), WARM_CYCLES, CYCLES), "group cycles")
