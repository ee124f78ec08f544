"""The fuzz corpora of tests/test_gpu_fuzz.py, and a directed scene with partial NaN flags, through the entry points that came
after tests/test_gpu_fuzz_entry_points.py: cr_render_region_*, cr_render_aov_region_*, cr_render_adaptive_*,
cr_render_adaptive_frames_* and the pathtrace_kernel_listed kernels the adaptive calls run on.  No tolerance anywhere: words,
frames, counts and planes are compared as bytes, the positions of the NaNs on their own first (same_image, same_words).

The references never come from the device.  Adaptive renders: tests/adaptive_model.py fed with the relaxed ORACLE's per-pass
CR_OUTPUT_FIXED_SUM words (pass_words).  Regions: crops of the relaxed oracle's words and frame, its counters row by row.
Guide regions: crops of tests/test_gpu_aov.py's model.  The scene rota of tests/test_gpu_fuzz.py by seed % 3 stays: 0 the
reference tree, 1 refit_boxes, 2 an opt-in tree of TREES, exported and handed to the oracle.

scenes.nan_window_scene(0) is the first frame in the suite where flagged words (bit 63 of a relaxed sum) sit beside ordinary
magnitudes, in some pixels and some passes only; what it and the corpora have to contain is asserted on the CPU, from the
oracle and the model alone (test_nan_window_scene_has_the_classes, test_corpora_give_mixed_decisions).

A CR_ERR_NAN from a host form is pinned by its status, its message and stats.render.nan_pixels only (host_adaptive,
host_region: ctypes calls with their own buffers); bytes and counts come from the device forms, which run no Color::new
check, into torch tensors."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as M
import scenes
from crucible_amd import _abi as A
from crucible_amd.renderer import Renderer, adaptive_arg
from test_gpu_aov import NAMES, model
from test_gpu_fuzz import BIG_SEEDS, COUNTERS, HOSTILE_SEEDS, RANDOM_SEEDS
from test_gpu_fuzz_entry_points import DIRECTED, REAL_IDS, REALS, make_scene, same_planes, set_variant
from test_gpu_region import EXTRA, combine, crop, scaled
from test_gpu_region import P as PARTITION

gpu = pytest.mark.gpu

SEED = 0xC0FFEE
RELAX, FIXED = A.CR_SUM_RELAXED, A.CR_OUTPUT_FIXED_SUM
FLAG, MAG = M.FLAG, M.MAG
ORACLE_THREADS = 4        # the images are at most 73 pixels wide
NAN_MESSAGE = "a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)"
# hostile seeds whose camera has no basis, no focus distance or a half-turn field of view so that every pixel of the frame
# is flagged, in both precisions (test_corpora_give_mixed_decisions asserts it)
FULLY_FLAGGED = [1200001, 1200002, 1200004, 1200005, 1200006]
# test_adaptive_on_the_corpora: (samples, pass_samples, min_samples, block); the big scenes at 8 samples, for the oracle's sake
CORPUS_RUN = {"random": (12, 2, 4, 8), "hostile": (12, 2, 4, 8), "big": (8, 2, 4, 8)}
# test_adaptive_nan_window and the batches: 16 samples, passes of 2, judged from 4 on
WINDOW_RUN = (16, 2, 4)


def small_cases():
    return [("random", s) for s in RANDOM_SEEDS] + [("hostile", s) for s in HOSTILE_SEEDS + DIRECTED]


def all_cases():
    return small_cases() + [("big", s) for s in BIG_SEEDS]


def case_ids(cases):
    return [f"{k}-{s}" for k, s in cases]


def np_real(rt):
    return np.float64 if rt == A.CR_REAL_F64 else np.float32


def scene_of(kind, seed):
    try:
        return make_scene(kind, seed)
    except ValueError:
        assert kind == "hostile"
        pytest.skip("the mirror's own argument checks reject this scene")


# ------------------------------------------------------------------ comparisons
def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_image(got, want, what):
    """The positions of the NaNs on their own, then the bytes with the NaNs zeroed (tests/test_gpu_aov.py's same, for one array)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: {int((gn != wn).sum())} NaN positions differ, first at {np.argwhere(gn != wn)[:4].tolist()}"
    a, b = bits(np.where(gn, 0, got)), bits(np.where(wn, 0, want))
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def same_words(got, want, what):
    """CR_OUTPUT_FIXED_SUM words: the flags on their own, then the whole words."""
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    gf, wf = (got & FLAG) != 0, (want & FLAG) != 0
    assert np.array_equal(gf, wf), f"{what}: {int((gf != wf).sum())} flags differ, first at {np.argwhere(gf != wf)[:4].tolist()}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {int(got[tuple(bad[0])]):#x} != {int(want[tuple(bad[0])]):#x}")


def bad_mask(frame):
    """The pixels Color::new refuses: a channel that is NaN or outside [0, 1]."""
    with np.errstate(invalid="ignore"):
        return ~((frame >= 0) & (frame <= 1)).all(axis=-1)


# ------------------------------------------------------------------ the oracle's words and the model
class OracleScene:
    """One scene in the oracle, on the tree the device walks (tree / linear_list as Oracle.render_image takes them)."""

    def __init__(self, oracle, sc, flat=None, tree=None, linear_list=False):
        self.oracle, self.cam = oracle, sc.scene_cam
        self.h = oracle.scene_create(flat if flat is not None else sc.flatten())
        if tree is not None:
            oracle.set_tree(self.h, *tree)
        if linear_list:
            oracle.lib.oracle_use_list(self.h)

    def close(self):
        self.oracle.scene_destroy(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def render(self, seed, **kw):
        out, st = self.oracle.render(self.h, self.cam, seed=seed, sum_order=RELAX, **{"n_threads": ORACLE_THREADS, **kw})
        if kw.get("pix_begin") is None and kw.get("pix_end") is None:
            out = out.reshape(self.cam.image_height, self.cam.image_width, 3)
        return out, st

    def pass_words(self, seed, P):
        """The per-pass CR_OUTPUT_FIXED_SUM words of the frame: (samples / P, H, W, 3) uint64, the model's input."""
        return np.stack([self.render(seed, sample_begin=p * P, sample_count=P, output_sum=FIXED)[0] for p in range(self.cam.samples // P)])

    def rows(self, seed, region, **kw):
        """The region's pixels row by row (pix_begin / pix_end): ((h, w, 3) array, summed counters), tests/test_gpu_region.py's oracle_rows."""
        x0, y0, w, h = region
        rows, tot = [], {c: 0 for c in COUNTERS}
        for j in range(h):
            b = (y0 + j) * self.cam.image_width + x0
            out, st = self.render(seed, pix_begin=b, pix_end=b + w, n_threads=1, **kw)
            rows.append(out)
            for c in COUNTERS:
                tot[c] += st[c]
        return np.stack(rows), tot


def pass_words(oracle, sc, seed, P, **kw):
    with OracleScene(oracle, sc, **kw) as o:
        return o.pass_words(seed, P)


def median_tolerance(words, P, min_samples, samples, block):
    """tests/test_gpu_adaptive.py's: the median over blocks of D_b / (2^(S-12) qP 3 N_b) at the first judgement."""
    return float(np.median(np.array(M.first_judgement_ratios(words, P, min_samples, samples, block), dtype=np.float64)))


class Want:
    """What the model makes of a frame's words: counts, frame, the judgements, and the numbers the stats must show."""

    def __init__(self, words, P, min_samples, block, R, tol=None):
        passes, H, W, _ = words.shape
        S = passes * P
        self.tol = median_tolerance(words, P, min_samples, S, block) if tol is None else tol
        self.counts, self.frame, self.decisions = M.adaptive(words, P, min_samples, S, block, self.tol, R)
        self.rects = M.blocks_of(W, H, block)
        self.blocks = len(self.rects)
        self.stopped = sum(1 for x0, y0, _, _ in self.rects if self.counts[y0, x0] < S)
        self.passes = int(self.counts.max()) // P
        self.samples = int(self.counts.sum(dtype=np.int64))
        self.nan_pixels = int(bad_mask(self.frame).sum())
        self.flagged = bool(((words & FLAG) != 0).any())


def variant_model(words, P, min_samples, samples, block, tolerance, R, keep_flag=False, nan_from="run"):
    """The model's loop restated with one rule made wrong.  keep_flag: the judge's term is taken of the accumulators as they
    are, bit 63 included.  nan_from: "run" the flags of the passes the block ran in both halves (the model's), "E" of the even
    passes alone, "all" of every pass of the frame, run or not.  Returns (counts, frame)."""
    _, H, W, _ = words.shape
    S = M.fx_log2(samples)
    flags = (words & FLAG) != 0
    counts = np.zeros((H, W), dtype=np.int32)
    frame = np.zeros((H, W, 3), dtype=R)
    for x0, y0, w, h in M.blocks_of(W, H, block):
        box = (slice(y0, y0 + h), slice(x0, x0 + w))

        def halves(q):
            E, O, _ = M.block_sums(words, q, (x0, y0, w, h))
            fe, fo = flags[(slice(0, 2 * q, 2),) + box].any(axis=0), flags[(slice(1, 2 * q, 2),) + box].any(axis=0)
            return E, O, fe, fo

        q = 0
        while True:
            q += 1
            n = 2 * q * P
            if n >= samples:
                break
            if n < min_samples:
                continue
            E, O, fe, fo = halves(q)
            if keep_flag:
                E, O = E | np.where(fe, FLAG, np.uint64(0)), O | np.where(fo, FLAG, np.uint64(0))
                D = sum(abs(int(e) - int(o)) >> 12 for e, o in zip(E.reshape(-1).tolist(), O.reshape(-1).tolist()))
            else:
                D = M.difference(E, O)
            if D <= M.threshold(tolerance, S, q * P, w * h):
                break
        E, O, fe, fo = halves(q)
        nan = {"run": fe | fo, "E": fe, "all": flags[(slice(None),) + box].any(axis=0)}[nan_from]
        counts[box] = n
        frame[box] = M.finalize(E + O, nan, n, S, R)
    return counts, frame


# ------------------------------------------------------------------ 2. what the inputs contain (CPU)
_WINDOW = {}


def window(oracles, rt, frame):
    """(scene, the oracle's per-pass words) of nan_window_scene(frame) at WINDOW_RUN, computed once and never changed."""
    if (rt, frame) not in _WINDOW:
        samples, P, _ = WINDOW_RUN
        sc = scenes.nan_window_scene(frame, samples=samples)
        words = pass_words(oracles[rt], sc, SEED, P)
        words.setflags(write=False)
        _WINDOW[(rt, frame)] = (sc, words)
    return _WINDOW[(rt, frame)]


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
def test_nan_window_scene_has_the_classes(oracles, rt, tag):
    """nan_window_scene(0) at 16 samples, passes of 2, min_samples 4, block 8 and the median tolerance, from the relaxed oracle's
    words and the model alone.  Measured, identical in f32 and f64: 421 of 1073 pixels carry a flag somewhere in the 16
    samples; the model's counts are 4 / 8 / 12 / 16 on 481 / 104 / 424 / 64 pixels, and blocks holding flagged pixels end at
    all four; 240 pixels of the model's frame are NaN, 113 of them first flagged after min_samples; 181 pixels are flagged
    only in passes their block never ran and come out finite; the median tolerance is 0.10805261297423006 in f64.  Frame 1
    has no flag.  A judge term that keeps bit 63 changes 969 counts, a NaN mask taken from E's flags alone changes 94 pixels
    and no count, flags taken from all 16 samples change 181 pixels.  Asserted as "at least one" of each."""
    samples, P, min_samples = WINDOW_RUN
    R = np_real(rt)
    _, words = window(oracles, rt, 0)
    want = Want(words, P, min_samples, 8, R)
    flags = ((words & FLAG) != 0).any(axis=3)                                  # (passes, H, W)
    ran = (np.arange(samples // P)[:, None, None] * P) < want.counts[None]     # the passes each pixel's block ran
    somewhere, in_run = flags.any(axis=0), (flags & ran).any(axis=0)
    nan = np.isnan(want.frame).any(axis=2)
    assert np.array_equal(nan, in_run) and np.array_equal(np.isnan(want.frame).all(axis=2), nan)   # a flag covers the pixel's three channels here
    assert want.nan_pixels == int(nan.sum()) > 0                               # and nothing finite leaves [0, 1]
    assert sorted(np.unique(want.counts)) == [4, 8, 12, 16]
    for n in (4, 8, 12, 16):
        assert (in_run & (want.counts == n)).any(), n                          # a flagged pixel in a block of every count
    early = (flags & ran)[:min_samples // P].any(axis=0)
    assert (in_run & ~early).any()                                             # first flagged after min_samples
    beyond = somewhere & ~in_run
    assert beyond.any() and np.isfinite(want.frame[beyond]).all()              # flagged only beyond the block's stop: finite
    assert (~somewhere & (want.counts == min_samples)).any() and (~somewhere & (want.counts == samples)).any()
    assert 0 < somewhere.sum() < somewhere.size and ((words & MAG)[:, somewhere] != 0).any()   # flags beside ordinary magnitudes
    # frame 1: no flag at all
    _, words1 = window(oracles, rt, 1)
    assert not ((words1 & FLAG) != 0).any()
    # each wrong rule differs from the model on frame 0
    args = (words, P, min_samples, samples, 8, want.tol, R)
    c, f = variant_model(*args)
    assert np.array_equal(c, want.counts) and bits(f).tobytes() == bits(want.frame).tobytes()   # the restated loop is the model's
    c, _ = variant_model(*args, keep_flag=True)
    assert (c != want.counts).any()
    c, f = variant_model(*args, nan_from="E")
    assert np.array_equal(c, want.counts) and (np.isnan(f).any(axis=2) != nan).any()
    c, f = variant_model(*args, nan_from="all")
    assert np.array_equal(c, want.counts) and (np.isnan(f).any(axis=2) != nan).any()


def test_corpora_give_mixed_decisions(oracles):
    """Every random and hostile case (DIRECTED included) at 12 samples, passes of 2, min_samples 4, block 8 and the median
    tolerance, on the reference tree with its construction-time boxes (an opt-in tree needs the device; with the rota's refit
    90 random pairs instead of 92 take three counts), from the oracle and the model alone.  Measured over the pairs (case,
    precision):

                 pairs   counts {4, 8, 12}   median tolerance 0   one-block frames   rejected by the mirror
        random    168           92                   22                  0                     -
        hostile   120           16                   59                 38                     0

    A tolerance of exactly 0 stops exactly the blocks with D = 0.  The one-block frames are 1x1 to 9x5 pixels.  The seeds of
    FULLY_FLAGGED are flagged in every pixel; 309589 in f32 has one flagged pixel.  The floors below (80 and 12) sit under the
    measured 92 and 16 so that a toolchain moving one ratio does not fail them; they are not to be lowered."""
    S, P, min_samples, block = CORPUS_RUN["random"]
    assert CORPUS_RUN["hostile"] == CORPUS_RUN["random"]
    tally = {k: dict(pairs=0, three=0, zero=0, one_block=0) for k in ("random", "hostile")}
    rejected, fully, partly = set(), set(), set()
    for kind, seed in small_cases():
        for rt, tag in REALS:
            try:
                sc, rseed = make_scene(kind, seed)
            except ValueError:
                assert kind == "hostile"
                rejected.add(seed)
                continue
            sc.scene_cam.set_samples(S)
            words = pass_words(oracles[rt], sc, rseed, P)
            want = Want(words, P, min_samples, block, np_real(rt))
            t = tally[kind]
            t["pairs"] += 1
            t["three"] += sorted(np.unique(want.counts)) == [4, 8, 12]
            t["one_block"] += want.blocks == 1
            if want.tol == 0.0:
                t["zero"] += 1
                for (x0, y0, _, _), log in zip(want.rects, want.decisions):   # T = 0 at every judgement: a block stops exactly when its D is 0
                    assert log and all(T == 0 for _, _, T in log) and all(D > 0 for _, D, _ in log[:-1])
                    assert (want.counts[y0, x0] < S) == (log[-1][1] == 0) and want.counts[y0, x0] in (log[-1][0], S)
            flagged = ((words & FLAG) != 0).any(axis=(0, 3))
            if flagged.all():
                fully.add((seed, tag))
            elif flagged.any():
                partly.add((seed, tag))
    assert not rejected, rejected
    assert tally["random"]["pairs"] == 2 * len(RANDOM_SEEDS) and tally["hostile"]["pairs"] == 2 * len(HOSTILE_SEEDS + DIRECTED), tally
    assert tally["random"]["three"] >= 80 and tally["hostile"]["three"] >= 12, tally
    assert tally["random"]["zero"] > 0 and tally["hostile"]["zero"] > 0 and tally["hostile"]["one_block"] > 0, tally
    assert {(s, t) for s in FULLY_FLAGGED for _, t in REALS} <= fully, fully
    assert partly, "no corpus frame with flags in some pixels only"


# ------------------------------------------------------------------ the calls
def adaptive_kw(rt, seed, tol, P, min_samples, block):
    return dict(seed=seed, real_type=rt, tolerance=tol, min_samples=min_samples, pass_samples=P, block=block, sum_order=RELAX)


def device_adaptive(r, cam, frames=None, **kw):
    """cr_render_adaptive_device (frames: cr_render_adaptive_frames_device) into torch tensors: (images, counts, stats) -- the
    device forms run no Color::new check, so the bytes of a frame with NaN pixels come back."""
    import torch
    n = 1 if frames is None else len(frames)
    H, W = cam.image_height, cam.image_width
    d_img = torch.full((n, H, W, 3), -1.0, dtype=torch.float64 if kw["real_type"] == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    d_cnt = torch.full((n, H, W), -1, dtype=torch.int32, device="cuda:0")
    guard = torch.full((64,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if frames is None:
        st = r.render_adaptive_device(cam, d_img.data_ptr(), d_cnt.data_ptr(), **kw)
    else:
        st = r.render_adaptive_frames_device(cam, frames, d_img.data_ptr(), d_cnt.data_ptr(), **kw)
    r.synchronize()
    assert (guard.cpu().numpy() == -1).all()
    img, cnt = d_img.cpu().numpy(), d_cnt.cpu().numpy()
    return (img[0], cnt[0], st) if frames is None else (img, cnt, st)


def host_adaptive(lib, r, cam, frames=None, *, seed, real_type, tolerance, min_samples, pass_samples, block, sum_order):
    """cr_render_adaptive_host (frames: cr_render_adaptive_frames_host) through ctypes with buffers of its own:
    (status, cr_last_error's text, stats).  The header promises nothing about the buffers after an error: they are dropped."""
    cd, p = cam.desc(), cam.params(seed, real_type, 0, None, False, sum_order)
    ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
    n = 1 if frames is None else len(frames)
    out = np.empty((n, cam.image_height, cam.image_width, 3), dtype=np_real(real_type))
    cnt = np.empty((n, cam.image_height, cam.image_width), dtype=np.int32)
    st = A.CrAdaptiveStats()
    if frames is None:
        rc = lib.cr_render_adaptive_host(r.h, C.byref(cd), C.byref(p), C.byref(ap), out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                         C.byref(st))
    else:
        rc = lib.cr_render_adaptive_frames_host(r.h, C.byref(cd), C.byref(p), C.byref(ap), (C.c_int32 * n)(*frames), n,
                                                out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(st))
    return rc, (lib.cr_last_error(r.h) or b"").decode() if rc != A.CR_OK else "", st.as_dict()


def host_region(lib, r, cam, region, *, seed, real_type):
    """cr_render_region_host's mean form through ctypes with a buffer of its own: (status, cr_last_error's text, stats)."""
    cd, p = cam.desc(), cam.params(seed, real_type, 0, None, False, RELAX)
    out = np.empty((region[3], region[2], 3), dtype=np_real(real_type))
    st = A.CrStats()
    rc = lib.cr_render_region_host(r.h, C.byref(cd), C.byref(p), C.byref(A.CrRegion(*region)), out.ctypes.data_as(C.c_void_p), C.byref(st))
    return rc, (lib.cr_last_error(r.h) or b"").decode() if rc != A.CR_OK else "", st.as_dict()


def device_region(r, cam, region, *, seed, real_type):
    """cr_render_region_device's mean form into a torch tensor: ((h, w, 3) array, stats)."""
    import torch
    d = torch.full((region[3], region[2], 3), -1.0, dtype=torch.float64 if real_type == A.CR_REAL_F64 else torch.float32, device="cuda:0")
    guard = torch.full((64,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = r.render_region_device(cam, region, d.data_ptr(), seed=seed, real_type=real_type, sum_order=RELAX, want_stats=True)
    r.synchronize()
    assert (guard.cpu().numpy() == -1).all()
    return d.cpu().numpy(), st


def check_adaptive_stats(st, want, P, nan_pixels=None, passes=None):
    assert st["blocks"] == want.blocks and st["blocks_stopped"] == want.stopped, (st, want.blocks, want.stopped)
    assert st["passes"] == (want.passes if passes is None else passes), (st["passes"], want.passes, passes)
    assert st["render"]["samples"] == want.samples, (st["render"]["samples"], want.samples)
    if nan_pixels is not None:
        assert st["render"]["nan_pixels"] == nan_pixels, (st["render"]["nan_pixels"], nan_pixels)


def check_host_status(rc, msg, st, nan_pixels, what):
    """CR_ERR_NAN exactly when the model's frame has a pixel that is NaN or outside [0, 1]; nan_pixels is their number."""
    assert rc == (A.CR_ERR_NAN if nan_pixels else A.CR_OK), (what, rc, msg, nan_pixels)
    assert st["nan_pixels"] == nan_pixels, (what, st["nan_pixels"], nan_pixels)
    if nan_pixels:
        assert NAN_MESSAGE in msg, (what, msg)


def block_counters(r, cam, want, rt, seed):
    """What each block took, from the region-and-shard renders (tests/test_gpu_adaptive.py's check_mixed): its pixels, the
    samples [0, n_b).  As words, which come back without the Color::new check."""
    tot = {c: 0 for c in COUNTERS}
    for x0, y0, w, h in want.rects:
        _, rst = r.render_region(cam, (x0, y0, w, h), seed=seed, real_type=rt, sum_order=RELAX, sample_begin=0,
                                 sample_count=int(want.counts[y0, x0]), output_sum=FIXED)
        for c in COUNTERS:
            tot[c] += rst[c]
    return tot


# ------------------------------------------------------------------ 3(a). adaptive renders of the corpora
def uploaded(renderer, sc, seed, rt):
    """Upload by the rota of the seed: (flat scene, the oracle's tree arguments)."""
    variant = set_variant(sc, seed)
    flat = sc.flatten()
    renderer.upload_scene(flat)
    kw = {}
    if variant == 2:
        tree = renderer.export_bvh(rt)
        kw = dict(linear_list=True) if len(tree[1]) == 0 else dict(tree=tree)
    return flat, kw


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("kind,seed", all_cases(), ids=case_ids(all_cases()))
def test_adaptive_on_the_corpora(renderer, hiplib, oracles, kind, seed, rt, tag):
    """One corpus scene by the rota of its seed, adaptively at CORPUS_RUN and the median tolerance: the device form's counts
    and frame are the model's; the host form's status, nan_pixels, samples, blocks, blocks_stopped and passes are the model's;
    a frame without flags has the work counters of the region-and-shard renders its blocks took."""
    sc, rseed = scene_of(kind, seed)
    S, P, min_samples, block = CORPUS_RUN[kind]
    cam = sc.scene_cam
    cam.set_samples(S)
    flat, okw = uploaded(renderer, sc, seed, rt)
    words = pass_words(oracles[rt], sc, rseed, P, flat=flat, **okw)
    want = Want(words, P, min_samples, block, np_real(rt))
    kw = adaptive_kw(rt, rseed, want.tol, P, min_samples, block)
    what = f"{kind} {seed}"
    img, counts, st = device_adaptive(renderer, cam, **kw)
    assert np.array_equal(counts, want.counts), f"{what}: {int((counts != want.counts).sum())} counts differ"
    same_image(img, want.frame, what)
    check_adaptive_stats(st, want, P)
    rc, msg, hst = host_adaptive(hiplib, renderer, cam, **kw)
    check_host_status(rc, msg, hst["render"], want.nan_pixels, what)
    check_adaptive_stats(hst, want, P, nan_pixels=want.nan_pixels)
    if not want.flagged:
        tot = block_counters(renderer, cam, want, rt, rseed)
        for c in COUNTERS:
            assert st["render"][c] == hst["render"][c] == tot[c], (what, c, st["render"][c], hst["render"][c], tot[c])


# ------------------------------------------------------------------ 3(b). the frame with partial flags
def plain_finalized(r, cam, rt, n):
    """The plain relaxed render of the frame at samples = n, as words (no Color::new check) through the Python finalize."""
    keep = cam.samples
    cam.set_samples(n)
    try:
        words, _ = r.render(cam, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED)
    finally:
        cam.set_samples(keep)
    return M.finalize(words & MAG, (words & FLAG) != 0, n, M.fx_log2(n), np_real(rt))


def check_window(r, lib, oracles, rt, block):
    samples, P, min_samples = WINDOW_RUN
    R = np_real(rt)
    sc, words = window(oracles, rt, 0)
    cam = sc.scene_cam
    want = Want(words, P, min_samples, block, R)
    # block 8: counts 4 / 8 / 12 / 16 and 240 NaN pixels; block 16: counts 4 / 8 and 175 NaN pixels
    assert 0 < want.nan_pixels < cam.image_width * cam.image_height and len(np.unique(want.counts)) >= (4 if block == 8 else 2)
    if block == 8:
        assert want.nan_pixels == 240
    r.upload_scene(sc.flatten())
    kw = adaptive_kw(rt, SEED, want.tol, P, min_samples, block)
    img, counts, st = device_adaptive(r, cam, **kw)
    assert np.array_equal(counts, want.counts), f"{int((counts != want.counts).sum())} counts differ"
    same_image(img, want.frame, "frame 0")
    check_adaptive_stats(st, want, P)
    for n in np.unique(counts):   # every pixel, the NaN ones too, is the pixel of the plain render with its own count
        ref = plain_finalized(r, cam, rt, int(n))
        same_image(img[counts == n], ref[counts == n], f"pixels that took {n} samples")
    rc, msg, hst = host_adaptive(lib, r, cam, **kw)
    assert rc == A.CR_ERR_NAN and "frame" not in msg
    check_host_status(rc, msg, hst["render"], want.nan_pixels, "frame 0")
    check_adaptive_stats(hst, want, P, nan_pixels=want.nan_pixels)
    # an error leaves no state behind: frame 1 on the same handle, no flag anywhere
    sc1, words1 = window(oracles, rt, 1)
    want1 = Want(words1, P, min_samples, block, R, tol=want.tol)
    assert want1.nan_pixels == 0
    r.upload_scene(sc1.flatten())
    rc, msg, hst = host_adaptive(lib, r, sc1.scene_cam, **kw)
    check_host_status(rc, msg, hst["render"], 0, "frame 1")
    check_adaptive_stats(hst, want1, P, nan_pixels=0)
    img1, counts1, _ = r.render_adaptive(sc1.scene_cam, **kw)
    assert np.array_equal(counts1, want1.counts) and not np.isnan(img1).any()
    same_image(img1, want1.frame, "frame 1")
    return st


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("where", ["block8", "block16", "global-memory"])
def test_adaptive_nan_window(renderer, hiplib, oracles, monkeypatch, where, rt, tag):
    """nan_window_scene(0): counts, frame bytes and NaN mask are the model's; every pixel equals the plain relaxed
    CR_OUTPUT_FIXED_SUM render at samples = counts[pixel]; the host form answers CR_ERR_NAN with the model's nan_pixels (240 at
    block 8), and the next call on the handle renders frame 1 with CR_OK and the model's bytes.  global-memory: a handle
    whose scene stays out of LDS, so that the global-memory listed kernel sees flags."""
    if where != "global-memory":
        check_window(renderer, hiplib, oracles, rt, 8 if where == "block8" else 16)
        return
    monkeypatch.setenv("CRUCIBLE_LDS_LIMIT", "0")
    monkeypatch.setenv("CRUCIBLE_LDS_TOP_KB", "0")
    r = Renderer(0)
    try:
        st = check_window(r, hiplib, oracles, rt, 8)
        assert st["render"]["scene_in_lds"] == 0
    finally:
        r.close()


# ------------------------------------------------------------------ 3(c). batches: flags stay in their frame
# 37 x 29 pixels in a pass of 2 samples: work tiles of 8 x 4 pixels x 2 samples, 5 x 8 of them, 64 work items each
WINDOW_FRAME_ITEMS = 5 * 8 * 64


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("frames,first,split", [([0, 1], 0, False), ([1, 0], 1, False), ([1, 0, 0, 1], 1, False), ([0, 1], 0, True)],
                         ids=["0-1", "1-0", "1-0-0-1", "0-1-one-frame-per-loop"])
def test_adaptive_batches_keep_flags_in_their_frame(renderer, hiplib, oracles, monkeypatch, frames, first, split, rt, tag):
    """Frames 0 (partial flags) and 1 (none) of nan_window_scene in one batch: the device form equals the single calls and the
    model frame for frame, frame 1's slices hold no NaN; the host form answers CR_ERR_NAN, nan_pixels the sum over the entries,
    and names frame 0 at its first entry.  split: CRUCIBLE_WORK_COUNTER_MAX leaves one frame per pass loop."""
    samples, P, min_samples = WINDOW_RUN
    block, R = 8, np_real(rt)
    sc, words0 = window(oracles, rt, 0)
    _, words1 = window(oracles, rt, 1)
    want0 = Want(words0, P, min_samples, block, R)
    want = {0: want0, 1: Want(words1, P, min_samples, block, R, tol=want0.tol)}
    assert want[0].nan_pixels > 0 and want[1].nan_pixels == 0 and not np.isnan(want[1].frame).any()
    kw = adaptive_kw(rt, SEED, want0.tol, P, min_samples, block)
    r = renderer
    if split:
        monkeypatch.setenv("CRUCIBLE_WORK_COUNTER_MAX", str(WINDOW_FRAME_ITEMS))
        r = Renderer(0)
        monkeypatch.delenv("CRUCIBLE_WORK_COUNTER_MAX")
    try:
        cam = sc.scene_cam
        r.upload_scene(sc.flatten())
        singles = {}
        for f in (0, 1):
            cam.frame = f
            singles[f] = device_adaptive(r, cam, **kw)
        cam.frame = 12345   # params->frame is ignored
        imgs, counts, st = device_adaptive(r, cam, frames, **kw)
        for k, f in enumerate(frames):
            what = f"{frames} frame {f} (entry {k})"
            assert np.array_equal(counts[k], singles[f][1]) and np.array_equal(counts[k], want[f].counts), what
            same_image(imgs[k], singles[f][0], what + " against the single call")
            same_image(imgs[k], want[f].frame, what + " against the model")
            assert np.isnan(imgs[k]).any() == (f == 0), what
        loops = [frames[k:k + 1] for k in range(len(frames))] if split else [frames]
        passes = sum(max(want[f].passes for f in loop) for loop in loops)
        for got in (st, None):
            if got is None:
                rc, msg, got = host_adaptive(hiplib, r, cam, frames, **kw)
                assert rc == A.CR_ERR_NAN and got["render"]["nan_pixels"] == sum(want[f].nan_pixels for f in frames), (rc, msg, got)
                assert f"frame 0 (entry {first} of the batch): " + NAN_MESSAGE in msg, msg
                assert frames.index(0) == first
            assert got["passes"] == passes, (got["passes"], passes)
            assert got["blocks"] == sum(want[f].blocks for f in frames) and got["blocks_stopped"] == sum(want[f].stopped for f in frames)
            assert got["render"]["samples"] == sum(want[f].samples for f in frames)
        # the handle is usable, and a batch without frame 0 is clean
        rc, msg, got = host_adaptive(hiplib, r, cam, [1, 1], **kw)
        assert rc == A.CR_OK and got["render"]["nan_pixels"] == 0, (rc, msg)
    finally:
        sc.scene_cam.frame = 0
        if split:
            r.close()


# ------------------------------------------------------------------ 3(d), (e). regions
def regions_of(W, H):
    """(regions, partition): tests/test_gpu_region.py's partition moved into the W x H frame, empty rectangles dropped, plus
    the last pixel and the whole frame.  A 1 x 1 frame is its one region."""
    if (W, H) == (1, 1):
        return [(0, 0, 1, 1)], [(0, 0, 1, 1)]
    part = [reg for reg in scaled(PARTITION, W, H) if reg[2] > 0 and reg[3] > 0]
    assert sum(w * h for _, _, w, h in part) == W * H
    return part + [reg for reg in scaled(EXTRA, W, H) if reg not in part], part


def check_regions(r, lib, o, cam, rseed, rt, regions, partition, what):
    """Per region: the words are the crop of the oracle's relaxed words, flags included; the device's mean form is the crop of
    the oracle's relaxed frame; the counters are the oracle's for those rows; the host's mean form answers CR_ERR_NAN exactly
    when the oracle's pixels inside the region fail Color::new, nan_pixels their number, in a message that names no frame.
    Over the partition the counters add up to the whole frame's.  Returns (the oracle's words, its frame)."""
    W, H, S = cam.image_width, cam.image_height, cam.samples
    words, wst = o.render(rseed, output_sum=FIXED)
    frame, fst = o.render(rseed)
    bad = bad_mask(frame)
    assert fst["nan_pixels"] == int(bad.sum())
    tot = {c: 0 for c in COUNTERS + ("samples",)}
    for reg in regions:
        tag = f"{what} region {reg}"
        got, st = r.render_region(cam, reg, seed=rseed, real_type=rt, sum_order=RELAX, output_sum=FIXED)
        same_words(got, crop(words, reg), tag)
        mean, mst = device_region(r, cam, reg, seed=rseed, real_type=rt)
        same_image(mean, crop(frame, reg), tag)
        _, ost = o.rows(rseed, reg)
        for c in COUNTERS:
            assert st[c] == mst[c] == ost[c], (tag, c, st[c], mst[c], ost[c])
        assert st["samples"] == mst["samples"] == reg[2] * reg[3] * S
        n_bad = int(crop(bad, reg).sum())
        rc, msg, hst = host_region(lib, r, cam, reg, seed=rseed, real_type=rt)
        check_host_status(rc, msg, hst, n_bad, tag)
        assert "frame" not in msg and "entry" not in msg, msg
        if reg in partition:
            for c in tot:
                tot[c] += st[c]
        if reg == (0, 0, W, H):
            for c in COUNTERS:
                assert st[c] == wst[c] == fst[c], (tag, c)
    if partition:
        _, full = r.render_region(cam, (0, 0, W, H), seed=rseed, real_type=rt, sum_order=RELAX, output_sum=FIXED)
        for c in tot:
            assert tot[c] == full[c] and (c == "samples" or full[c] == fst[c]), (what, c, tot[c], full[c])
    return words, frame


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("kind,seed", small_cases(), ids=case_ids(small_cases()))
def test_regions_on_the_corpora(renderer, hiplib, oracles, kind, seed, rt, tag):
    sc, rseed = scene_of(kind, seed)
    cam = sc.scene_cam
    flat, okw = uploaded(renderer, sc, seed, rt)
    regions, part = regions_of(cam.image_width, cam.image_height)
    with OracleScene(oracles[rt], sc, flat=flat, **okw) as o:
        check_regions(renderer, hiplib, o, cam, rseed, rt, regions, part, f"{kind} {seed}")


def clean_region(bad):
    """The largest rectangle (x0, y0, w, h) without a pixel of the mask `bad`, or None."""
    H, W = bad.shape
    best = None
    for y0 in range(H):
        ok = np.ones(W, dtype=bool)
        for y1 in range(y0, H):
            ok &= ~bad[y1]
            run = x0 = 0
            for x in range(W + 1):
                if x < W and ok[x]:
                    run += 1
                    continue
                if run and (best is None or run * (y1 - y0 + 1) > best[2] * best[3]):
                    best = (x0, y0, run, y1 - y0 + 1)
                run, x0 = 0, x + 1
    return best


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
def test_regions_of_the_nan_window(renderer, hiplib, oracles, rt, tag):
    """test_regions_on_the_corpora's checks on nan_window_scene(0) at 16 samples, whose regions hold flagged and ordinary
    pixels side by side; a region chosen from the oracle's mask to hold no flagged pixel answers CR_OK with nan_pixels 0; the
    words of the shards [0, 6) and [6, 16) of a region combine, by the header's rule, to the region's whole words."""
    sc, pw = window(oracles, rt, 0)
    cam = sc.scene_cam
    renderer.upload_scene(sc.flatten())
    regions, part = regions_of(cam.image_width, cam.image_height)
    with OracleScene(oracles[rt], sc) as o:
        words, frame = check_regions(renderer, hiplib, o, cam, SEED, rt, regions, part, "nan window")
        flagged = ((words & FLAG) != 0).any(axis=2)
        assert np.array_equal(flagged, ((pw & FLAG) != 0).any(axis=(0, 3))) and np.array_equal(flagged, bad_mask(frame))
        mixed = [reg for reg in part if 0 < crop(flagged, reg).sum() < reg[2] * reg[3]]
        assert mixed
        clean = clean_region(flagged)
        assert clean is not None and clean[2] * clean[3] >= 16 and not crop(flagged, clean).any()
        check_regions(renderer, hiplib, o, cam, SEED, rt, [clean], [], "nan window, clean")
        rc, msg, hst = host_region(hiplib, renderer, cam, clean, seed=SEED, real_type=rt)
        assert rc == A.CR_OK and hst["nan_pixels"] == 0, (rc, msg)
        reg = max(mixed, key=lambda g: g[2] * g[3])
        head, tail = combine(combine(pw[0], pw[1]), pw[2]), combine(combine(combine(pw[3], pw[4]), combine(pw[5], pw[6])), pw[7])
        assert (crop((head ^ tail) & FLAG, reg) != 0).any()   # a flag in one shard only
        a, ast = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED, sample_begin=0, sample_count=6)
        b, bst = renderer.render_region(cam, reg, seed=SEED, real_type=rt, sum_order=RELAX, output_sum=FIXED, sample_begin=6, sample_count=10)
        same_words(a, crop(head, reg), "shard [0, 6)")
        same_words(b, crop(tail, reg), "shard [6, 16)")
        same_words(combine(a, b), crop(words, reg), "shards [0, 6) and [6, 16) combined")
        assert ast["samples"] == reg[2] * reg[3] * 6 and bst["samples"] == reg[2] * reg[3] * 10


# ------------------------------------------------------------------ 3(f). guide regions of the hostile corpus
def hostile_cases():
    return [("hostile", s) for s in HOSTILE_SEEDS + DIRECTED]


@gpu
@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("kind,seed", hostile_cases(), ids=case_ids(hostile_cases()))
def test_guide_regions_on_the_hostile_corpus(renderer, oracles, kind, seed, rt, tag):
    """cr_render_aov_region_* over the partition of every hostile scene: each plane is the crop of the model's plane (the
    positions of the NaNs on their own, then the bytes); the counters of the partition add up to the whole frame's."""
    sc, rseed = scene_of(kind, seed)
    cam = sc.scene_cam
    _, okw = uploaded(renderer, sc, seed, rt)
    W, H = cam.image_width, cam.image_height
    regions, part = regions_of(W, H)
    want, _ = model(oracles[rt], sc, rseed, **okw)
    tot = {c: 0 for c in COUNTERS + ("samples",)}
    for reg in regions:
        got, st = renderer.render_aov_region(cam, reg, seed=rseed, real_type=rt)
        same_planes(got, {n: crop(want[n], reg) for n in NAMES}, f"{kind} {seed} region {reg}")
        assert st["samples"] == reg[2] * reg[3] * cam.samples == st["segments"] and st["nan_pixels"] == 0
        if reg in part:
            for c in tot:
                tot[c] += st[c]
    _, full = renderer.render_aov(cam, seed=rseed, real_type=rt)
    for c in tot:
        assert tot[c] == full[c], (kind, seed, c, tot[c], full[c])
