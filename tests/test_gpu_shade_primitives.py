"""What a path does around the walk, on the device, one function at a time (tests/shade_check.hip runs the functions of
crucible_amd/csrc/pathtrace.hpp and refit.hpp; tests/shade_corpus.py makes the inputs):
  (a) shade() after a closest hit -- every material, checker and image textures, the reference-order attenuation record and
      the relaxed throughput, texel reads -- against oracle_world_hit + oracle_scatter with the same RNG key, draw for draw,
      including degenerate triangles (a normal that is not a number), the total-internal-reflection threshold +-1 ulp,
      dot(ud, n) below -1, the Lambertian 1e-8 tolerance (dir = n) and RNG keys on the Schlick and scatter_prob thresholds;
  (b) shade() after a miss, both skies, with an empty stack and with five levels to unwind (and the relaxed thr of five
      factors), against oracle_sky and the oracle's Color products;
  (c) the texture a hit reads (CR_CHECKER_LEAF, image_lookup) against oracle_texture_value;
  (d) camera_ray (static, keyed and defocused cameras, every kernel variant) against oracle_camera_ray;
  (e) timeline_eval / timeline_vertex against oracle_timeline_eval;
  (f) the refit box: it contains the primitive at every time the walk can see (ground truth from oracle_timeline_eval), and
      it is exactly the rule's union of sample boxes grown by timeline_pad.
All bit for bit, in f64 and f32.  Renders almost never land on texel edges, key starts or the uv seam; these inputs do."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_corpus as S  # noqa: E402
from crucible_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "crucible_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "shade_check.hip")
SEED = 0x5EED5
HIT_WORDS, HIT_VARIANTS = 18, 4
VARIANTS = ("ANIM", "ANIM+RELAX", "static", "static+RELAX")


def build_shade_check(exe):
    subprocess.run(HIPCC + ["-o", str(exe), SRC], check=True, timeout=600)


def full_desc():
    """The one scene every part reads: the shading scene plus the animated primitives of the refit and timeline parts."""
    d = S.shade_desc()
    S.anim_desc(d)
    d.anim_prims += [i for i, _, _, _ in d.hit_prims if d.prims[i].key_count > 0]
    return d


def hexrow(row):
    return " ".join(float(v).hex() for v in np.asarray(row, dtype=np.float64).ravel())


def first_bad(ok, rows, names, what, extra=None):
    """Assertion message for the first row where `ok` is false."""
    bad = np.flatnonzero(~np.asarray(ok))
    if len(bad) == 0:
        return ""
    i = bad[0]
    msg = f"{what}: {len(bad)} mismatches; first in group {names[i]}: row {hexrow(rows[i])}"
    if extra is not None:
        msg += "; " + extra(i)
    return msg


def same_bits(a, b):
    """Equal bit for bit, or both not a number."""
    a, b = np.asarray(a), np.asarray(b)
    it = np.uint64 if a.dtype == np.float64 else np.uint32
    return (a.view(it) == b.view(it)) | (np.isnan(a) & np.isnan(b))


def rows_ok(got, ref):
    """Per row (first axis): every value the same bits, or both not a number."""
    return same_bits(got, ref).reshape(len(got), -1).all(axis=1)


def row_ok(got, ref):
    return bool(same_bits(got, ref).all())


# ------------------------------------------------------------------ oracle references
def oracle_hits(o, d, flat, rays):
    """For every ray: the oracle's closest hit (t, material) at the ray's time, or t = -1."""
    sc = o.scene_create(flat)
    out = np.zeros(10, dtype=o.np_real)
    mat = C.c_int32()
    res = []
    try:
        for i, g, ro, rd, tm, _ in rays:
            ro_, rd_ = o.arr(ro), o.arr(rd)
            hit = o.lib.oracle_world_hit(sc, o._p(ro_), o._p(rd_), o.real(tm), o.real(0.001), o.real(np.inf), o._p(out), C.byref(mat))
            res.append((float(out[0]), mat.value) if hit else (-1.0, -1))
    finally:
        o.scene_destroy(sc)
    return res


def hit_cases(d, flat, o64, o32):
    """hit.in rows (prim, t64, t32, ro, rd, rtime, pixel, sample) for rays whose closest hit, in either precision, is the
    primitive they aim at, each with several RNG keys."""
    rays = S.hit_rays(d)
    h64, h32 = oracle_hits(o64, d, flat, rays), oracle_hits(o32, d, flat, rays)
    rows, names = [], []
    rs = np.random.RandomState(17)
    for (i, g, ro, rd, tm, keys), (t64, m64), (t32, m32) in zip(rays, h64, h32):
        want = d.prims[i].material
        t64 = t64 if m64 == want else -1.0
        t32 = t32 if m32 == want else -1.0
        if t64 < 0 and t32 < 0:
            continue
        for pixel, sample in list(keys) + [(rs.randint(0, 1 << 20), rs.randint(0, 64)) for _ in range(6)]:
            rows.append([i, t64, t32] + list(ro) + list(rd) + [tm, pixel, sample])
            names.append(g + ("/threshold_key" if (pixel, sample) in keys else ""))
    return np.array(rows, dtype=np.float64), np.array(names)


def scatter_ref(o, sc, row, mat):
    """oracle_scatter for one hit.in row in o's precision: (some, att[3], origin[3], dir[3], draws) or None (no hit)."""
    t = row[1] if o.np_real == np.float64 else row[2]
    if t < 0:
        return None
    ro, rd = o.arr(row[3:6]), o.arr(row[6:9])
    rec = np.zeros(10, dtype=o.np_real)
    m = C.c_int32()
    assert o.lib.oracle_world_hit(sc, o._p(ro), o._p(rd), o.real(row[9]), o.real(0.001), o.real(np.inf), o._p(rec), C.byref(m))
    assert m.value == mat
    out = np.zeros(10, dtype=o.np_real)
    some = o.lib.oracle_scatter(sc, m.value, o._p(ro), o._p(rd), o._p(rec), C.c_uint64(SEED), C.c_uint32(int(row[10])),
                                C.c_uint32(int(row[11])), o._p(out))
    return bool(some), out[0:3].copy(), out[3:6].copy(), out[6:9].copy(), float(out[9])


@pytest.fixture(scope="module")
def shade(tmp_path_factory, o64, o32):
    """One run of shade_check on every part's inputs."""
    dd = tmp_path_factory.mktemp("shade_check")
    exe = dd / "shade_check"
    build_shade_check(exe)
    d = full_desc()
    flat = d.flat()
    d.write(dd / "scene.bin")
    np.array([SEED], dtype=np.uint64).tofile(dd / "seed.in")
    STACK.astype(np.float64).tofile(dd / "stack.in")
    hit, hit_names = hit_cases(d, flat, o64, o32)
    hit.tofile(dd / "hit.in")
    sky, sky_names = S.sky_rows()
    sky.tofile(dd / "sky.in")
    tex, tex_names = S.texture_rows(d)
    tex.tofile(dd / "texture.in")
    cams = S.cameras()
    S.write_cameras(dd / "camera.in", cams, A.CR_REAL_F64)
    tl, tl_names = S.timeline_rows(d)
    tl.tofile(dd / "timeline.in")
    rf, rf_names = S.refit_rows(d)
    rf.tofile(dd / "refit.in")
    r = subprocess.run([str(exe), str(dd)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(part, sfx, words):
        return np.fromfile(dd / f"{part}{sfx}.out", dtype=np.float64).reshape(-1, *words)

    res = {"desc": d, "flat": flat, "hit": hit, "hit_names": hit_names, "sky": sky, "sky_names": sky_names, "tex": tex,
           "tex_names": tex_names, "cams": cams, "tl": tl, "tl_names": tl_names, "rf": rf, "rf_names": rf_names}
    for sfx in ("64", "32"):
        res["hit" + sfx] = load("hit", sfx, (HIT_VARIANTS, HIT_WORDS))
        res["sky" + sfx] = load("sky", sfx, (2, 4, 4))
        res["texture" + sfx] = load("texture", sfx, (4,))
        res["camera" + sfx] = load("camera", sfx, (3, 8))
        res["timeline" + sfx] = load("timeline", sfx, (9,))
        res["refit" + sfx] = load("refit", sfx, (6,))
    return res


PRECISIONS = (("64", np.float64), ("32", np.float32))


# attenuations of the stacked misses (tests/shade_check.hip stack.in); the first is also the relaxed hits' starting thr
STACK = np.array([[0.7, 0.3, 0.9], [0.55, 0.8, 0.45], [0.9, 0.65, 0.35], [0.6, 0.95, 0.75], [0.85, 0.4, 0.5]])


def texel_reads(d, ti):
    """Texel reads of a lookup that starts at texture ti: 1 when every leaf below it is an image, 0 when none is."""
    t = d.texs[ti]
    if t.kind == A.CR_TEX_CHECKER:
        even, odd = texel_reads(d, t.even), texel_reads(d, t.odd)
        return even if even == odd else None
    return int(t.kind == A.CR_TEX_IMAGE)


def hit_mismatches(d, rows, out, o, sc, dt):
    """(per-row failure messages, cases checked, cases absorbed) of the hit part against oracle_scatter, in o's precision."""
    bad, checked, finished = {}, 0, 0
    thr0 = STACK[0].astype(dt)
    for r, row in enumerate(rows):
        i = int(row[0])
        ref = scatter_ref(o, sc, row, d.prims[i].material)
        if ref is None:
            continue
        some, att, org, dirn, draws = ref
        mat = d.mats[d.prims[i].material]
        want_tex = texel_reads(d, mat.texture) if mat.kind == A.CR_MAT_LAMBERTIAN else 0
        for v in range(HIT_VARIANTS if d.prims[i].key_count == 0 else 2):
            w = out[r, v]
            relax = v % 2 == 1
            got = w.astype(dt)
            ok = w[16] == draws and bool(w[0]) == (not some) and (want_tex is None or w[15] == want_tex)
            if not some:   # absorbed: black, nothing pushed, depth unchanged
                ok &= row_ok(got[1:4], np.zeros(3, dt)) and w[10] == 10 and (relax or w[14] == 0)
            else:
                ok &= row_ok(got[4:7], org) and row_ok(got[7:10], dirn) and w[10] == 9
                if mat.kind == A.CR_MAT_DIELECTRIC:   # attenuation (1, 1, 1): not stored, thr unchanged
                    ok &= row_ok(got[11:14], thr0) if relax else (w[14] == 0)
                else:   # the pushed record, or thr = thr0 * att
                    ok &= row_ok(got[11:14], thr0 * att) if relax else (row_ok(got[11:14], att) and w[14] == 1)
            if not ok and r not in bad:
                bad[r] = (f"variant {VARIANTS[v]}: device {hexrow(w)}; oracle some {some} att {hexrow(att)} origin {hexrow(org)} "
                          f"dir {hexrow(dirn)} draws {draws}, texel reads {want_tex}")
            checked += 1
        finished += not some
    return bad, checked, finished


@pytest.mark.gpu
def test_shade_after_a_hit_matches_the_oracle_scatter(shade, o64, o32):
    d, rows, names = shade["desc"], shade["hit"], shade["hit_names"]
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        sc = o.scene_create(shade["flat"])
        try:
            bad, checked, finished = hit_mismatches(d, rows, shade["hit" + sfx], o, sc, dt)
        finally:
            o.scene_destroy(sc)
        ok = ~np.isin(np.arange(len(rows)), list(bad))
        assert ok.all(), first_bad(ok, rows, names, f"shade hit ({dt.__name__})", lambda i: bad[i])
        print(f"\n[shade (a)] {dt.__name__}: {checked} (case, variant) pairs, {finished} cases absorbed, 0 mismatches")
        assert checked > 2000 and finished > 20, (checked, finished)


def _rng_u64(o, pixel, sample, n):
    out = np.zeros(n, dtype=np.uint64)
    o.lib.oracle_rng_u64(C.c_uint64(SEED), C.c_uint32(pixel), C.c_uint32(sample), n, out.ctypes.data_as(C.c_void_p))
    return out


def test_hit_corpus_reaches_its_edges(o64, o32):
    """The edge groups of the hit corpus sit where they claim to: threshold keys on their draws (the oracle's own stream),
    TIR rays on ri * sin_theta = 1 and +-1 ulp, the tolerance rays on dir = n, degenerate triangles hit with a normal that
    is not a number, and head-on sphere hits with dot(ud, n) below -1."""
    d = full_desc()
    flat = d.flat()
    rows, names = hit_cases(d, flat, o64, o32)
    u24 = lambda u: float(int(u) >> 40) * 2.0 ** -24  # noqa: E731   the f32 uniform of a draw
    for pixel, sample in S.R0_KEYS:   # first draw between r0(1/2.4) and r0(2.4), both f32
        r0 = lambda ri: ((np.float32(1) - ri) / (np.float32(1) + ri)) ** 2  # noqa: E731
        lo, hi = sorted((r0(np.float32(1) / np.float32(2.4)), r0(np.float32(2.4))))
        assert lo <= u24(_rng_u64(o32, pixel, sample, 1)[0]) < hi, (pixel, sample)
    for pixel, sample in S.HALF_KEYS:   # fourth draw exactly 0.5
        assert u24(_rng_u64(o32, pixel, sample, 4)[3]) == 0.5, (pixel, sample)
    for pixel, sample in S.TOLERANCE_KEYS_F32:   # third draw: z = -1 + 2 u = -0.5
        assert u24(_rng_u64(o32, pixel, sample, 3)[2]) == 0.25, (pixel, sample)
    reached = {np.float64: set(), np.float32: set()}
    for i, rd, param, dt, target in d.tir_rows:
        prod, _ = S.dielectric_terms(rd, S.TIR_E1, S.TIR_E2, param, dt)
        assert prod == dt(target), (rd, param, dt, prod, target)
        reached[dt].add(float(target))
    assert reached[np.float32] == {float(np.nextafter(np.float32(1), np.float32(0))), 1.0, float(np.nextafter(np.float32(1), np.float32(2)))}
    assert {1.0, float(np.nextafter(1.0, 2.0))} <= reached[np.float64]
    for o, col, dt in ((o64, 1, np.float64), (o32, 2, np.float32)):
        sc = o.scene_create(flat)
        try:
            tol = deg = below = tir = 0
            for row, g in zip(rows, names):
                if row[col] < 0:
                    continue
                ro, rd = o.arr(row[3:6]), o.arr(row[6:9])
                rec = np.zeros(10, dtype=o.np_real)
                m = C.c_int32()
                o.lib.oracle_world_hit(sc, o._p(ro), o._p(rd), o.real(row[9]), o.real(0.001), o.real(np.inf), o._p(rec), C.byref(m))
                if g.startswith(f"lambert_tolerance/{dt.__name__}/threshold_key"):
                    ref = scatter_ref(o, sc, row, m.value)
                    assert row_ok(ref[3], rec[4:7]), (g, ref[3], rec[4:7])   # scattered along n itself
                    tol += 1
                elif g.endswith("triangle_degenerate"):
                    assert np.isnan(rec[4:7]).all(), rec
                    deg += 1
                elif g.endswith(f"tir_threshold/{dt.__name__}"):
                    tir += 1
                elif "dielectric" in g and g.endswith("sphere/head_on"):
                    p = d.prims[int(row[0])]
                    below += S.sphere_dot(ro, rd, o.np_real(row[col]), np.array(p.v[:3]), p.v[3], dt) < -1
        finally:
            o.scene_destroy(sc)
        print(f"\n[shade edges] {dt.__name__}: {tol} tolerance hits, {deg} degenerate-triangle hits, {tir} TIR-threshold hits, "
              f"{below} head-on hits with dot(ud, n) < -1")
        assert tol >= 2 and deg >= 5 and tir >= 2 and below >= 5, (dt, tol, deg, tir, below)


@pytest.mark.gpu
def test_shade_after_a_miss_matches_the_oracle_sky(shade, o64, o32):
    rows, names = shade["sky"], shade["sky_names"]
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        out = shade["sky" + sfx]
        st = STACK.astype(dt)
        thr = st[0].copy()
        for k in range(1, len(st)):
            thr = thr * st[k]   # the relaxed throughput: a_1 * a_2 * ... in path order
        for kind in (A.CR_SKY_DEFAULT, A.CR_SKY_SPHERICAL):
            sc = o.scene_create(shade["desc"].flat(sky_kind=kind))
            try:
                sky = np.array([_sky(o, sc, r) for r in rows])
                unwound = sky.copy()
                for k in range(len(st) - 1, -1, -1):   # a_1 * (a_2 * (... (a_5 * sky))), Color's clamped products
                    for r in range(len(rows)):
                        unwound[r] = o.vec_fn("oracle_color_mul", st[k], unwound[r])
            finally:
                o.scene_destroy(sc)
            for v, what, ref in ((0, "reference order", sky), (1, "relaxed", sky), (2, "reference order, 5 levels", unwound),
                                 (3, "relaxed, thr of 5 levels", thr * sky)):
                got = out[:, kind, v, :3].astype(dt)
                ok = rows_ok(got, ref)
                assert ok.all(), first_bad(ok, rows, names, f"sky kind {kind} ({dt.__name__}, {what})",
                                           lambda i: f"device {hexrow(got[i])} oracle {hexrow(ref[i])}")
                assert (out[:, kind, v, 3] == (kind == A.CR_SKY_SPHERICAL)).all(), "one texel read per spherical-sky miss, none for the gradient"
    print(f"\n[shade (b)] {len(rows)} directions x 2 skies x 4 stacks x 2 precisions, 0 mismatches")


def _sky(o, sc, d):
    out = np.zeros(3, dtype=o.np_real)
    dv = o.arr(d)
    o.lib.oracle_sky(sc, o._p(dv), o._p(out))
    return out


@pytest.mark.gpu
def test_texture_lookup_matches_the_oracle(shade, o64, o32):
    rows, names = shade["tex"], shade["tex_names"]
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        got = shade["texture" + sfx][:, :3].astype(dt)
        sc = o.scene_create(shade["flat"])
        ref = np.zeros((len(rows), 3), dtype=dt)
        try:
            for r, row in enumerate(rows):
                p = o.arr(row[3:6])
                with np.errstate(over="ignore"):
                    o.lib.oracle_texture_value(sc, int(row[0]), o.real(row[1]), o.real(row[2]), o._p(p), o._p(ref[r]))
        finally:
            o.scene_destroy(sc)
        ok = rows_ok(got, ref)
        assert ok.all(), first_bad(ok, rows, names, f"texture ({dt.__name__}) vs oracle_texture_value",
                                   lambda i: f"device {hexrow(got[i])} oracle {hexrow(ref[i])}")
        reads = shade["texture" + sfx][:, 3]
        want = np.array([texel_reads(shade["desc"], int(r[0])) for r in rows])
        ok = reads == want
        assert ok.all(), first_bad(ok, rows, names, f"texel reads ({dt.__name__})", lambda i: f"device {reads[i]} expected {want[i]}")
    print(f"\n[shade (c)] {len(rows)} lookups x 2 precisions, 0 mismatches")


@pytest.mark.gpu
def test_camera_ray_matches_the_oracle(shade, o64, o32):
    cams = shade["cams"]
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        out = shade["camera" + sfx]
        k = 0
        for name, dsc, fk, ak, prm, ijs in cams:
            p = prm(o.real_type)
            for i, j, s in ijs:
                ref = np.zeros(8, dtype=o.np_real)
                o.lib.oracle_camera_ray(C.byref(dsc), C.byref(p), i, j, s, o._p(ref))
                for v in range(3 if not (fk or ak) else 2):
                    got = out[k, v].astype(dt)
                    ok = row_ok(got[:7], ref[:7]) and out[k, v, 7] == ref[7]
                    assert ok, (f"camera_ray ({dt.__name__}) vs oracle_camera_ray: camera {name}, pixel ({i}, {j}) sample {s}, "
                                f"variant {('ANIM', 'CAMK', 'static')[v]}: device {hexrow(got)} oracle {hexrow(ref)}")
                k += 1
        assert k == len(out)
    print(f"\n[shade (d)] {len(cams)} cameras, {len(out)} samples x 2 precisions, 0 mismatches")


def timeline_ref(o, d, rows):
    ref = np.zeros((len(rows), 9), dtype=o.np_real)
    for r, row in enumerate(rows):
        v = S.eval_prim(o, d, int(row[0]), o.np_real(row[1])).ravel()
        ref[r, :len(v)] = v
    return ref


def check_timeline(d, rows, names, out_by_precision, o64, o32):
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        got = out_by_precision[sfx].astype(dt)
        ref = timeline_ref(o, d, rows)
        ok = rows_ok(got, ref)
        assert ok.all(), first_bad(ok, rows, names, f"timeline ({dt.__name__}) vs oracle_timeline_eval",
                                   lambda i: f"device {hexrow(got[i])} oracle {hexrow(ref[i])}")


def check_refit(d, rows, names, out_by_precision, o64, o32, n_uniform):
    """Containment against the ground truth and equality with the rule, both precisions."""
    for (sfx, dt), o in zip(PRECISIONS, (o64, o32)):
        boxes = out_by_precision[sfx]
        bad = S.refit_ground_truth_violations(o, d, rows, names, boxes, n_uniform)
        ok = ~np.isin(np.arange(len(rows)), [b[0] for b in bad])
        assert not bad, first_bad(ok, rows, names, f"refit box ({dt.__name__}) too small",
                                  lambda i: f"box {hexrow(boxes[i])}; at t {float(bad[0][1]).hex()} the primitive spans "
                                            f"{hexrow(bad[0][2])} .. {hexrow(bad[0][3])}")
        col = 1 if dt == np.float64 else 3
        ref = np.array([np.concatenate(S.rule_box(o, d, int(r[0]), dt(r[col]), dt(r[col + 1]))) for r in rows])
        got = boxes.astype(dt)
        ok = rows_ok(got, ref)
        assert ok.all(), first_bad(ok, rows, names, f"refit box ({dt.__name__}) vs the rule's sample union + timeline_pad",
                                   lambda i: f"device {hexrow(got[i])} rule {hexrow(ref[i])}")


@pytest.mark.gpu
def test_timeline_matches_the_oracle(shade, o64, o32):
    check_timeline(shade["desc"], shade["tl"], shade["tl_names"], {s: shade["timeline" + s] for s in ("64", "32")}, o64, o32)
    print(f"\n[shade (e)] {len(shade['tl'])} evaluations x 2 precisions, 0 mismatches")


@pytest.mark.gpu
def test_refit_box_contains_the_primitive_and_is_the_rule(shade, o64, o32):
    check_refit(shade["desc"], shade["rf"], shade["rf_names"], {s: shade["refit" + s] for s in ("64", "32")}, o64, o32, 100)
    print(f"\n[shade (f)] {len(shade['rf'])} intervals x 2 precisions: contained at every walk time, equal to the rule")
