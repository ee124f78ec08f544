"""Inputs of tests/shade_check.hip, aimed at the edges where the device code around the walk can differ from the oracle:
texel edges and the v flip, nested checkers on integer multiples of 1/inv_scale and beyond 2^31, the sphere-uv seam and the
poles, every material branch, the two skies, corner pixels and keyed cameras, key starts and ends +-1 ulp, and refit
intervals that start or end on a key.  Every case carries a group name, so that a failure names its group.

The scene is a plain list of C-ABI descriptors (include/crucible_hip.h); Desc.flat() hands it to the oracle and
Desc.write() to the check program, which packs it with the library's own functions (crucible_amd/csrc/pack.hpp)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crucible_amd import _abi as A  # noqa: E402
from crucible_amd.scene import FlatScene  # noqa: E402

TX, TY, TZ, RAD, SX, SY, SZ = range(7)
NERP, LERP = 0, 1


def ulp_shift(x, k):
    """x moved k ulps (k may be negative), elementwise, in x's own precision."""
    x = np.asarray(x)
    out = x.copy()
    for _ in range(abs(int(k))):
        out = np.nextafter(out, np.array(np.inf if k > 0 else -np.inf, dtype=x.dtype))
    return out


def key(ch, t0, t1, a, b=0.0, interp=LERP):
    return A.CrKeyframe(ch, interp, t0, t1, a, b)


class Desc:
    """A scene as C-ABI descriptors, with the group name of every primitive."""

    def __init__(self):
        self.prims, self.mats, self.texs, self.keys, self.images = [], [], [], [], []
        self.groups = []
        self.sky_kind, self.sky_image = A.CR_SKY_DEFAULT, -1

    def image(self, rgb8):
        self.images.append(np.ascontiguousarray(rgb8, dtype=np.uint8))
        return len(self.images) - 1

    def tex(self, kind, even=-1, odd=-1, image=-1, color=(0, 0, 0), inv_scale=0.0):
        self.texs.append(A.CrTexture(kind, even, odd, image, (C.c_double * 3)(*color), inv_scale))
        return len(self.texs) - 1

    def mat(self, kind, texture=-1, albedo=(0, 0, 0), param=0.0):
        self.mats.append(A.CrMaterial(kind, texture, (C.c_double * 3)(*albedo), param))
        return len(self.mats) - 1

    def prim(self, kind, g, mat, keys=(), group=""):
        v = (C.c_double * 9)(*(list(g) + [0.0] * (9 - len(g))))
        self.prims.append(A.CrPrimitive(kind, mat, 0, len(self.keys), len(keys), 0, v))
        self.keys.extend(keys)
        self.groups.append(group)
        return len(self.prims) - 1

    def sphere(self, c, r, mat, keys=(), group=""):
        return self.prim(A.CR_PRIM_SPHERE, list(c) + [r], mat, keys, group)

    def triangle(self, a, b, c, mat, keys=(), group=""):
        return self.prim(A.CR_PRIM_TRIANGLE, list(a) + list(b) + list(c), mat, keys, group)

    def prim_keys(self, i):
        p = self.prims[i]
        return self.keys[p.key_first:p.key_first + p.key_count]

    def flat(self, sky_kind=None):
        return FlatScene(self.prims, self.mats, self.texs, self.images, self.keys, self.sky_kind if sky_kind is None else sky_kind,
                         self.sky_image)

    def write(self, path):
        """scene.bin of shade_check.hip."""
        hdr = np.array([len(self.prims), len(self.mats), len(self.texs), len(self.images), len(self.keys), self.sky_kind,
                        self.sky_image], dtype=np.int32)
        parts = [hdr.tobytes()]
        for arr, T in ((self.prims, A.CrPrimitive), (self.mats, A.CrMaterial), (self.texs, A.CrTexture), (self.keys, A.CrKeyframe)):
            if arr:
                parts.append(bytes((T * len(arr))(*arr)))
        for im in self.images:
            parts.append(np.array([im.shape[1], im.shape[0]], dtype=np.int32).tobytes() + im.tobytes())
        with open(path, "wb") as f:
            f.write(b"".join(parts))


# ------------------------------------------------------------------ timelines and refit
def _key_sets():
    """(group, is_sphere, keys) -- the key lists of the animated primitives."""
    out = []
    # one translate key per channel, LERP and NERP, positive and negative
    for ch in (TX, TY, TZ):
        for interp in (LERP, NERP):
            for a in (2.5, -3.25):
                out.append(("single_key", True, [key(ch, 0.25, 0.75, a, interp=interp)]))
                out.append(("single_key", False, [key(ch, 0.25, 0.75, a, interp=interp)]))
    # zero-length keys (t0 = t1): a jump at t0, 0/0 at the instant itself
    for interp in (LERP, NERP):
        out.append(("zero_length", True, [key(TX, 0.5, 0.5, 1.5, interp=interp)]))
        out.append(("zero_length", False, [key(TY, 0.5, 0.5, -1.5, interp=interp), key(TX, 0.25, 0.75, 1.0)]))
    # several keys on one channel, overlapping, with opposite signs: the rounded sum of a rising and a falling term
    out.append(("opposite_signs", True, [key(TX, 0.0, 1.0, 1.0), key(TX, 0.0, 1.0, -1.0)]))
    out.append(("opposite_signs", True, [key(TX, 0.1, 0.9, 0.7), key(TX, 0.3, 1.1, -0.7)]))
    out.append(("opposite_signs", False, [key(TY, 0.0, 1.0, 0.3), key(TY, 0.0, 1.0, -0.1), key(TY, 0.2, 0.6, -0.2)]))
    out.append(("opposite_signs", True, [key(TZ, 0.0, 1.0, 1e-3), key(TZ, 0.0, 1.0, -1e-3 * (1 + 2 ** -40))]))
    out.append(("opposite_signs", False, [key(TX, 0.0, 1.0, 3.0), key(TX, 0.0, 1.0, -3.0), key(TX, 0.5, 0.5, 1.0)]))
    # a sphere moving one way while its radius shrinks at the same rate: centre + radius is constant in exact arithmetic
    out.append(("move_and_shrink", True, [key(TX, 0.0, 1.0, 1.0), key(RAD, 0.0, 1.0, 2.0, 1.0)]))
    out.append(("move_and_shrink", True, [key(TY, 0.0, 1.0, -0.3), key(RAD, 0.0, 1.0, 0.5, 0.8)]))
    out.append(("move_and_shrink", True, [key(TX, 0.0, 1.0, 0.1), key(TX, 0.0, 1.0, 0.2), key(RAD, 0.0, 1.0, 1.0, 0.7)]))
    # radius keys: the last active one wins, before the first and after the last key
    out.append(("radius", True, [key(RAD, 0.2, 0.4, 1.0, 2.0), key(RAD, 0.6, 0.8, 3.0, 0.5)]))
    out.append(("radius", True, [key(RAD, 0.2, 0.4, 1.0, 2.0, NERP), key(RAD, 0.3, 0.5, 0.25, 0.5)]))
    out.append(("radius", True, [key(RAD, 0.5, 0.5, 2.0, 3.0)]))
    # triangle scales: ScaleX / Y / Z, the last active one winning, with and without translate keys (the bilinear branch)
    for ch in (SX, SY, SZ):
        out.append(("scale_xyz", False, [key(ch, 0.2, 0.8, 1.0, 2.0)]))
        out.append(("scale_xyz", False, [key(TX, 0.0, 1.0, 2.0), key(TY, 0.1, 0.6, -1.0), key(ch, 0.2, 0.8, 1.0, -1.5)]))
        out.append(("scale_xyz", False, [key(TX, 0.0, 1.0, -2.0), key(ch, 0.0, 1.0, 0.5, 1.5), key(SZ, 0.5, 0.7, 2.0, 0.5, NERP)]))
    out.append(("scale_xyz", False, [key(TX, 0.3, 0.3, 1.0), key(SX, 0.3, 0.3, 2.0, 3.0), key(SY, 0.1, 0.9, -1.0, 1.0)]))
    # extremes only a key end or a left limit reaches: a channel that rises until one key ends while another falls on,
    # and one that rises into a NERP key's start, where it jumps back
    for is_sphere in (True, False):
        out.append(("key_end_extreme", is_sphere, [key(TX, 0.0, 0.6, 1.0), key(TX, 0.2, 1.0, -1.0)]))
        out.append(("key_end_extreme", is_sphere, [key(TY, 0.1, 0.45, -0.5), key(TY, 0.0, 0.9, 0.75), key(TZ, 0.3, 0.7, 0.2)]))
        out.append(("left_limit_extreme", is_sphere, [key(TX, 0.0, 1.0, 1.0), key(TX, 0.5, 1.0, -2.0, interp=NERP)]))
        out.append(("left_limit_extreme", is_sphere, [key(TZ, 0.0, 1.0, -1.0), key(TZ, 0.25, 0.25, 3.0, interp=NERP)]))
    out.append(("left_limit_extreme", True, [key(RAD, 0.0, 1.0, 1.0, 2.0), key(RAD, 0.5, 1.0, 0.5, 0.5, NERP)]))
    out.append(("left_limit_extreme", False, [key(SX, 0.0, 1.0, 1.0, 2.0), key(SX, 0.5, 1.0, 0.5, 0.5, NERP)]))
    out.append(("key_end_extreme", False, [key(TX, 0.0, 0.6, 1.0), key(TX, 0.2, 1.0, -1.0), key(SY, 0.0, 1.0, 1.0, 1.5)]))
    # times before the first key and after the last; many keys
    ks = [key(TX + (i % 3), 0.05 * i, 0.05 * i + 0.1, (-1.0) ** i * 0.3 * (i + 1), interp=i % 2) for i in range(12)]
    out.append(("many_keys", True, ks))
    out.append(("many_keys", False, ks + [key(SY, 0.4, 0.6, 0.5, 2.0)]))
    return out


def anim_desc(d=None):
    """Animated primitives added to d (or a new scene): every key set on a sphere or a triangle whose box crosses zero, and on
    a far one.  d.anim_prims lists them."""
    d = Desc() if d is None else d
    m = d.mat(A.CR_MAT_METAL, albedo=(0.5, 0.5, 0.5), param=0.0)
    d.anim_prims = []
    for group, is_sphere, ks in _key_sets():
        if is_sphere:
            d.anim_prims.append(d.sphere((0.25, -0.5, 0.125), 0.75, m, ks, group))
            d.anim_prims.append(d.sphere((1e3 + 0.1, 3.0, -7.0), 0.3, m, ks, group + "_far"))
        else:
            d.anim_prims.append(d.triangle((-0.5, -0.25, 0.5), (0.75, 0.3, -0.2), (0.1, 0.9, 0.05), m, ks, group))
            d.anim_prims.append(d.triangle((1e3 + 0.3, 2.0, 5.0), (1e3 - 0.7, 2.5, 5.5), (1e3, 1.0, 4.5), m, ks, group + "_far"))
    return d


def frame_interval(frame, rate, angle, dt):
    """[current_time, current_time + shutter_length] as the library computes it in dt (ray_casting.rs:77-79)."""
    one = dt(1)
    ct = dt(frame) * (one / dt(rate))
    sl = (dt(angle) / dt(360)) * (one / dt(rate))
    return ct, ct + sl, ct, sl


def key_times(ks):
    return sorted({k.t0 for k in ks} | {k.t1 for k in ks})


def refit_rows(d):
    """(rows, names): prim, ta64, tb64, ta32, tb32.  Intervals on every key t0 / t1 (exactly and +-1 ulp), spanning
    several keys, of zero length (shutter 0), and from frame times in each precision."""
    rows, names = [], []
    for i in d.anim_prims:
        g = d.groups[i]
        ts = key_times(d.prim_keys(i))
        pairs = [(-1.0, 2.0), (0.0, 1.0), (0.5, 0.5), (0.3, 0.3), (-5.0, -4.0), (4.0, 5.0)]
        for t in ts:
            for u in (t, float(ulp_shift(np.float64(t), -1)), float(ulp_shift(np.float64(t), 1))):
                pairs += [(u, u), (u, u + 0.05), (u - 0.05, u), (u, 1.5), (-0.5, u)]
        for a, b in zip(ts, ts[1:]):
            pairs.append((a, b))
        for ta, tb in pairs:
            rows.append([i, ta, tb, np.float32(ta), np.float32(tb)])
            names.append(g)
        for frame, rate, angle in ((0, 4, 180.0), (1, 4, 360.0), (3, 8, 90.0), (1, 2, 0.0), (7, 24, 180.0), (2, 4, 360.0)):
            ta64, tb64, _, _ = frame_interval(frame, rate, angle, np.float64)
            ta32, tb32, _, _ = frame_interval(frame, rate, angle, np.float32)
            rows.append([i, ta64, tb64, ta32, tb32])
            names.append(g + "_frame")
    return np.array(rows, dtype=np.float64), np.array(names)


def timeline_rows(d):
    """(rows, names): prim, t -- every key t0 / t1 and +-1..2 ulp (f64 and f32 ulps), before the first and after the last."""
    rows, names = [], []
    for i in d.anim_prims:
        g = d.groups[i]
        ts = [-1.0, 0.0, 0.4, 0.55, 0.9, 2.0]
        for t in key_times(d.prim_keys(i)):
            ts.append(t)
            for k in (-2, -1, 1, 2):
                ts.append(float(ulp_shift(np.float64(t), k)))
                ts.append(float(ulp_shift(np.float32(t), k)))
        for t in ts:
            rows.append([i, t])
            names.append(g)
    return np.array(rows, dtype=np.float64), np.array(names)


# ---- references for the refit rule, from oracle_timeline_eval
def eval_prim(o, d, i, t, keys=None):
    """The primitive at time t as the hit test sees it (oracle_timeline_eval): sphere (c, r) -> 4 values; triangle -> 3x3."""
    p = d.prims[i]
    ks = d.prim_keys(i) if keys is None else keys
    karr = (A.CrKeyframe * max(1, len(ks)))(*ks)
    out = np.zeros(4, dtype=o.np_real)
    R = o.real
    if p.kind == A.CR_PRIM_SPHERE:
        init = o.arr([p.v[0], p.v[1], p.v[2], p.v[3]])
        o.lib.oracle_timeline_eval(o._p(init), karr, len(ks), 1, R(t), o._p(out))
        return out.copy()
    vs = []
    for j in range(3):
        init = o.arr([p.v[3 * j], p.v[3 * j + 1], p.v[3 * j + 2], 1.0])
        o.lib.oracle_timeline_eval(o._p(init), karr, len(ks), 0, R(t), o._p(out))
        vs.append(out[:3].copy())
    return np.array(vs)


def box_of(p_kind, v, dt):
    """Sphere::new's box (c + (-r), c + r, ordered) or the triangle's vertex min / max (f64::min/max: NaN ignored)."""
    if p_kind == A.CR_PRIM_SPHERE:
        c, r = v[:3].astype(dt), dt(v[3])
        lo_, hi_ = c + (-r), c + r
        return np.where(lo_ <= hi_, lo_, hi_), np.where(lo_ <= hi_, hi_, lo_)
    v = v.astype(dt)
    return np.fmin(np.fmin(v[0], v[1]), v[2]), np.fmax(np.fmax(v[0], v[1]), v[2])


def walk_times(ks, ta, tb, dt, n_uniform=2000, seed=0):
    """Times the walk can see in [ta, tb], in dt: ta, tb, every key t0 / t1 inside and its +-1..4-ulp neighbours, the
    largest ray time ta + (tb - ta) * u can produce, and uniform times."""
    ta, tb = dt(ta), dt(tb)
    umax = dt(1) - (dt(2.0 ** -53) if dt == np.float64 else dt(2.0 ** -24))
    ts = [ta, tb, ta + (tb - ta) * umax]
    for k in ks:
        for t in (dt(k.t0), dt(k.t1)):
            for s in range(-4, 5):
                ts.append(ulp_shift(t, s))
    rs = np.random.RandomState(seed)
    u = rs.random_sample(n_uniform).astype(dt)
    ts.extend(list(ta + (tb - ta) * u))
    ts = np.array(ts, dtype=dt)
    return np.unique(ts[(ts >= ta) & (ts <= tb)])


def rule_samples(ks, ta, tb):
    """The refit rule's sample times (refit.hpp refit_sample): (t, before_start) pairs."""
    out = [(ta, False), (tb, False)]
    for k in ks:
        t0, t1 = type(ta)(k.t0), type(ta)(k.t1)
        if ta < t0 <= tb:
            out += [(t0, False), (t0, True)]
        if ta < t1 < tb:
            out.append((t1, False))
    return out


def _without_starting(ks, t, dt):
    """The key list with the keys that start exactly at t left out: the left limit at a key start."""
    return [k for k in ks if not (dt(k.t0) == t and not (t > dt(k.t1)))]


def _right_limit(ks, t, dt):
    """The key list with every zero-length key at t completed: its value just after t (s = 1), as a NERP key."""
    out = []
    for k in ks:
        if dt(k.t0) == t and dt(k.t1) == t:
            a = dt(k.a)
            if k.channel >= RAD and k.interp == LERP:
                a = a + (dt(k.b) - a) * dt(1)
            k = key(k.channel, k.t0, k.t1, float(a), float(a), NERP)
        out.append(k)
    return out


def _side(ks, t, before_start, dt):
    return _without_starting(ks, t, dt) if before_start else _right_limit(ks, t, dt)


def timeline_pad(d, i, dt):
    """refit.hpp timeline_pad, written out: B * (4 n + 32) * 2^-p, or 0 when no key moves anything."""
    p = d.prims[i]
    ks = d.prim_keys(i)
    g = dt(0)
    for x in (p.v[:4] if p.kind == A.CR_PRIM_SPHERE else p.v[:9]):
        g = max(g, abs(dt(x)))
    tr, v = dt(0), dt(1)
    for k in ks:
        if k.channel <= TZ:
            tr = dt(tr + abs(dt(k.a)))
        else:
            v = max(v, abs(dt(k.a)), abs(dt(k.b)))
    if not any(k.interp == LERP and (dt(k.a) != 0 if k.channel <= TZ else dt(k.a) != dt(k.b)) for k in ks):
        return dt(0)   # no key moves anything
    b = dt((g + tr) + v) if p.kind == A.CR_PRIM_SPHERE else dt((v + dt(1)) * (g + tr))
    eps = dt(2.0 ** -53) if dt == np.float64 else dt(2.0 ** -24)
    with np.errstate(over="ignore"):
        pad = dt(b * dt(dt(4 * len(ks) + 32) * eps))
    return pad if pad == pad else dt(np.inf)


def rule_box(o, d, i, ta, tb):
    """The rule's box over [ta, tb] from oracle_timeline_eval at its sample times (NaN sample boxes are not united), each
    sample taken as its one-sided limit, grown by timeline_pad when the primitive has keys."""
    dt = o.np_real
    p = d.prims[i]
    ks = d.prim_keys(i)
    lo, hi = np.full(3, np.inf, dt), np.full(3, -np.inf, dt)
    scaled = any(k.channel >= SX for k in ks)

    def unite(blo, bhi):
        nonlocal lo, hi
        if np.isnan(blo).any() or np.isnan(bhi).any():
            return
        lo, hi = np.where(lo <= blo, lo, blo), np.where(hi >= bhi, hi, bhi)

    samples = rule_samples(ks, dt(ta), dt(tb))
    if not ks:
        unite(*box_of(p.kind, eval_prim(o, d, i, dt(ta)), dt))
        return lo, hi

    def padded():
        if not lo[0] <= hi[0]:
            return lo, hi
        pad = timeline_pad(d, i, dt)
        with np.errstate(invalid="ignore"):
            return lo - pad, hi + pad

    if not scaled:
        for t, bs in samples:
            unite(*box_of(p.kind, eval_prim(o, d, i, t, _side(ks, t, bs, dt)), dt))
        return padded()
    # translate part at t1, scale part at t2, every pair (refit.hpp prim_box_at2)
    tr_keys = [k for k in ks if k.channel <= TZ]
    sc_keys = [k for k in ks if k.channel >= SX]
    for t1, b1 in samples:
        trans = eval_prim(o, d, i, t1, _side(tr_keys, t1, b1, dt))   # 3x3, unit scale
        for t2, b2 in samples:
            kind, v = scale_at(o, _side(sc_keys, t2, b2, dt), t2)
            unite(*box_of(p.kind, apply_scale(kind, v, trans, dt), dt))
    return padded()


def scale_at(o, sc_keys, t):
    """(channel of the winning scale key or -1, its value) at t, the value from oracle_timeline_eval on the point (1, 0, 1)."""
    dt = o.np_real
    t = dt(t)
    kind = -1
    for k in sc_keys:
        if t > dt(k.t1) or (dt(k.t0) <= t <= dt(k.t1)):
            kind = k.channel
    if kind < 0:
        return -1, dt(1)
    karr = (A.CrKeyframe * max(1, len(sc_keys)))(*sc_keys)
    out = np.zeros(4, dtype=dt)
    init = o.arr([1.0, 0.0, 1.0, 1.0])
    o.lib.oracle_timeline_eval(o._p(init), karr, len(sc_keys), 0, o.real(t), o._p(out))
    return kind, {SX: out[0], SY: out[1], SZ: out[2]}[kind]


def apply_scale(kind, v, pts, dt):
    """scale_point on each vertex (include/crucible_hip.h: ScaleX (v*x, y, z), ScaleY (x, v*x + y, z), ScaleZ (x, y, v*z))."""
    out = pts.astype(dt).copy()
    v = dt(v)
    for j in range(3):
        x, y, z = out[j]
        if kind == SX:
            out[j] = (v * x, y, z)
        elif kind == SY:
            out[j] = (x, v * x + y, z)
        elif kind == SZ:
            out[j] = (x, y, v * z)
        else:
            out[j] = (v * x, v * y, v * z)
    return out


def refit_ground_truth_violations(o, d, rows, names, boxes, n_uniform=400):
    """Rows whose box misses the primitive at some time the walk can see: list of (row, t, truth lo, truth hi)."""
    dt = o.np_real
    col = 1 if dt == np.float64 else 3
    bad = []
    for r, row in enumerate(rows):
        i = int(row[0])
        ta, tb = dt(row[col]), dt(row[col + 1])
        lo, hi = boxes[r, :3].astype(dt), boxes[r, 3:].astype(dt)
        ks = d.prim_keys(i)
        for t in walk_times(ks, ta, tb, dt, n_uniform, seed=r):
            blo, bhi = box_of(d.prims[i].kind, eval_prim(o, d, i, t), dt)
            if np.isnan(blo).any() or np.isnan(bhi).any():
                continue
            if (blo < lo).any() or (bhi > hi).any():
                bad.append((r, t, blo, bhi))
                break
    return bad


# ------------------------------------------------------------------ textures, materials, hits, sky
def _rgb(rs, h, w):
    return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)


ENV_W, ENV_H = 33, 17


def shade_desc(seed=11):
    """Images of 1x1, 1xN, Nx1, odd and environment-map sizes; solid, image and nested checker textures (up to
    CR_MAX_CHECKER_DEPTH levels); every material branch on a static and a keyed sphere and triangle, each primitive with a
    material of its own (the oracle's closest hit names the material, which then names the primitive)."""
    rs = np.random.RandomState(seed)
    d = Desc()
    imgs = {"1x1": d.image(_rgb(rs, 1, 1)), "1x7": d.image(_rgb(rs, 7, 1)), "5x1": d.image(_rgb(rs, 1, 5)),
            "7x5": d.image(_rgb(rs, 5, 7)), "env": d.image(_rgb(rs, ENV_H, ENV_W))}
    d.sky_kind, d.sky_image = A.CR_SKY_SPHERICAL, imgs["env"]
    texs = {}
    solid_a = d.tex(A.CR_TEX_SOLID, color=(0.25, 0.5, 0.75))
    solid_b = d.tex(A.CR_TEX_SOLID, color=(0.9, 0.1, 0.3))
    for name, im in imgs.items():
        texs["image_" + name] = d.tex(A.CR_TEX_IMAGE, image=im)
    for inv in (1.0, 3.0, 1.0 / 0.3, 1e-3, 2.0 ** 20):
        texs[f"checker_{inv:g}"] = d.tex(A.CR_TEX_CHECKER, even=solid_a, odd=solid_b, inv_scale=inv)
    texs["checker_images"] = d.tex(A.CR_TEX_CHECKER, even=texs["image_7x5"], odd=texs["image_1x7"], inv_scale=2.0)
    t = solid_a
    for k in range(32):   # a chain of CR_MAX_CHECKER_DEPTH checker levels, alternating scales
        t = d.tex(A.CR_TEX_CHECKER, even=t if k % 2 == 0 else solid_b, odd=solid_b if k % 2 == 0 else t,
                  inv_scale=(1.0, 0.5, 2.0, 1.0 / 3.0)[k % 4])
    texs["checker_depth32"] = t
    d.tex_names = texs
    d.tex_mats = {name: d.mat(A.CR_MAT_LAMBERTIAN, texture=ti, param=1.0) for name, ti in texs.items()}   # puts them on the device
    # materials of the hit cases: (group, kind, texture, albedo, param)
    mats = [("lambert_solid_p1", A.CR_MAT_LAMBERTIAN, solid_a, (0, 0, 0), 1.0),
            ("lambert_solid_p05", A.CR_MAT_LAMBERTIAN, solid_b, (0, 0, 0), 0.5),
            ("lambert_solid_p0", A.CR_MAT_LAMBERTIAN, solid_a, (0, 0, 0), 0.0),
            ("lambert_solid_neg", A.CR_MAT_LAMBERTIAN, solid_b, (0, 0, 0), -0.5),
            ("lambert_checker", A.CR_MAT_LAMBERTIAN, texs["checker_3"], (0, 0, 0), 0.8),
            ("lambert_checker_images", A.CR_MAT_LAMBERTIAN, texs["checker_images"], (0, 0, 0), 1.0),
            ("lambert_image", A.CR_MAT_LAMBERTIAN, texs["image_7x5"], (0, 0, 0), 1.0),
            ("lambert_image_env", A.CR_MAT_LAMBERTIAN, texs["image_env"], (0, 0, 0), 0.7),
            ("lambert_checker_depth32", A.CR_MAT_LAMBERTIAN, texs["checker_depth32"], (0, 0, 0), 1.0),
            ("metal_fuzz0", A.CR_MAT_METAL, -1, (0.8, 0.6, 0.2), 0.0),
            ("metal_fuzz03", A.CR_MAT_METAL, -1, (0.5, 0.5, 0.5), 0.3),
            ("metal_fuzz15", A.CR_MAT_METAL, -1, (0.9, 0.9, 0.9), 1.5),
            ("dielectric_15", A.CR_MAT_DIELECTRIC, -1, (1, 1, 1), 1.5),
            ("dielectric_1", A.CR_MAT_DIELECTRIC, -1, (1, 1, 1), 1.0),
            ("dielectric_07", A.CR_MAT_DIELECTRIC, -1, (1, 1, 1), 1.0 / 1.4),
            ("dielectric_24", A.CR_MAT_DIELECTRIC, -1, (1, 1, 1), 2.4)]
    d.hit_prims = []   # (prim, group, centre, size, is_sphere)
    x = 0.0
    for g, kind, tex, alb, param in mats:
        for geo in ("sphere", "sphere_keyed", "triangle", "triangle_keyed"):
            m = d.mat(kind, texture=tex, albedo=alb, param=param)
            c = np.array([x, 0.5, -1.0])
            ks = ()
            if geo == "sphere_keyed":
                ks = (key(TX, 0.0, 1.0, 0.5), key(TY, 0.25, 0.75, -0.25, interp=NERP), key(RAD, 0.0, 1.0, 1.0, 0.75))
            elif geo == "triangle_keyed":
                ks = (key(TZ, 0.0, 1.0, 0.5), key(SY, 0.2, 0.8, 1.0, 1.5))
            if geo.startswith("sphere"):
                i = d.sphere(c, 1.0, m, ks, g + "/" + geo)
            else:
                i = d.triangle(c + (-1.0, -1.0, 0.0), c + (1.0, -1.0, 0.0), c + (0.0, 1.0, 0.1), m, ks, g + "/" + geo)
            d.hit_prims.append((i, g + "/" + geo, c, geo.startswith("sphere")))
            x += 10.0
    d.special_rays = []
    x = _degenerate_triangles(d, x, mats)
    x = _tir_threshold(d, x)
    _lambert_tolerance(d, x, solid_a)
    return d


def _unit(v, dt):
    """unit() in dt: v * (1 / sqrt(x*x + y*y + z*z)) (pathtrace.hpp divs)."""
    v = np.asarray(v, dtype=dt)
    return v * (dt(1) / np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]))[..., None]


def sphere_dot(ro, rd, t, c, r, dt):
    """dot(unit(rd), n) of a static sphere's hit as shade() computes it in dt: loc = ro + t rd, n = (1/r) (loc - c), turned
    to face the ray."""
    ro, rd, c = (np.asarray(v, dtype=dt) for v in (ro, rd, c))
    n = (dt(1) / dt(r)) * ((ro + dt(t) * rd) - c)
    if not _dot(rd, n) < 0:
        n = -n
    return _dot(_unit(rd, dt), n)


def _degenerate_triangles(d, x, mats):
    """Collinear vertices: the hit test can still report a hit (det rounds past epsilon), and the normal is 0/0."""
    rs = np.random.RandomState(23)
    k = 0
    for g, kind, tex, alb, param in mats:
        if g not in ("lambert_solid_p05", "lambert_image", "metal_fuzz03", "dielectric_15", "dielectric_07"):
            continue
        a, e = np.array([-50.0 - 60.0 * k, 0.0, 0.0]), np.array([12.0, 20.0, 28.0])   # away from the rest of the scene
        k += 1
        i = d.triangle(a, a + e, a + 2 * e, d.mat(kind, texture=tex, albedo=alb, param=param), (), g + "/triangle_degenerate")
        for _ in range(800):   # 1-5 % of them hit
            tgt = a + e * rs.uniform(0, 2)
            ro = tgt + rs.normal(size=3)
            d.special_rays.append((i, g + "/triangle_degenerate", ro, tgt - ro, 0.0, ()))
    return x


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def dielectric_terms(rd, e1, e2, param, dt):
    """For rays rd (..., 3) hitting a static triangle with edges e1, e2 of a dielectric of refraction index param, in dt,
    as shade() computes them: (ri * sin_theta, dot(unit(rd), n)) -- the face-flipped normal unit(cross(e1, e2))."""
    rd = np.asarray(rd, dtype=dt)
    n = _unit(_cross(np.asarray(e1, dtype=dt), np.asarray(e2, dtype=dt)), dt)
    front = _dot(rd, n) < 0
    n = np.where(front[..., None], n, -n)
    ud = _unit(rd, dt)
    d = _dot(ud, n)
    cos = -np.fmin(d, dt(1))
    with np.errstate(invalid="ignore"):
        sin = np.sqrt(dt(1) - cos * cos)
    ri = np.where(front, dt(1) / dt(param), dt(param))
    return ri * sin, d


# the TIR triangles: edges whose normal is no axis (a triangle in an axis plane has a flat box, which Aabb::hit never enters)
TIR_E1, TIR_E2 = (10.0, 0.0, 0.5), (0.0, 10.0, 0.0)


def tir_directions(param, sz, dt):
    """Values s of the direction (s, 0, sz) for which ri * sin_theta is 1 - 1 ulp, exactly 1, 1 + 1 ulp in dt."""
    e1 = np.array(TIR_E1)
    lo, hi = 0.0, 10.0   # bisect for the threshold in f64, then scan the dt grid around it
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        prod, _ = dielectric_terms(np.array([mid, 0.0, sz]), e1, TIR_E2, param, np.float64)
        lo, hi = (lo, mid) if prod > 1.0 else (mid, hi)
    grid = dt(lo)
    sv = (grid + np.arange(-300000, 300001).astype(dt) * np.spacing(grid)).astype(dt)
    rd = np.stack([sv, np.zeros_like(sv), np.full_like(sv, sz)], axis=-1)
    prod, _ = dielectric_terms(rd, e1, TIR_E2, param, dt)
    out = []
    for target in (np.nextafter(dt(1), dt(0)), dt(1), np.nextafter(dt(1), dt(2))):
        k = np.flatnonzero(prod == target)
        if len(k):
            out.append((float(sv[k[0]]), float(target)))
    return out


def _tir_threshold(d, x):
    """Dielectric hits where ri * sin_theta is 1 - 1 ulp, exactly 1 and 1 + 1 ulp, in each precision: a back face of
    ri = 1.5 and a front face of refraction index 1/1.4 (ri = 1.4).  d.tir_rows: (prim, direction, param, dt, target)."""
    d.tir_rows = []
    for g, param, sz in (("dielectric_15", 1.5, 1.0), ("dielectric_07", 1.0 / 1.4, -1.0)):
        a = np.array([x - 5.0, -5.0, -1.0])
        i = d.triangle(a, a + TIR_E1, a + TIR_E2, d.mat(A.CR_MAT_DIELECTRIC, albedo=(1, 1, 1), param=param), (), g + "/tir_threshold")
        hit = a + 0.3 * np.array(TIR_E1) + 0.3 * np.array(TIR_E2)
        for dt in (np.float64, np.float32):
            for s, target in tir_directions(param, sz, dt):
                rd = np.array([s, 0.0, sz])
                d.special_rays.append((i, g + f"/tir_threshold/{dt.__name__}", hit - 2 * rd, rd, 0.0, ()))
                d.tir_rows.append((i, rd, param, dt, target))
        x += 20.0
    return x


def first_triple(seed, pixel, sample, dt):
    """The first random_unit_vector candidate of a key in dt and whether it is accepted."""
    s = stream_keys(seed, np.array([pixel]), np.array([sample]))
    us = []
    for _ in range(3):
        s, u = stream_next(s)
        us.append(u01_f32(u)[0] if dt == np.float32 else np.float64(int(u[0] >> _M(11))) * 2.0 ** -53)
    p = np.array([dt(-1) + dt(2) * dt(u) for u in us], dtype=dt)
    lensq = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    tiny = dt(0) if dt == np.float32 else dt(1e-160)
    return p, bool(tiny < lensq <= dt(1))


# (pixel, sample) keys of seed 0x5EED5 whose first f32 random_unit_vector candidate is accepted with z = -0.5 exactly
# (search_keys(0x5EED5, tolerance_accept)): a triangle whose edge cross product is -2 p then has the normal -ruv to the bit.
TOLERANCE_KEYS_F32 = ((505832, 60), (536279, 28))
TOLERANCE_SEED = 0x5EED5


def _lambert_tolerance(d, x, solid):
    """Lambertian hits whose normal cancels the key's random_unit_vector, so that n + ruv falls under the 1e-8 tolerance
    and the scattered direction is n itself.  f32: the keys above, cancelling exactly.  f64: the first accepted keys with
    z < 0; the edges (1, 0, -p.x/p.z) and (0, 1, -p.y/p.z) give a normal within a few ulps of -ruv."""
    m = d.mat(A.CR_MAT_LAMBERTIAN, texture=solid, param=1.0)
    f64_keys = []
    for pixel in range(1000):
        p, ok = first_triple(TOLERANCE_SEED, pixel, 0, np.float64)
        if ok and p[2] < -0.3:
            f64_keys.append((pixel, 0))
        if len(f64_keys) == 2:
            break
    d.tolerance_keys = []
    for dt, keys in ((np.float32, TOLERANCE_KEYS_F32), (np.float64, f64_keys)):
        for pixel, sample in keys:
            p, ok = first_triple(TOLERANCE_SEED, pixel, sample, dt)
            assert ok and p[2] < 0
            p = p.astype(np.float64)
            e1, e2 = np.array([1.0, 0.0, -p[0] / p[2]]), np.array([0.0, 1.0, -p[1] / p[2]])
            a = np.array([x, 0.5, -1.0])
            g = f"lambert_tolerance/{dt.__name__}"
            i = d.triangle(a, a + e1, a + e2, m, (), g)
            hit = a + 0.25 * e1 + 0.25 * e2
            ruv = p / np.sqrt(p @ p)
            d.special_rays.append((i, g, hit - 3 * ruv, 3 * ruv, 0.0, ((pixel, sample),)))
            d.tolerance_keys.append((pixel, sample, dt))
            x += 10.0
    return x


def texture_rows(d):
    """(rows, names): texture, u, v, p[3]."""
    rows, names = [], []

    def edge_values(n):
        vals = [0.0, -0.0, 1.0, float(np.nextafter(1.0, 0.0)), -0.25, 1.25, np.nan, np.inf, -np.inf, 0.5]
        for k in range(n + 1):
            for dt in (np.float64, np.float32):
                u = dt(k) / dt(n)
                vals += [float(u), float(ulp_shift(u, -1)), float(ulp_shift(u, 1))]
        return vals

    for name, ti in d.tex_names.items():
        if name.startswith("image_"):
            im = d.images[d.texs[ti].image]
            h, w = im.shape[:2]
            for u in edge_values(w):
                for v in (0.0, 0.5, 1.0, float(np.nextafter(1.0, 0.0))):
                    rows.append([ti, u, v, 0, 0, 0]); names.append(name + "/u_edges")
            for v in edge_values(h):
                for u in (0.0, 0.5, 1.0):
                    rows.append([ti, u, v, 0, 0, 0]); names.append(name + "/v_edges")
        else:
            inv = d.texs[ti].inv_scale
            pts = []
            for k in range(-3, 4):
                for dt in (np.float64, np.float32):
                    q = dt(k) / dt(inv)
                    pts += [float(q), float(ulp_shift(q, -1)), float(ulp_shift(q, 1))]
            rs = np.random.RandomState(len(rows))
            for _ in range(400):
                rows.append([ti, 0.3, 0.6] + list(rs.choice(pts, 3))); names.append(name + "/integer_multiples")
            big = 2.0 ** 31 / inv
            for p in ([big, 0, 0], [big, big, big], [-big, -big, 0.5 / inv], [1.5 * big, 0.7 * big, 0], [-4 * big, 3 * big, 2 * big],
                      [2 * big, 2 * big, -0.5 / inv], [np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 1, 1], [1e300, -1e300, 0]):
                rows.append([ti, 0.3, 0.6] + p); names.append(name + "/beyond_2^31")
            for _ in range(100):
                rows.append([ti, rs.rand(), rs.rand()] + list(rs.uniform(-50, 50, 3) / inv)); names.append(name + "/random")
    return np.array(rows, dtype=np.float64), np.array(names)


def sky_rows():
    """(rows, names): ray directions for the sky."""
    rows, names = [], []
    for dvec in ([0, 1, 0], [0, -1, 0], [0, 1e-300, 0], [0, -3, 0]):
        rows.append(dvec); names.append("pole")
    for x in (0.0, -0.0):
        for z in (-1.0, -0.0, 0.0, 1.0, -1e-30):
            for y in (0.0, 0.3, -0.3):
                rows.append([x, y, z]); names.append("seam")
    for z in (-1.0, -2.0):
        for x in (1e-300, -1e-300, 2.0 ** -60, -(2.0 ** -60), 2.0 ** -30, -(2.0 ** -30)):
            rows.append([x, 0.1, z]); names.append("seam_near")
    rs = np.random.RandomState(5)
    for s in (1.0, 1e-3, 1e3, 1e-150, 1e150):
        for _ in range(200):
            rows.append(list(rs.normal(size=3) * s)); names.append(f"random_len_{s:g}")
    # directions whose u or v lands on a texel edge of the environment map
    for k in range(ENV_W + 1):
        th = (k / ENV_W - 0.5) * 2 * np.pi
        rows.append([np.sin(th), 0.2, np.cos(th)]); names.append("texel_edge_u")
    for k in range(ENV_H + 1):
        ph = (k / ENV_H - 0.5) * np.pi
        rows.append([0.3, np.sin(ph), np.cos(ph)]); names.append("texel_edge_v")
    return np.array(rows, dtype=np.float64), np.array(names)


# (pixel, sample) keys of the seed the GPU test uses (0x5EED5) whose draws sit exactly on a decision in f32, found by
# stepping the streams of 2^22 x 64 keys with numpy (the f64 draws are 2^29 times finer: no such keys are in reach):
#   R0_KEYS: the first draw is 2844580 * 2^-24, which lies between Schlick's r0 of ri = 2.4 packed for a front face,
#            r0(1/2.4) = 0x1.5b3d22p-3, and for a back face, r0(2.4) = 0x1.5b3d20p-3.  A head-on hit at a pole has
#            cos_theta = 1, so the reflectance is r0 itself: the front-face record reflects, the back-face one would refract.
#   HALF_KEYS: random_unit_vector accepts its first triple, and the fourth draw, the Lambertian's, is exactly 0.5 --
#            scatter_prob 0.5 scatters (u <= p), a strict u < p would absorb.
R0_KEYS = ((177097, 5), (216421, 7), (660493, 9), (686306, 60))
HALF_KEYS = ((731513, 40), (1331176, 35), (2163584, 60), (2221524, 27))


def hit_rays(d, seed=7):
    """Candidate rays per hit primitive: (prim, group, ro, rd, rtime, keys) -- random rays at the primitive, the poles, the
    uv seam, grazing rays, rays from inside (back faces), at key starts and ends.  keys: (pixel, sample) pairs the ray must
    be shaded with besides random ones (R0_KEYS, HALF_KEYS), or ()."""
    rs = np.random.RandomState(seed)
    out = []
    for i, g, c, is_sphere in d.hit_prims:
        keyed = d.prims[i].key_count > 0
        times = [0.0, 0.25, 0.5, 0.75, 1.0, float(np.nextafter(0.25, 0)), 0.6] if keyed else [0.0]
        for _ in range(24):
            tgt = c + rs.uniform(-0.6, 0.6, 3) * (1, 1, 0.2 if not is_sphere else 1)
            ro = c + rs.normal(size=3) * 4 + (0, 0, 4 if not is_sphere else 0)
            out.append((i, g + "/random", ro, tgt - ro, float(rs.choice(times)), HALF_KEYS if g.startswith("lambert_solid_p05") else ()))
        if is_sphere:
            for t in times[:3]:
                out.append((i, g + "/pole_top", c + (0, 4, 0), np.array([0.0, -1.0, 0.0]), t, R0_KEYS if g.startswith("dielectric_24") else ()))
                out.append((i, g + "/pole_bottom", c + (0, -4, 0), np.array([0.0, 1.0, 0.0]), t, ()))
                out.append((i, g + "/seam", c + (-4, 0, 0), np.array([1.0, 0.0, 0.0]), t, ()))
                out.append((i, g + "/seam", c + (-4, 0.3, 0), np.array([1.0, 0.0, 0.0]), t, ()))
                out.append((i, g + "/grazing", c + (-4, 0.999, 0), np.array([1.0, 0.0, 0.0]), t, ()))
                out.append((i, g + "/inside", c + (0.1, 0.2, -0.1), rs.normal(size=3), t, ()))
                out.append((i, g + "/inside", c + (0.0, 0.0, 0.0), np.array([0.6, 0.0, 0.8]), t, ()))
            if g.startswith("dielectric") and not keyed:   # head-on: |dot(unit(rd), n)| can round past 1
                for _ in range(60):
                    ro = c + _unit(rs.normal(size=3), np.float64) * 4.0
                    out.append((i, g + "/head_on", ro, c - ro, 0.0, ()))
        else:
            for t in times[:3]:
                out.append((i, g + "/back_face", c + (0.1, -0.2, -3), np.array([0.0, 0.1, 1.0]), t, ()))
                out.append((i, g + "/front_face", c + (0.1, -0.2, 3), np.array([0.0, 0.1, -1.0]), t, ()))
                out.append((i, g + "/grazing", c + (-0.2, -0.3, 3), np.array([0.0, 0.0, -1.0]) + (0, 1e-9, 0), t, ()))
    return out + d.special_rays


def cameras():
    """(name, CrCameraDesc, from keys, at keys, params(real_type), pixel-sample triples)."""
    out = []
    W, H = 16, 9

    def desc(from_keys=(), at_keys=(), defocus=0.0, vfov=40.0, lf=(0.0, 1.0, 3.0), la=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0)):
        fa = (A.CrKeyframe * max(1, len(from_keys)))(*from_keys)
        aa = (A.CrKeyframe * max(1, len(at_keys)))(*at_keys)
        dsc = A.CrCameraDesc(W, H, vfov, defocus, 3.4, (C.c_double * 3)(*lf), (C.c_double * 3)(*la), (C.c_double * 3)(*vup),
                             len(from_keys), len(at_keys), fa, aa)
        dsc._keep = (fa, aa)
        return dsc, list(from_keys), list(at_keys)

    def params(frame, rate, angle, seed=1234):
        return lambda rt: A.CrRenderParams(4, 0, 4, 8, seed, frame, rt, rate, angle, 0, 0, 0, 0)

    pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (7, 4), (8, 5)]
    ijs = [(i, j, s) for i, j in pix for s in range(4)]
    keyed_from = (key(TX, 0.0, 0.5, 1.0), key(TY, 0.25, 0.5, -0.5, interp=NERP), key(TZ, 0.5, 0.5, 0.25))
    keyed_at = (key(TY, 0.0, 1.0, 0.5),)
    for name, (dsc, fk, ak), prm in (
            ("static", desc(), params(0, 24, 0.0)),
            ("static_shutter360", desc(), params(1, 24, 360.0)),
            ("static_defocus", desc(defocus=2.0), params(0, 24, 180.0)),
            ("static_far_frame", desc(), params(100003, 24, 180.0)),
            ("static_tilted", desc(lf=(2.0, -1.0, 5.0), la=(-1.0, 2.0, 0.0), vup=(0.2, 1.0, 0.1), vfov=90.0), params(0, 24, 0.0)),
            ("keyed_key_start", desc(keyed_from, keyed_at), params(1, 4, 0.0)),
            ("keyed_key_end", desc(keyed_from, keyed_at), params(2, 4, 0.0)),
            ("keyed_shutter360", desc(keyed_from, keyed_at), params(1, 4, 360.0)),
            ("keyed_defocus", desc(keyed_from, keyed_at, defocus=3.0), params(0, 4, 180.0)),
            ("keyed_far_frame", desc(keyed_from, keyed_at), params(100001, 4, 90.0))):
        out.append((name, dsc, fk, ak, prm, ijs))
    return out


def write_cameras(path, cams, real_type):
    parts = []
    for name, dsc, fk, ak, prm, ijs in cams:
        parts.append(bytes(dsc) + bytes(prm(real_type)) + np.array([len(ijs)], dtype=np.int32).tobytes() +
                     np.array(ijs, dtype=np.uint32).tobytes() + (bytes((A.CrKeyframe * len(fk + ak))(*(fk + ak))) if fk + ak else b""))
    with open(path, "wb") as f:
        f.write(b"".join(parts))


# ------------------------------------------------------------------ RNG streams and threshold searches
# The library's RNG (pathtrace.hpp rng_key / rng_next / u01) over many (pixel, sample) keys at once, for the searches
# that found the threshold keys of the corpus.  The tests do not run the searches; they check the keys they found
# against the oracle's own stream (oracle_rng_u64).
_M = np.uint64


def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
    return z ^ (z >> _M(31))


def stream_keys(seed, pixels, samples):
    gamma = _M(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        k = _mix64(_mix64(_M(seed) + gamma) ^ ((pixels.astype(_M) << _M(32)) | samples.astype(_M)))
    return np.where(k == 0, gamma, k)


def stream_next(s):
    """(new state, output) of one xorshift64* step."""
    s = s ^ (s >> _M(12))
    s = s ^ (s << _M(25))
    s = s ^ (s >> _M(27))
    with np.errstate(over="ignore"):
        return s, s * _M(0x2545F4914F6CDD1D)


def u01_f32(u):
    return (u >> _M(40)).astype(np.float32) * np.float32(2.0 ** -24)


def search_keys(seed, accept, n_pixels=1 << 22, want=4, chunk=1 << 16):
    """(pixel, sample) keys, sample < 64, whose first four f32 draws u1..u4 satisfy accept(u1, u2, u3, u4)."""
    found = []
    samp = np.arange(64, dtype=_M)
    for first in range(0, n_pixels, chunk):
        pix = np.repeat(np.arange(first, first + chunk, dtype=_M), 64)
        s = stream_keys(seed, pix, np.tile(samp, chunk))
        us = []
        for _ in range(4):
            s, u = stream_next(s)
            us.append(u01_f32(u))
        hit = np.flatnonzero(accept(*us))
        found += [(int(pix[i]), int(i % 64)) for i in hit]
        if len(found) >= want:
            return found[:want]
    return found


def r0_threshold_accept(u1, u2, u3, u4):   # R0_KEYS: the first draw between r0(1/2.4) and r0(2.4) in f32
    return u1 == np.float32(2844580 * 2.0 ** -24)


def half_accept(u1, u2, u3, u4):   # HALF_KEYS: the first triple accepted, the fourth draw exactly 0.5
    x, y, z = (np.float32(-1) + np.float32(2) * u for u in (u1, u2, u3))
    lensq = x * x + y * y + z * z
    return (lensq > 0) & (lensq <= 1) & (u4 == np.float32(0.5))


def tolerance_accept(u1, u2, u3, u4):   # TOLERANCE_KEYS_F32: the first triple accepted with z = -0.5 exactly
    x, y, z = (np.float32(-1) + np.float32(2) * u for u in (u1, u2, u3))
    lensq = x * x + y * y + z * z
    return (lensq > 0) & (lensq <= 1) & (z == np.float32(-0.5))
