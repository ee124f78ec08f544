"""Inputs for tests/walk_check.hip (tests/test_gpu_walk_primitives.py) and the plain references they are compared with.

Box cases are rows of 13 f64: box planes x0 x1 y0 y1 z0 z1, ray origin (3), direction (3), tmax; tmin is always 0.001
(walk_round's).  The generators aim at the corners of the f64 screen's error bound (crucible_amd/csrc/pathtrace.hpp, the
comment above walk_round): rays that graze a box so that hi - lo lies within a few 2^-20 of zero, ties with tmax and
tmin, 1/direction and origin at the edges of the screen's range, box planes outside the normal f32 range, degenerate
boxes and signed zeros.  aabb_hit_ref is Aabb::hit (bvh.rs:96-132) in numpy, in either precision."""
import numpy as np

TMIN = 0.001


def ulp_shift(x, k):
    """x moved by k units in the last place of its own type (finite nonzero entries only)."""
    x = np.array(x)
    it = np.int64 if x.dtype == np.float64 else np.int32
    k = np.broadcast_to(np.asarray(k), x.shape).astype(it)
    ok = np.isfinite(x) & (x != 0)
    bits = x.view(it).copy()
    bits[ok] += k[ok]
    y = bits.view(x.dtype)
    y = np.where(np.isfinite(y) | ~ok, y, x)   # never step into inf/NaN
    return y


def slabs(c, dtype=np.float64):
    """Slab distances (n, 6) of Aabb::hit, 1/dir hoisted as the device does (the same value as the reference's per-axis
    1/d), in `dtype` arithmetic on the inputs rounded to `dtype`."""
    with np.errstate(all="ignore"):   # f64 beyond FLT_MAX becomes inf in f32, as on the device
        c = np.asarray(c, dtype=np.float64).astype(dtype)
        inv = dtype(1) / c[:, 9:12]
        t = np.empty((len(c), 6), dtype=dtype)
        for a in range(3):
            t[:, 2 * a] = (c[:, 2 * a] - c[:, 6 + a]) * inv[:, a]
            t[:, 2 * a + 1] = (c[:, 2 * a + 1] - c[:, 6 + a]) * inv[:, a]
    return t, inv


def aabb_hit_ref(c, dtype=np.float64):
    """Aabb::hit with the reference's compare/select form and per-axis early return, NaN slab distances included."""
    c = np.asarray(c, dtype=np.float64)
    t, _ = slabs(c, dtype)
    lo = np.full(len(c), dtype(TMIN), dtype=dtype)
    hi = c[:, 12].astype(dtype)
    alive = np.ones(len(c), dtype=bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            t0, t1 = t[:, 2 * a], t[:, 2 * a + 1]
            lt = t0 < t1
            nmin = np.where(lt, np.where(t0 > lo, t0, lo), np.where(t1 > lo, t1, lo))
            nmax = np.where(lt, np.where(t1 < hi, t1, hi), np.where(t0 < hi, t0, hi))
            lo, hi = nmin, nmax
            alive &= ~(hi <= lo)
    return alive


def interval_ref(c):
    """(lo, hi) of the f64 test in min/max form: lo = max(nears, 0.001), hi = min(fars, tmax) (rows with no NaN slab)."""
    t, _ = slabs(c)
    near = np.minimum(t[:, 0::2], t[:, 1::2])
    far = np.maximum(t[:, 0::2], t[:, 1::2])
    lo = np.maximum(near.max(axis=1), TMIN)
    hi = np.minimum(far.min(axis=1), np.asarray(c)[:, 12])
    return lo, hi


def _rows(b, o, d, tmax):
    return np.concatenate([b, o, d, np.asarray(tmax, dtype=np.float64).reshape(-1, 1)], axis=1)


def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _boxes(rs, n, scale, far=None):
    """Boxes of size ~scale; their centres up to `far` times scale away from the world origin."""
    far = np.ones(n) if far is None else far
    centre = rs.uniform(-4, 4, (n, 3)) * (scale * far)[:, None]
    half = rs.uniform(0.05, 1.0, (n, 3)) * scale[:, None]
    b = np.empty((n, 6))
    b[:, 0::2] = centre - half
    b[:, 1::2] = centre + half
    return b


def _surface_target(rs, b):
    """A point on a box corner, on an edge, or on a face plane (possibly beyond the face)."""
    n = len(b)
    lo, hi = b[:, 0::2], b[:, 1::2]
    side = rs.randint(0, 2, (n, 3))
    p = np.where(side == 1, hi, lo)
    kind = rs.randint(0, 3, n)                         # 0 corner, 1 edge, 2 face plane
    free = rs.randint(0, 3, n)
    u = rs.uniform(0, 1, n)
    ar = np.arange(n)
    edge_pt = lo[ar, free] + u * (hi[ar, free] - lo[ar, free])
    p[kind == 1, free[kind == 1]] = edge_pt[kind == 1]
    for a in range(3):
        m = (kind == 2) & (free != a)
        w = hi[m, a] - lo[m, a]
        p[m, a] = lo[m, a] - w + rs.uniform(0, 3, m.sum()) * w
    return p


def grazing(rs, n_want, far_origin=False, outside_band=False, batch=200000):
    """Rays aimed at a box edge, corner or face-plane point, the direction then moved by +-k ulp; kept when the f64
    hi - lo lies within 2^-18 M of zero (M = max(|lo|, |hi|)).  Scales 1e-6 .. 1e6.  far_origin: the box and the ray
    origin far from the world origin compared with the box (|o| |1/d| >> the slab distances: the 2^-21 Q term of TH).
    outside_band: kept only when hi - lo lies just outside the band (cases the screen decides, close to its boundary)."""
    out = []
    got = 0
    while got < n_want:
        scale = 10.0 ** rs.uniform(-6, 6, batch)
        far = 10.0 ** rs.uniform(1, 5, batch) if far_origin else None
        b = _boxes(rs, batch, scale, far)
        p = _surface_target(rs, b)
        dist = scale * 10.0 ** rs.uniform(-0.5, 3, batch)
        o = p + _unit(rs, batch) * dist[:, None]
        d = (p - o) * (10.0 ** rs.uniform(-3, 3, batch))[:, None]
        if outside_band:   # up to 2^41 ulp off: hi - lo just outside the band
            d = ulp_shift(d, rs.randint(-64, 65, d.shape) * 2 ** rs.randint(20, 36, (batch, 1)))
        else:
            d = ulp_shift(d, rs.randint(-64, 65, d.shape))
        tmax = np.where(rs.uniform(size=batch) < 0.8, np.inf, dist * 10.0 ** rs.uniform(-1, 1, batch) / np.linalg.norm(d, axis=1))
        c = _rows(b, o, d, tmax)
        lo, hi = interval_ref(c)
        with np.errstate(all="ignore"):
            m = np.maximum(np.abs(lo), np.abs(hi))
            keep = np.isfinite(hi - lo) & (np.abs(hi - lo) <= 2.0 ** -18 * m)
            if outside_band:   # beyond TH's estimate (its 2^-20 M and 2^-21 Q terms) by 10 %
                q = np.abs(c[:, 6:9] / c[:, 9:12]).max(axis=1)
                keep &= np.abs(hi - lo) > 1.1 * (2.0 ** -20 * m + 2.0 ** -21 * q)
        out.append(c[keep])
        got += keep.sum()
    return np.concatenate(out)[:n_want]


def random_set(rs, n):
    """Unbiased: boxes and rays of a small scene."""
    centre = rs.uniform(-10, 10, (n, 3))
    half = rs.uniform(0, 3, (n, 3))
    b = np.empty((n, 6))
    b[:, 0::2] = centre - half
    b[:, 1::2] = centre + half
    o = rs.uniform(-20, 20, (n, 3))
    d = rs.normal(size=(n, 3))
    tmax = np.where(rs.uniform(size=n) < 0.5, np.inf, rs.uniform(0, 50, n))
    return _rows(b, o, d, tmax)


def ties(rs, n):
    """tmax equal to one of the slab distances or +-1 ulp of it (f64 and f32 slab distances), and boxes near the origin
    whose plane puts a slab distance at tmin = 0.001 +- a few ulp."""
    c = random_set(rs, n)
    c[:, 6:9] = rs.uniform(-3, 3, (n, 3)) + (c[:, 0:6:2] + c[:, 1:6:2]) * 0.5 * (rs.uniform(size=(n, 1)) < 0.5)
    half = n // 2
    t64, _ = slabs(c[:half])
    t32, _ = slabs(c[half:], np.float32)
    k = rs.randint(0, 6, n)
    tt = np.concatenate([t64[np.arange(half), k[:half]], t32[np.arange(n - half), k[half:]].astype(np.float64)])
    tt = np.abs(tt)
    step = rs.randint(-1, 2, n)
    tmax = np.where(np.arange(n) < half, ulp_shift(tt, step), ulp_shift(tt.astype(np.float32), step).astype(np.float64))
    c[:, 12] = tmax
    # tmin ties: plane a = o + 0.001 d on one axis, moved by a few ulp (f64 or f32 ulps)
    m = n // 2
    e = random_set(rs, m)
    e[:, 6:9] = rs.uniform(-1e-3, 1e-3, (m, 3))
    ax = rs.randint(0, 3, m)
    which = rs.randint(0, 2, m)
    ar = np.arange(m)
    plane = e[ar, 6 + ax] + TMIN * e[ar, 9 + ax]
    in32 = rs.uniform(size=m) < 0.5
    p64 = ulp_shift(plane, rs.randint(-3, 4, m))
    p32 = ulp_shift(plane.astype(np.float32), rs.randint(-3, 4, m)).astype(np.float64)
    plane = np.where(in32, p32, p64)
    other = plane + np.where(e[ar, 9 + ax] > 0, 1.0, -1.0) * rs.uniform(0.01, 2, m) * np.where(which == 1, 1.0, -1.0)
    e[ar, 2 * ax] = np.minimum(plane, other)
    e[ar, 2 * ax + 1] = np.maximum(plane, other)
    for a in range(3):   # the other axes: a box around the ray near tmin
        sel = ax != a
        pt = e[sel, 6 + a] + TMIN * e[sel, 9 + a]
        w = rs.uniform(1e-4, 1, sel.sum())
        e[sel, 2 * a] = pt - w
        e[sel, 2 * a + 1] = pt + w
    return np.concatenate([c, e])


def range_limits(rs, n):
    """|1/d| and |o| at 2^-100 and 2^100 (f32 values, the screen's range test) and one f32 ulp either side."""
    lim = np.array([2.0 ** -100, 2.0 ** 100], dtype=np.float32)
    cases = []
    for which in range(2):
        for step in (-1, 0, 1):
            v = ulp_shift(np.full(n, lim[which], dtype=np.float32), step).astype(np.float64)
            # 1/d at the limit on one axis, the others ordinary or at the limit too
            c = random_set(rs, n)
            ax = rs.randint(0, 3, n)
            sign = np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)
            c[np.arange(n), 9 + ax] = sign / v
            allax = rs.uniform(size=n) < 0.3
            c[allax, 9:12] = np.sign(c[allax, 9:12]) / v[allax, None]
            cases.append(c)
            # the origin at the limit on one axis, the box next to it
            c = random_set(rs, n)
            ax = rs.randint(0, 3, n)
            c[np.arange(n), 6 + ax] = sign * v
            ctr = c[:, 6:9] + rs.normal(size=(n, 3)) * (v[:, None] * 10.0 ** rs.uniform(-8, 0, (n, 1)))
            half = np.abs(ctr) * 10.0 ** rs.uniform(-9, -1, (n, 3)) + 1.0
            c[:, 0:6:2], c[:, 1:6:2] = ctr - half, ctr + half
            c[:, 9:12] = ctr - c[:, 6:9] + rs.normal(size=(n, 3)) * half
            cases.append(c)
    return np.concatenate(cases)


def extreme_planes(rs, n):
    """Box planes below the normal f32 range (subnormal or flushed to 0 in f32) and beyond FLT_MAX (inf in f32)."""
    tiny = np.array([1e-39, 3e-40, 1e-44, 1e-45, 7e-46, 1e-50, 1.1754942e-38, 1.1754944e-38, 0.0])
    huge = np.array([3.4028235e38, 3.4028236e38, 3.5e38, 1e39, 1e300, np.finfo(np.float64).max])
    cases = []
    c = random_set(rs, n)
    c[:, 0:6] = rs.choice(tiny, (n, 6)) * np.where(rs.uniform(size=(n, 6)) < 0.5, -1.0, 1.0)
    c[:, 0:6:2], c[:, 1:6:2] = np.minimum(c[:, 0:6:2], c[:, 1:6:2]), np.maximum(c[:, 0:6:2], c[:, 1:6:2])
    c[:, 6:9] = rs.choice(np.concatenate([tiny, -tiny, [1e-30, -1e-30]]), (n, 3))
    c[:, 9:12] = rs.normal(size=(n, 3)) * (10.0 ** rs.uniform(-40, 0, (n, 1)))   # |1/d| up to about 2^100 and beyond
    c[:, 12] = np.where(rs.uniform(size=n) < 0.5, np.inf, 10.0 ** rs.uniform(-4, 2, n))
    cases.append(c)
    c = random_set(rs, n)
    big = rs.choice(huge, (n, 6)) * np.where(rs.uniform(size=(n, 6)) < 0.5, -1.0, 1.0)
    use = rs.uniform(size=(n, 6)) < 0.5
    c[:, 0:6] = np.where(use, big, c[:, 0:6])
    c[:, 0:6:2], c[:, 1:6:2] = np.minimum(c[:, 0:6:2], c[:, 1:6:2]), np.maximum(c[:, 0:6:2], c[:, 1:6:2])
    cases.append(c)
    return np.concatenate(cases)


def degenerate(rs, n):
    """Zero-thickness boxes (axis-flat triangles), empty boxes (+inf .. -inf, as the builder leaves an empty wrapper) and
    inverted ones, planes one f64 ulp apart (the same f32)."""
    cases = []
    g = grazing(rs, n)
    ax = rs.randint(0, 3, n)
    ar = np.arange(n)
    g[ar, 2 * ax + 1] = g[ar, 2 * ax]
    cases.append(g)
    c = random_set(rs, n)
    c[ar, 2 * ax + 1] = c[ar, 2 * ax]
    c[ar, 6 + ax] = np.where(rs.uniform(size=n) < 0.3, c[ar, 2 * ax], c[ar, 6 + ax])
    cases.append(c)
    c = random_set(rs, n)
    c[:, 0:6:2] = np.inf
    c[:, 1:6:2] = -np.inf
    cases.append(c)
    c = random_set(rs, n)
    c[ar, 2 * ax], c[ar, 2 * ax + 1] = c[ar, 2 * ax + 1].copy(), c[ar, 2 * ax].copy()
    cases.append(c)
    c = random_set(rs, n)
    c[ar, 2 * ax + 1] = ulp_shift(c[ar, 2 * ax], 1)
    cases.append(c)
    return np.concatenate(cases)


def signed_zeros(rs, n):
    """The origin exactly on a box plane (b - o = +0), with 1/d of either sign: the slab distance is -0 or +0; and zero
    or subnormal direction components (infinite 1/d: NaN slab distances, the exact_box rays)."""
    cases = []
    c = random_set(rs, n)
    ar = np.arange(n)
    for _ in range(2):
        ax = rs.randint(0, 3, n)
        c[ar, 6 + ax] = c[ar, 2 * ax + rs.randint(0, 2, n)]
    c[:, 9:12] = np.where(rs.uniform(size=(n, 3)) < 0.5, -1.0, 1.0) * np.abs(c[:, 9:12])
    cases.append(c)
    c = c.copy()
    c[rs.uniform(size=n) < 0.5, 6:9] = 0.0
    c[:, 0:6] = np.where(rs.uniform(size=(n, 6)) < 0.3, np.where(rs.uniform(size=(n, 6)) < 0.5, 0.0, -0.0), c[:, 0:6])
    c[:, 0:6:2], c[:, 1:6:2] = np.minimum(c[:, 0:6:2], c[:, 1:6:2]), np.maximum(c[:, 0:6:2], c[:, 1:6:2])
    cases.append(c)
    c = random_set(rs, n)
    ax = rs.randint(0, 3, n)
    zs = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e-320, 1e-39, -1e-45, 1e-46])
    c[ar, 9 + ax] = rs.choice(zs, n)
    on = rs.uniform(size=n) < 0.5
    c[on, 6 + ax[on]] = c[on, 2 * ax[on]]
    cases.append(c)
    return np.concatenate(cases)


# Found by this corpus: a finite f64 plane beyond FLT_MAX is an infinite f32 plane, and the f32 box then reaches past the
# f64 box's far end: here Aabb::hit misses (y leaves at t = 3.5e8, x enters at 1e9) while the f32 screen sees hi32 - lo32 =
# 1e9, far above TH.  The screening records report such planes and the tree is then walked without the screen.
OVERFLOW_MISS = np.array([[1e9, 2e9, -1.0, 3.5e38, -1.0, 1e10, 0.0, 0.0, 0.0, 1.0, 1e30, 1.0, np.inf]])


def box_corpus(seed=1, scale=1):
    """Named groups of box cases.  scale multiplies the group sizes (1: the GPU test's corpus)."""
    rs = np.random.RandomState(seed)
    k = lambda m: max(64, int(m * scale))  # noqa: E731
    return {
        "grazing": grazing(rs, k(150000)),
        "grazing_far_origin": grazing(rs, k(100000), far_origin=True),
        "grazing_outside_band": np.concatenate([grazing(rs, k(20000), outside_band=True), grazing(rs, k(10000), True, True)]),
        "ties": ties(rs, k(60000)),
        "range_limits": range_limits(rs, k(10000)),
        "extreme_planes": extreme_planes(rs, k(30000)),
        "degenerate": degenerate(rs, k(20000)),
        "signed_zeros": signed_zeros(rs, k(30000)),
        "random": random_set(rs, k(200000)),
        "overflow_miss": OVERFLOW_MISS,
    }


def prim_corpus(seed=2, n=8000):
    """Rows of 17 f64 for walk_check's prim part: kind (0 sphere, 1 triangle), g[9] (centre + radius, or a, b, c), origin,
    direction, tmax (inf here: tests/test_gpu_walk_primitives.py adds the tmax ties from the oracle's own t)."""
    rs = np.random.RandomState(seed)
    rows = []

    def put(kind, g, o, d):
        m = len(o)
        r = np.zeros((m, 17))
        r[:, 0] = kind
        r[:, 1:1 + g.shape[1]] = g
        r[:, 10:13], r[:, 13:16], r[:, 16] = o, d, np.inf
        rows.append(r)

    for scale in (1e-6, 1e-3, 1.0, 1e3, 1e6):
        c = rs.uniform(-4, 4, (n, 3)) * scale
        rad = rs.uniform(0.1, 2, n) * scale
        # tangent rays: through the point c + r n with a direction perpendicular to n, then +-k ulp
        nrm = _unit(rs, n)
        t = np.cross(nrm, _unit(rs, n))
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        p = c + rad[:, None] * nrm
        dist = rad * 10.0 ** rs.uniform(0, 2, n)
        o = p - t * dist[:, None]
        put(0, np.column_stack([c, rad]), o, ulp_shift(t * 10.0 ** rs.uniform(-2, 2, (n, 1)), rs.randint(-8, 9, (n, 3))))
        # origins on the surface, and 0.001 |d| before it (t at the tmin boundary)
        u = _unit(rs, n)
        d = _unit(rs, n) * 10.0 ** rs.uniform(-1, 1, (n, 1))
        on = c + rad[:, None] * u
        o = np.where((rs.uniform(size=n) < 0.5)[:, None], on, on - TMIN * d)
        put(0, np.column_stack([c, rad]), ulp_shift(o, rs.randint(-2, 3, (n, 3))), d)
        # zero radius, aimed at the centre or near it
        o = c + _unit(rs, n) * (scale * 5)
        put(0, np.column_stack([c, np.zeros(n)]), o, ulp_shift(c - o, rs.randint(-2, 3, (n, 3))))
        # triangles: aim at a vertex, an edge (u or v = 0, u + v = 1) or inside, then +-k ulp
        a = rs.uniform(-4, 4, (n, 3)) * scale
        e1, e2 = rs.normal(size=(n, 3)) * scale, rs.normal(size=(n, 3)) * scale
        b, cc = a + e1, a + e2
        uu = rs.choice([0.0, 1.0, 0.5, 0.25], n)
        vv = np.where(rs.uniform(size=n) < 0.5, 1.0 - uu, rs.choice([0.0, 0.5], n))
        inside = rs.uniform(size=n) < 0.2
        uu[inside], vv[inside] = rs.uniform(0, 0.5, inside.sum()), rs.uniform(0, 0.5, inside.sum())
        p = a + uu[:, None] * e1 + vv[:, None] * e2
        o = p + _unit(rs, n) * (scale * 10.0 ** rs.uniform(0, 2, (n, 1)))
        put(1, np.column_stack([a, b, cc]), o, ulp_shift(p - o, rs.randint(-4, 5, (n, 3))))
        # det at +-eps: a direction almost in the triangle's plane
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        inplane = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
        eps = np.where(rs.uniform(size=n) < 0.5, 2.220446049250313e-16, 1.1920928955078125e-07)
        # det = dot(e1, cross(d, e2)) = tilt |e1 x e2| for d = e1/|e1| + tilt n
        tilt = eps * rs.choice([0.5, 0.99, 1.0, 1.01, 2.0, -1.0], n) / np.linalg.norm(np.cross(e1, e2), axis=1)
        d = inplane + tilt[:, None] * nrm
        o = a + 0.3 * e1 + 0.3 * e2 - d * scale
        put(1, np.column_stack([a, b, cc]), o, d)
        # zero area: collinear vertices, or two equal
        cc2 = np.where((rs.uniform(size=n) < 0.5)[:, None], a + 2.0 * e1, a)
        o = a + _unit(rs, n) * scale * 3
        put(1, np.column_stack([a, b, cc2]), o, a + 0.5 * e1 - o)
    return np.concatenate(rows)


def trig_inputs():
    """The inputs of test_defined_trig_functions_against_glibc, plus every breakpoint of the software atan / asin / acos
    (0.4375, 0.6875, 1.1875, 2.4375; 0.5, 1) and +-2 ulp of it, in f64 and f32 ulps, both signs."""
    rs = np.random.RandomState(5)
    n = 200000
    y = np.concatenate([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n) * 10.0 ** rs.uniform(-8, 8, n)])
    x = np.concatenate([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n) * 10.0 ** rs.uniform(-8, 8, n)])
    special_y = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.4375, 0.6875, 1.1875, 2.4375, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0]
    special_x = [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, -0.0, 0.0, 1.0, -np.inf, 1.0, 1.0]
    bps = np.array([0.4375, 0.6875, 1.1875, 2.4375, 0.5, 1.0])
    pts = [bps]
    for k in (-2, -1, 1, 2):
        pts.append(ulp_shift(bps, k))
        pts.append(ulp_shift(bps.astype(np.float32), k).astype(np.float64))
    pts = np.concatenate(pts)
    pts = np.concatenate([pts, -pts])
    by = np.concatenate([pts, pts, np.ones_like(pts), -np.ones_like(pts)])
    bx = np.concatenate([np.ones_like(pts), -np.ones_like(pts), 1.0 / pts, -1.0 / pts])
    return np.concatenate([y, special_y, by]), np.concatenate([x, special_x, bx])
