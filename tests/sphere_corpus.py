"""Inputs for tests/sphere_roots_check.hip (tests/test_gpu_sphere_roots.py, tests/test_sphere_roots_host.py) and a numpy model of
Sphere::hit's root search in both of its forms: the reference's two divisions, and sphere_t's (crucible_amd/csrc/pathtrace.hpp),
which decides the second root without dividing where rule A or rule B proves the outcome.

A case is a row of 11 f64: centre (3), radius, ray origin (3), direction (3), tmax; tmin is always 0.001 (walk_round's).  The f32
forms take the f32 roundings of the row, so half of every group is made in f32 arithmetic and is exact in both types."""
import numpy as np

from walk_corpus import ulp_shift

TMIN = 0.001
# where a case left the search
P_NEG_DISC, P_ROOT1, P_RULE_A, P_RULE_B, P_DIV_MISS, P_DIV_HIT = range(6)
PATH_NAMES = ("disc<0", "root1", "rule A", "rule B", "divided: miss", "divided: root2")
# groups built so that each holds cases returned by rule A, by rule B and by the second division
RULE_GROUPS = ("on_sphere", "tmax_at_root", "root_at_tmin")


def model(rows, dt):
    """(hit_old, t_old, hit_new, t_new, path) of both forms in `dt` arithmetic on the rows rounded to `dt`; the expression
    trees are sphere_t's (no contraction: every numpy operation rounds once)."""
    it, shift = (np.int64, 32) if dt == np.float64 else (np.int32, 0)
    mbits = 20 if dt == np.float64 else 23
    with np.errstate(all="ignore"):
        r = np.asarray(rows, dtype=np.float64).astype(dt)
        c, rad, o, d, tmax = r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7:10], r[:, 10]
        oc = c - o
        h = (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1]) + d[:, 2] * oc[:, 2]
        cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - rad * rad
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        disc = h * h - a * cc
        neg = disc < 0
        s = np.sqrt(disc)
        n1, n2 = h - s, h + s
        root1, root2 = n1 / a, n2 / a
        tmin = dt(TMIN)
        in1 = (tmin < root1) & (root1 < tmax)
        in2 = (tmin < root2) & (root2 < tmax)
        hit_old = ~neg & (in1 | in2)
        t_old = np.where(in1, root1, root2)
        rule_a = ~(root1 <= tmin)
        hn = (n2.view(it) >> shift).astype(np.int64)
        ha = (a.view(it) >> shift).astype(np.int64)
        rule_b = hn < ha - (11 << mbits)
    path = np.full(len(r), P_DIV_MISS, dtype=np.uint8)
    path[in2] = P_DIV_HIT
    path[rule_b] = P_RULE_B
    path[rule_a] = P_RULE_A
    path[in1] = P_ROOT1
    path[neg] = P_NEG_DISC
    hit_new = (path == P_ROOT1) | (path == P_DIV_HIT)
    t_new = np.where(path == P_ROOT1, root1, root2)
    return hit_old, t_old, hit_new, t_new, path, (root1, root2)


def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _perp(n):
    """A unit vector perpendicular to every row of n."""
    k = np.argmin(np.abs(n), axis=1)
    e = np.zeros_like(n)
    e[np.arange(len(n)), k] = 1.0
    t = np.cross(n, e)
    return t / np.linalg.norm(t, axis=1)[:, None]


def _spheres(rs, n):
    c = rs.uniform(-10, 10, size=(n, 3))
    r = np.where(rs.rand(n) < 0.15, 1000.0, rs.uniform(0.2, 1.2, size=n))   # book1: small spheres on a ground of radius 1000
    return c, r


def _rows(c, r, o, d, tmax):
    return np.concatenate([c, r[:, None], o, d, np.broadcast_to(np.asarray(tmax, dtype=np.float64), (len(c),))[:, None]], axis=1)


def _native(rows, rs):
    """Half of the rows rounded to f32 (exact in both precisions), picked at random; the choice is returned."""
    f32 = rs.rand(len(rows)) < 0.5
    with np.errstate(over="ignore"):
        rows[f32] = rows[f32].astype(np.float32).astype(np.float64)
    return f32


def _surface_point(c, r, n, f32):
    """centre + r * n evaluated in the row's own precision."""
    o = c + r[:, None] * n
    with np.errstate(over="ignore"):
        o32 = (c.astype(np.float32) + r.astype(np.float32)[:, None] * n.astype(np.float32)).astype(np.float64)
    return np.where(f32[:, None], o32, o)


def _shift_own(x, k, f32):
    """x moved by k ulps of the row's own precision."""
    with np.errstate(over="ignore"):
        y32 = ulp_shift(x.astype(np.float32), k).astype(np.float64)
    return np.where(f32 if x.ndim == 1 else f32[:, None], y32, ulp_shift(x, k))


def on_sphere(rs, n):
    """A scattered ray's own sphere: origin centre + r n moved by 0, +-1, +-2 ulp per coordinate, direction outward, tangent
    or inward; and, as in a leaf of two, the neighbour's test with a closer hit already found (tmax before the sphere)."""
    c, r = _spheres(rs, n)
    nrm = _unit(rs, n)
    rows = _rows(c, r, np.zeros((n, 3)), np.zeros((n, 3)), np.inf)
    f32 = _native(rows, rs)
    c, r = rows[:, 0:3], rows[:, 3]
    o = _shift_own(_surface_point(c, r, nrm, f32), rs.randint(-2, 3, size=(n, 3)), f32)
    kind = rs.randint(0, 3, size=n)
    out = nrm + 0.9 * _unit(rs, n) * rs.rand(n)[:, None]   # Lambertian's normal + unit vector, shortened
    tan = _perp(nrm)
    inw = -nrm + 0.7 * _unit(rs, n)
    d = np.where((kind == 0)[:, None], out, np.where((kind == 1)[:, None], tan, inw)) * rs.uniform(0.3, 2.0, size=n)[:, None]
    rows[:, 4:7], rows[:, 7:10] = o, d
    rows[:, 10] = np.where(rs.rand(n) < 0.5, np.inf, rs.uniform(0.01, 20.0, size=n))
    # the neighbour: a sphere ahead of the ray, tested with tmax in front of it
    nb = rs.rand(n) < 0.15
    dn = d / np.linalg.norm(d, axis=1)[:, None]
    dist = rs.uniform(2.0, 6.0, size=n)
    rows[nb, 0:3] = (o + dn * dist[:, None])[nb]
    rows[nb, 3] = rs.uniform(0.2, 1.0, size=nb.sum())
    rows[nb, 10] = rs.uniform(0.01, 0.5, size=nb.sum())
    with np.errstate(over="ignore"):
        rows[f32] = rows[f32].astype(np.float32).astype(np.float64)
    return rows


def inside(rs, n):
    c, r = _spheres(rs, n)
    o = c + (r * rs.uniform(0, 0.95, size=n))[:, None] * _unit(rs, n)
    d = _unit(rs, n) * rs.uniform(0.3, 2.0, size=n)[:, None]
    tmax = np.where(rs.rand(n) < 0.7, np.inf, rs.uniform(0.001, 1.0, size=n))   # the short ones end before root2
    rows = _rows(c, r, o, d, tmax)
    _native(rows, rs)
    return rows


def _aimed(rs, n):
    """Origin outside, direction towards a point inside the sphere: both roots positive."""
    c, r = _spheres(rs, n)
    r = np.minimum(r, 1.2)
    o = c + (r * rs.uniform(1.5, 8.0, size=n))[:, None] * _unit(rs, n)
    target = c + (r * rs.uniform(0, 0.9, size=n))[:, None] * _unit(rs, n)
    d = (target - o)
    d = d / np.linalg.norm(d, axis=1)[:, None] * rs.uniform(0.3, 2.0, size=n)[:, None]
    return _rows(c, r, o, d, np.inf)


def tmax_at_root(rs, n):
    """tmax equal to a root of the row's own precision and one ulp to each side: rays from outside (rule A once tmax <= root1),
    from inside (root2 against tmax after the division) and leaving the surface (rule B whatever tmax is)."""
    k = n // 3
    rows = np.concatenate([_aimed(rs, k), inside(rs, k), on_sphere(rs, n - 2 * k)])
    f32 = _native(rows, rs)
    r64, r32 = model(rows, np.float64)[5], model(rows, np.float32)[5]
    which = rs.randint(0, 2, size=len(rows))
    root = np.where(f32, np.where(which == 0, r32[0], r32[1]).astype(np.float64), np.where(which == 0, r64[0], r64[1]))
    rows[:, 10] = _shift_own(root, rs.randint(-1, 2, size=len(rows)), f32)
    return rows


def root_at_tmin(rs, n):
    """A root at tmin and within a few ulp of it -- root1 from outside, root2 from inside -- and root2 around rule B's threshold
    2^-11.  Along the axis through the centre, at distance s from the surface and with |d| = L, the root is s / L."""
    c, r = _spheres(rs, n)
    r = np.minimum(r, 1.2)
    u = _unit(rs, n)
    L = rs.uniform(0.3, 2.0, size=n)
    flavour = rs.randint(0, 3, size=n)
    want = np.where(flavour == 2, 2.0 ** -11, TMIN)
    rows = _rows(c, r, np.zeros((n, 3)), u * L[:, None], np.inf)
    f32 = _native(rows, rs)
    c, r, d = rows[:, 0:3], rows[:, 3], rows[:, 7:10]
    L = np.linalg.norm(d, axis=1)
    want = np.where(f32 & (flavour != 2), np.float64(np.float32(TMIN)), want)
    s = _shift_own(want * L, rs.randint(-6, 7, size=n), f32)
    # outside, heading in: origin = centre - (r + s) u; inside, heading out: origin = centre + (r - s) u
    o = np.where((flavour == 0)[:, None], c - (r + s)[:, None] * (d / L[:, None]), c + (r - s)[:, None] * (d / L[:, None]))
    rows[:, 4:7] = o
    # half of the cases on a tiny sphere next to the origin, where nothing cancels and the root lands within an ulp or two of
    # s / L: origin 0, direction L e_k, centre +-(r +- s) e_k with r = 2^-12 (from outside) or 2^-9 (from inside)
    tiny = np.flatnonzero(rs.rand(n) < 0.5)
    k = len(tiny)
    Lt = rs.choice([0.5, 0.75, 1.0, 1.5, 2.0], size=k)
    rt = np.where(flavour[tiny] == 0, 2.0 ** -12, 2.0 ** -9)
    st = _shift_own(want[tiny] * Lt, rs.randint(-3, 4, size=k), f32[tiny])
    e = np.zeros((k, 3))
    e[np.arange(k), rs.randint(0, 3, size=k)] = rs.choice([-1.0, 1.0], size=k)
    rows[tiny, 0:3] = np.where((flavour[tiny] == 0)[:, None], (rt + st)[:, None] * e, -(rt - st)[:, None] * e)
    rows[tiny, 3] = rt
    rows[tiny, 4:7] = 0.0
    rows[tiny, 7:10] = Lt[:, None] * e
    near = rs.rand(n) < 0.4   # tmax next to tmin as well: rule A when root1 is just above both
    rows[near, 10] = _shift_own(np.full(n, TMIN), rs.randint(-3, 4, size=n), f32)[near]
    with np.errstate(over="ignore"):
        rows[f32] = rows[f32].astype(np.float32).astype(np.float64)
    return rows


def zero_discriminants(rows, dt):
    """How many cases have disc == 0 exactly in `dt` arithmetic (sphere_t's expression tree)."""
    with np.errstate(all="ignore"):
        r = np.asarray(rows, dtype=np.float64).astype(dt)
        c, rad, o, d = r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7:10]
        oc = c - o
        h = (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1]) + d[:, 2] * oc[:, 2]
        cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - rad * rad
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return int((h * h - a * cc == 0).sum())


def ties_with_tmin(rows, dt):
    """How many cases have a root one ulp below tmin, at tmin and one ulp above it, in `dt` arithmetic."""
    r1, r2 = model(rows, dt)[5]
    return [int(((r1 == t) | (r2 == t)).sum()) for t in (ulp_shift(np.array([dt(TMIN)]), k)[0] for k in (-1, 0, 1))]


def disc_zero(rs, n):
    """Tangent rays in exact arithmetic (small dyadic numbers: disc = 0 in both precisions), and the same moved by an ulp."""
    r = rs.randint(1, 9, size=n) / 4.0
    x = rs.randint(1, 12, size=n).astype(np.float64)
    L = 2.0 ** rs.randint(-3, 4, size=n)
    c = np.stack([np.zeros(n), r, np.zeros(n)], axis=1)
    o = np.stack([-x, np.zeros(n), np.zeros(n)], axis=1)
    d = np.stack([L, np.zeros(n), np.zeros(n)], axis=1)
    rows = _rows(c, r, o, d, np.where(rs.rand(n) < 0.5, np.inf, x / L))   # the tangent point is at t = x / L
    moved = rs.rand(n) < 0.5
    rows[moved, 1] = ulp_shift(rows[moved, 1].astype(np.float32), rs.randint(-1, 2, size=moved.sum())).astype(np.float64)
    perm = rs.permutation(3)   # not always the x axis
    for k in (0, 4, 7):
        rows[:, k:k + 3] = rows[:, k:k + 3][:, perm]
    return rows


def scaled_dir(rs, n):
    """Directions scaled by 2^+-500 and 2^-540 (|d|^2 subnormal in f64; overflow and zero in f32) and by 2^+-60, 2^-70 (the same
    corners in f32)."""
    k = n // 3
    rows = np.concatenate([_aimed(rs, k), inside(rs, k), on_sphere(rs, n - 2 * k)])
    e = rs.choice([500, -500, -540, 60, -60, -70], size=len(rows))
    rows[:, 7:10] *= (2.0 ** e)[:, None]
    fin = np.isfinite(rows[:, 10]) & (rs.rand(len(rows)) < 0.5)
    rows[fin, 10] *= 2.0 ** -e[fin]
    return rows


def zero_dir(rs, n):
    k = n // 3
    rows = np.concatenate([_aimed(rs, k), inside(rs, k), on_sphere(rs, n - 2 * k)])
    rows[:, 7:10] = np.where(rs.rand(len(rows), 3) < 0.5, 0.0, -0.0)
    return rows


def specials(rs, n_each):
    """+inf, -inf and NaN in each of the 11 operands of rays of every kind."""
    out = []
    for col in range(11):
        for v in (np.inf, -np.inf, np.nan):
            k = n_each // 3
            rows = np.concatenate([_aimed(rs, k), inside(rs, k), on_sphere(rs, n_each - 2 * k)])
            rows[:, col] = v
            out.append(rows)
    return np.concatenate(out)


def sphere_corpus(seed=5, scale=1.0):
    """Group name -> rows; about 2^20 cases at scale 1."""
    rs = np.random.RandomState(seed)
    n = lambda k: max(int(k * scale), 64)
    return {
        "on_sphere": on_sphere(rs, n(403000)),
        "inside": inside(rs, n(200000)),
        "tmax_at_root": tmax_at_root(rs, n(150000)),
        "root_at_tmin": root_at_tmin(rs, n(100000)),
        "disc_zero": disc_zero(rs, n(50000)),
        "scaled_dir": scaled_dir(rs, n(100000)),
        "zero_dir": zero_dir(rs, n(10000)),
        "specials": specials(rs, n(1100)),
    }


def check_coverage(names, path, hit, what):
    """The conditions that keep a comparison on this corpus from passing vacuously."""
    for g in RULE_GROUPS:
        sel = names == g
        for p in (P_RULE_A, P_RULE_B):
            assert (path[sel] == p).any(), f"{what}: group {g} has no case returned by {PATH_NAMES[p]}"
        assert ((path[sel] == P_DIV_MISS) | (path[sel] == P_DIV_HIT)).any(), f"{what}: group {g} has no case that divided"
    sel = names == "inside"
    assert (path[sel] == P_DIV_HIT).sum() > sel.sum() // 4, f"{what}: the inside group has too few hits at root2"
    assert hit[sel].any()


def coverage_table(names, path):
    lines = []
    for g in dict.fromkeys(names):
        sel = names == g
        lines.append(f"  {g}: {sel.sum()} cases; " + ", ".join(f"{PATH_NAMES[p]} {(path[sel] == p).sum()}" for p in range(6)))
    return "\n".join(lines)
