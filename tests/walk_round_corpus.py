"""Inputs of tests/walk_round_check.hip (tests/test_gpu_walk_round.py): scenes, ray groups, schedules and the lane
assignments, plus a walker of an exported tree in plain Python over the oracle's box and primitive tests, with which
tests/test_walk_round_corpus.py checks that every ray group reaches what it claims.

Every primitive has a material of its own, so the material index of a hit names the primitive (flatten() numbers the
materials in the order of the primitives)."""
import ctypes as C
import struct

import numpy as np

from crucible_amd import _abi as A
from crucible_amd.scene import HitList, Lambertian, Scene, Sphere, Triangle

EYE = np.array([0.0, 4.0, 11.0])
K = 4                       # rays per lane at the most
PERM_SEEDS = (101, 202, 303)
BUDGETS = (0, 1, 2, 3, 7, 1000)          # 0 = unbounded, as in the kernel
LEAF_MINS = (0, 1, 8, 63, 64)
EXITS = (1, 33, 64)
SCHEDULES = [(b, m, e) for b in BUDGETS for m in LEAF_MINS for e in EXITS]   # (budget, walk_leaf_min, walk_exit_lanes)
EXACT_GROUPS = ("axis_one_zero", "axis_two_zeros")            # an infinite 1/direction: Aabb::hit's compare/select form, every kernel
UNSCREENED_GROUPS = ("far_origin", "tiny_direction")        # outside screen_in_range: exact steps in the f64 SCREEN kernels alone


def own_material():
    return Lambertian.new_from_color((0.5, 0.5, 0.5), 1.0)


def scene(kind):
    """main: a ground, 170 small spheres and 30 triangles in the style of test_gpu_variants.matrix_scene; list: the same with
    twelve of the spheres in a HitList element; two: two spheres (the root is the only wrapper, and a leaf)."""
    sc = Scene.new_image(1.5, 12, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(1)
    cam.set_max_depth(1)
    cam.look_from(tuple(EYE))
    cam.look_at((0.0, 0.4, 0.0))
    cam.set_vfov(42.0)
    if kind == "two":
        sc.add_element(Sphere.new((-0.6, 0.5, 0.0), 0.5, own_material()), "a")
        sc.add_element(Sphere.new((0.7, 0.4, -1.0), 0.4, own_material()), "b")
        return sc
    assert kind in ("main", "list")
    rs = np.random.RandomState(91)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, own_material()), "ground")
    listed = HitList.default()
    for k in range(170):
        x, z = -6.0 + 12.0 * rs.rand(), -6.0 + 10.0 * rs.rand()
        r = 0.12 + 0.2 * rs.rand()
        s = Sphere.new((x, r, z), r, own_material())
        if kind == "list" and k < 12:
            listed.add(s)
        else:
            sc.add_element(s, f"s{k}")
    for k in range(30):
        x, z = -5.0 + 10.0 * rs.rand(), -5.0 + 8.0 * rs.rand()
        sc.add_element(Triangle.new((x, 0.0, z), (x + 0.5, 0.0, z + 0.1), (x + 0.2, 0.6, z - 0.1), own_material()), f"t{k}")
    if kind == "list":
        sc.add_element(listed, "listed")
    return sc


def prim_table(flat):
    """Per CrPrimitive record: (kind, v[9], material)."""
    return [(p.kind, np.array(p.v[:], dtype=np.float64), p.material) for p in flat.prims[:flat.desc.n_prims]]


def centres(flat):
    """A point inside every sphere and triangle of the description."""
    out = []
    for kind, v, _ in prim_table(flat):
        if kind == A.CR_PRIM_SPHERE and v[3] < 10.0:
            out.append(v[:3])
        elif kind == A.CR_PRIM_TRIANGLE:
            out.append((v[0:3] + v[3:6] + v[6:9]) / 3.0)
    return np.array(out)


# ------------------------------------------------------------------ a walker of the exported tree
def walk(o, prims, tree, ray):
    """BVHWrapper::hit over an exported tree (boxes, children, split_axis) with the oracle's own Aabb::hit, Sphere::hit and
    Triangle::hit: (closest primitive or -1, its t, node tests, primitive tests, events, visited), events = (leaf wrapper,
    primitive, t) of every hit that became the closest so far and visited = (wrapper, closest t when its box was tested), both
    in walk order.  Scenes without list elements."""
    boxes, kids, axis = tree
    orig, d = o.arr(ray[0:3]), o.arr(ray[3:6])
    st = {"t": np.inf, "best": -1, "nodes": 0, "prims": 0}
    events, visited = [], []
    rec = np.zeros(10, dtype=o.np_real)

    def prim_hit(desc):
        kind, v, _ = prims[desc]
        st["prims"] += 1
        if kind == A.CR_PRIM_SPHERE:
            g = o.arr(v[:4])
            hit = o.lib.oracle_sphere_hit(o._p(g), o._p(orig), o._p(d), o.real(0.001), o.real(st["t"]), o._p(rec))
        else:
            assert kind == A.CR_PRIM_TRIANGLE
            g = o.arr(v[:9])
            hit = o.lib.oracle_triangle_hit(o._p(g), o._p(orig), o._p(d), o.real(0.001), o.real(st["t"]), o._p(rec))
        return rec[0] if hit else None

    def visit(w):
        st["nodes"] += 1
        visited.append((w, float(st["t"])))
        box = o.arr(boxes[w])
        if not o.lib.oracle_aabb_hit(o._p(box), o._p(orig), o._p(d), o.real(0.001), o.real(st["t"])):
            return
        a, b = int(kids[w, 0]), int(kids[w, 1])
        if a < 0:
            for desc in ([~a] if a == b else [~a, ~b]):
                t = prim_hit(desc)
                if t is not None:
                    st["t"], st["best"] = t, desc
                    events.append((w, desc, float(t)))
        else:
            if axis[w] >= 0 and d[axis[w]] < 0:
                a, b = b, a
            visit(a)
            visit(b)

    visit(0)
    return st["best"], st["t"], st["nodes"], st["prims"], events, visited


# ------------------------------------------------------------------ the screen's band, restated
def screen_margin(box, ray, tmax=np.inf):
    """|hi32 - lo32| / TH of walk_round's f32 screen for this f64 box and ray with the closest hit so far at tmax, in numpy f32 with the slab
    distance as a product and a difference (the kernel fuses them: at most one more rounding of |of if|, far inside TH's
    16 u (M + Q)); inf where the ray is outside screen_in_range.  A ratio well below 1 lands in the band."""
    f = np.float32
    with np.errstate(all="ignore"):
        of = np.asarray(ray[0:3], dtype=np.float64).astype(f)
        inv = (1.0 / np.asarray(ray[3:6], dtype=np.float64)).astype(f)
        if not (np.isfinite(inv).all() and np.abs(inv).min() >= f(2.0 ** -100) and np.abs(inv).max() <= f(2.0 ** 100) and np.abs(of).max() <= f(2.0 ** 100)):
            return np.inf
        b = np.asarray(box, dtype=np.float64).astype(f).reshape(3, 2)
        p = of * inv
        t = b * inv[:, None] - p[:, None]
        lo = max(t.min(axis=1).max(), f(0.001))
        hi = min(t.max(axis=1).min(), f(tmax))
        q = np.abs(p).max()
        th = f(2.0 ** -20) * max(abs(lo), abs(hi)) + f(2.0 ** -20) * q + np.abs(inv).max() * f(2.0 ** -147) + f(1e-35)
        return float(abs(hi - lo) / th)


def in_band(tree, ray, ratio=0.25):
    """Indices of the wrappers on whose box the ray's screen test falls in the band with a margin."""
    return [w for w in range(len(tree[0])) if screen_margin(tree[0][w], ray) <= ratio]


def band_then_steps(o, prims, tree, ray):
    """By the walker's trace: the ray meets an inner wrapper whose screen test falls in the band (at the closest hit it has
    by then) and visits further wrappers after it."""
    visited = walk(o, prims, tree, ray)[5]
    at = [i for i, (w, tmax) in enumerate(visited) if tree[1][w, 0] >= 0 and screen_margin(tree[0][w], ray, tmax) <= 0.25]
    return bool(at) and at[0] + 1 < len(visited)


def band_candidates(tree, rs, per_tree=40, prefer=None):
    """Rays from EYE through a point of a box edge -- where a silhouette edge is met, the ray enters and leaves the box at the
    same distance -- moved by up to 3 ulp(f32) across the edge.  Wrappers from the whole tree, the root's children to the
    leaves; the rays `prefer` accepts come first and make up half of the group where that many are found."""
    boxes = tree[0]
    first, out = [], []
    picks = rs.permutation(len(boxes))
    for w in picks:
        b = boxes[w].reshape(3, 2)
        if not np.isfinite(b).all() or (b[:, 1] - b[:, 0]).max() > 50.0:
            continue
        for ax in range(3):                # the edge runs along ax
            u, v = [a for a in range(3) if a != ax]
            for cu in (0, 1):
                for cv in (0, 1):
                    e = np.zeros(3)
                    e[ax] = b[ax, 0] + (b[ax, 1] - b[ax, 0]) * rs.uniform(0.2, 0.8)
                    e[u], e[v] = b[u, cu], b[v, cv]
                    k = rs.randint(-3, 4)
                    e[u] = float(np.float32(e[u]) + k * np.spacing(np.float32(e[u])))
                    ray = np.concatenate([EYE, e - EYE, [0.0]])
                    if screen_margin(boxes[w], ray) <= 0.25:
                        (first if prefer is not None and prefer(ray) else out).append(ray)
        if len(first) >= per_tree // 2 and len(first) + len(out) >= per_tree:
            break
    return (first + out)[:per_tree]


# ------------------------------------------------------------------ ray groups
def camera_rays(o, cam, seed=7):
    cd = cam.desc()
    p = cam.params(seed, o.real_type, 0, None, 0, A.CR_SUM_DEFAULT)
    rows = np.zeros((cam.image_height * cam.image_width, 8), dtype=o.np_real)
    for j in range(cam.image_height):
        for i in range(cam.image_width):
            o.lib.oracle_camera_ray(C.byref(cd), C.byref(p), i, j, 0, o._p(rows[j * cam.image_width + i]))
    return rows[:, :7].astype(np.float64)


def rays(kind, o64, sc, trees):
    """(n x 7 f64 rows: origin, direction, time; group name per row).  trees: {"ref": exported CR_BVH_REFERENCE tree, "ord":
    exported CR_BVH_SAH_ORDERED tree} of the scene in f64; the groups that are found by a search use the walker on them."""
    flat = sc.flatten()
    prims = prim_table(flat)
    cs = centres(flat)
    rs = np.random.RandomState(5)
    groups = []

    def add(name, rows):
        groups.extend((name, np.asarray(r, dtype=np.float64)) for r in rows)

    add("camera", camera_rays(o64, sc.scene_cam))
    add("miss_root", [np.concatenate([[rs.uniform(-5, 5), 50.0, rs.uniform(-5, 5)], [rs.normal(), 0.2 + abs(rs.normal()), rs.normal()], [0.0]])
                      for _ in range(16)])
    inside = []
    for _ in range(32 if kind != "two" else 8):
        p = np.array([rs.uniform(-5, 5), rs.uniform(0.05, 0.5), rs.uniform(-5, 4)]) if kind != "two" else np.array([0.05, 0.45, -0.4]) + 0.05 * rs.normal(size=3)
        d = p - np.array([0.0, 0.3, -0.5]) + 0.3 * rs.normal(size=3)
        inside.append(np.concatenate([p, d, [0.0]]))
    add("inside_out", inside)
    two, one, tiny = [], [], []
    for c in cs[rs.permutation(len(cs))[:8]]:
        two += [np.concatenate([c + [0, 3, 0], [0, -1, 0], [0.0]]), np.concatenate([c + [20, 0, 0], [-2, 0, 0], [0.0]]),
                np.concatenate([c + [0, 0, 20], [0, 0, -1], [0.0]])]
        one += [np.concatenate([c + [0, 2, 5], [0, -2, -5], [0.0]]), np.concatenate([c + [3, 2, 0], [-3, -2, 0], [0.0]]),
                np.concatenate([c + [-4, 0, 6], [2, 0, -3], [0.0]])]
        tiny += [np.concatenate([c + [0, 3, 4], [1e-31, -3, -4], [0.0]]), np.concatenate([c + [2, 3, 0], [-2, -3, -1e-33], [0.0]])]
    add("axis_two_zeros", two)
    add("axis_one_zero", one)
    add("tiny_direction", tiny)     # a finite 1/direction beyond 2^100: outside screen_in_range
    add("far_origin", [np.concatenate([[2e30, rs.uniform(0, 1), rs.uniform(-3, 3)], [-1.0, rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1)], [0.0]])
                       for _ in range(8)] +
        [np.concatenate([[rs.uniform(-3, 3), 3e30, rs.uniform(-3, 3)], [rs.uniform(-0.1, 0.1), -1.0, rs.uniform(-0.1, 0.1)], [0.0]]) for _ in range(8)])
    for name, tree in sorted(trees.items()):
        add("band_" + name, band_candidates(tree, rs, prefer=(lambda r, tree=tree: band_then_steps(o64, prims, tree, r)) if kind == "main" else None))
    if kind == "main":
        for name, tree in sorted(trees.items()):
            second, later = [], []
            kids = tree[1]
            leaves = [w for w in range(len(kids)) if kids[w, 0] < 0 and kids[w, 0] != kids[w, 1]]
            for w in leaves:   # aim at the second primitive of a two-primitive leaf
                desc = ~int(kids[w, 1])
                kd, v, _ = prims[desc]
                target = v[:3] if kd == A.CR_PRIM_SPHERE else (v[0:3] + v[3:6] + v[6:9]) / 3.0
                if kd == A.CR_PRIM_SPHERE and v[3] > 10.0:
                    continue
                ray = np.concatenate([EYE, target - EYE, [0.0]])
                if len(second) < 24 and walk(o64, prims, tree, ray)[0] == desc:
                    second.append(ray)
            for _ in range(4000):   # low rays through the crowd: a farther primitive is met first, a nearer one later
                if len(later) >= 24:
                    break
                a = np.array([rs.uniform(-7, 7), rs.uniform(0.1, 0.5), rs.uniform(5, 7)])
                b = np.array([rs.uniform(-6, 6), rs.uniform(0.1, 0.4), rs.uniform(-6, -2)])
                ray = np.concatenate([a, b - a, [0.0]])
                if later_leaf_is_nearer(walk(o64, prims, tree, ray)[4]):
                    later.append(ray)
            add("second_primitive_" + name, second)
            add("later_leaf_nearer_" + name, later)
    names = np.array([g for g, _ in groups])
    rows = np.array([r for _, r in groups])
    return rows, names


def later_leaf_is_nearer(events):
    """Two different leaves each gave a hit, the later one the nearer (every event is nearer than the one before it)."""
    return len({w for w, _, _ in events}) >= 2


# ------------------------------------------------------------------ lanes
def assignments(n_rays):
    """PERM_SEEDS permutations of which ray sits in which lane and queue position: (P, B, 64, K) int32, -1 = no ray.  Most
    lanes carry K rays; some carry 0, 1 or 2, so that waves are partial from the start and lanes run dry at different times."""
    out = []
    blocks = None
    for seed in PERM_SEEDS:
        rs = np.random.RandomState(seed)
        caps = []
        while sum(caps) < n_rays:
            caps.append(int(rs.choice([0, 1, 2, K, K, K, K, K])))
        caps += [0] * (-len(caps) % 64)
        blocks = max(blocks or 0, len(caps) // 64)
        out.append(caps)
    table = np.full((len(PERM_SEEDS), blocks, 64, K), -1, dtype=np.int32)
    for p, (seed, caps) in enumerate(zip(PERM_SEEDS, out)):
        order = np.random.RandomState(seed + 1).permutation(n_rays)
        at = 0
        for lane, cap in enumerate(caps):
            take = order[at:at + cap]
            table[p, lane // 64, lane % 64, :len(take)] = take
            at += len(take)
        assert at == n_rays
    return table


def write_case(path, scene_bytes, rows, table):
    """The input files of one case directory (scene.bin's bytes come from test_tree_host.write_scene's format)."""
    path.mkdir(parents=True, exist_ok=True)
    (path / "scene.bin").write_bytes(scene_bytes)
    np.ascontiguousarray(rows, dtype=np.float64).tofile(path / "rays.in")
    np.array(SCHEDULES, dtype=np.int32).tofile(path / "sched.in")
    with open(path / "assign.in", "wb") as f:
        f.write(struct.pack("<3i", table.shape[0], table.shape[1], table.shape[3]))
        f.write(np.ascontiguousarray(table, dtype=np.int32).tobytes())
