"""The device-built CR_BVH_LBVH tree against an independent CPU build (tests/lbvh_model.py, itself pinned on the CPU by
tests/test_lbvh_model_host.py): cr_export_bvh's children and boxes must equal the model's exactly, in f32 and f64.

The other checks of this mode cannot see a build that is merely worse: the bit-exact renders hand the exported tree to
the oracle, which then walks whatever the device built, and the well-formedness test accepts any proper tree with
enclosing boxes.  A key kernel that returns 0, swapped axes, a sort over the wrong bits or an unstable one, boxes
that are supersets of the true unions, a mix-up of sorted position and prims index: all of them cost speed, none a
pixel.  Here every one of them changes `children` or `boxes`.  No tolerance anywhere."""
import time

import numpy as np
import pytest

import lbvh_model as M
import scenes
from crucible_amd import _abi as A
from crucible_amd.demo_builder import book1_end_scene, load_teapot, million_spheres

pytestmark = pytest.mark.gpu

REALS = [(A.CR_REAL_F64, np.float64), (A.CR_REAL_F32, np.float32)]
REAL_IDS = ["f64", "f32"]
S, T, L, B, HID, MEM = M.SPHERE, M.TRIANGLE, M.LIST, M.BVH, M.HIDDEN, M.MEMBER


# ------------------------------------------------------------------ scenes
def spheres(centres, radii, flags=None):
    centres = np.asarray(centres, dtype=np.float64)
    v = np.zeros((len(centres), 9))
    v[:, 0:3] = centres
    v[:, 3] = radii
    return scenes.ArrayScene(np.zeros(len(centres), dtype=np.int32), v, flags)


def random_spheres(n, seed=1, half=50.0):
    rng = np.random.RandomState(seed)
    return spheres(rng.uniform(-half, half, (n, 3)), rng.uniform(0.05, 0.5, n))


def concentric(hide_every_third=False):
    """300 spheres around one point: every key equal, the run longer than one block of the sort."""
    n = 300
    flags = np.where(np.arange(n) % 3 == 1, HID, 0) if hide_every_third else None
    return spheres(np.tile([0.5, -1.25, 2.0], (n, 1)), 0.1 + 0.01 * np.arange(n), flags)


def flat_in(axes, n=200, seed=3):
    """Random centres that vary along `axes` only (one radius, so the box midpoints have no extent elsewhere)."""
    rng = np.random.RandomState(seed)
    c = np.tile([0.5, -2.0, 4.0], (n, 1))
    for a in axes:
        c[:, a] = rng.uniform(-8, 8, n)
    return spheres(c, 0.25)


def two_points():
    rng = np.random.RandomState(4)
    pts = np.array([[1.0, 2.0, 3.0], [-2.0, 0.5, 7.0]])
    return spheres(pts[rng.randint(0, 2, 40)], 0.25)


def clamped_ends():
    """Spheres whose centre differs from the midpoint of their box by a rounding, in both real types: one holds the
    minimum of x with its midpoint above its centre, one the maximum with its midpoint below -- their u falls an ulp
    outside [0, 1] and is clamped.  The same on y and z; ordinary spheres in between."""
    rng = np.random.RandomState(9)

    def mid(c, r, real):
        c, r = real(c), real(r)
        return 0.5 * (np.float64(c + (-r)) + np.float64(c + r))

    def find(lo, hi, want_above):
        for _ in range(100000):     # c - r and c + r straddle |x| = 8: their roundings differ, so they do not cancel
            c, r = rng.uniform(lo, hi), rng.uniform(0.5, 0.9)
            if all((mid(c, r, real) > np.float64(real(c))) == want_above and mid(c, r, real) != np.float64(real(c))
                   for real in (np.float32, np.float64)):
                return c, r
        raise AssertionError("no such sphere found")
    cen = rng.uniform(-5, 5, (60, 3))
    rad = rng.uniform(0.1, 0.9, 60)
    for a in range(3):      # sphere 2a holds the minimum of axis a, sphere 2a + 1 the maximum
        c, r = find(-8.4, -7.6, True)
        cen[2 * a] = [c, c, c]
        rad[2 * a] = r
        cen[2 * a, (a + 1) % 3], cen[2 * a, (a + 2) % 3] = 0.3, -0.7
        c, r = find(7.6, 8.4, False)
        cen[2 * a + 1] = [c, c, c]
        rad[2 * a + 1] = r
        cen[2 * a + 1, (a + 1) % 3], cen[2 * a + 1, (a + 2) % 3] = -0.2, 0.9
    return spheres(cen, rad)


def lattice():
    """17 x 17 x 17 points, 1 to 4 primitives on each (spheres of several radii, triangles whose box is centred on the
    point), the list shuffled: many equal keys whose order only a stable sort by (key, position) reproduces."""
    rng = np.random.RandomState(17)
    g = np.arange(17) * 0.5 - 4.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    reps = rng.randint(1, 5, len(pts))
    p = np.repeat(pts, reps, axis=0)
    p = p[rng.permutation(len(p))]
    n = len(p)
    kind = (rng.uniform(size=n) < 0.3).astype(np.int32)
    v = np.zeros((n, 9))
    v[:, 0:3] = p
    v[:, 3] = rng.choice([0.0625, 0.125, 0.1875], n)
    d = 0.125
    tri = kind == T
    v[tri] = (np.tile(p[tri], (1, 3)) + np.array([-d, -d, d, d, d, -d, d, -d, -d]))
    sc = scenes.ArrayScene(kind, v, width=48, samples=2)
    sc.scene_cam.look_from((3.0, 5.0, 14.0))
    sc.scene_cam.look_at((0.0, 0.0, 0.0))
    sc.scene_cam.set_vfov(45.0)
    return sc


def mixed():
    """Spheres among long thin triangles (box midpoint far from the vertex mean), hidden primitives interleaved, a HitList
    element and a CR_PRIM_BVH element with hidden members; the list's members stand BEFORE their record, so sorted
    position, source position and prims index all differ."""
    rng = np.random.RandomState(23)
    kind, flags, rows = [], [], []

    def sphere(fl):
        kind.append(S)
        flags.append(fl)
        rows.append(list(rng.uniform(-6, 6, 3)) + [rng.uniform(0.1, 0.6)] + [0.0] * 5)

    def triangle(fl):
        a = rng.uniform(-6, 6, 3)
        kind.append(T)
        flags.append(fl)
        rows.append(list(a) + list(a + rng.uniform(-0.1, 0.1, 3)) + list(a + rng.uniform(2, 5, 3) * rng.choice([-1, 1], 3)))

    def record(k, first, count):
        kind.append(k)
        flags.append(0)
        rows.append([float(first), float(count)] + [0.0] * 7)
    for i in range(7):                          # objects of the list, ahead of its record
        (sphere if i % 2 else triangle)(MEM | (HID if i in (0, 3) else 0))
    for i in range(30):
        (sphere if i % 3 else triangle)(HID if i % 4 == 1 else 0)
    record(L, 0, 7)
    for i in range(12):
        (triangle if i % 3 else sphere)(HID if i % 5 == 2 else 0)
    first = len(kind) + 1
    record(B, first, 9)
    for i in range(9):
        (sphere if i % 2 else triangle)(MEM | (HID if i in (1, 2, 8) else 0))
    for i in range(10):
        sphere(HID if i == 9 else 0)
    return scenes.ArrayScene(kind, np.array(rows), flags)


def f32_collisions():
    """Centres distinct in f64 and equal in f32 (offsets below half an f32 ulp), and f64 neighbours that f32 reorders: the
    two real types must give different trees."""
    rng = np.random.RandomState(31)
    base = rng.uniform(1, 9, (40, 3))
    c = np.repeat(base.astype(np.float32).astype(np.float64), 4, axis=0)
    c += rng.uniform(-1, 1, c.shape) * 2.0 ** -27
    return spheres(c[rng.permutation(len(c))], 0.25)


def huge(scale):
    rng = np.random.RandomState(37)
    c = rng.uniform(-1, 1, (50, 3)) * scale
    c[:6] = [[scale, 0, 0], [-scale, 0, 0], [0, scale, -scale], [0, -scale, scale], [1.0, 2.0, 3.0], [scale, scale, scale]]
    return spheres(c, rng.uniform(0.1, 2.0, 50))


def teapot():
    return load_teapot(1, image_width=32, samples=1)


SCENES = {
    "n1": lambda: scenes.few_spheres(1), "n2": lambda: scenes.few_spheres(2), "n3": lambda: scenes.few_spheres(3),
    "n4": lambda: scenes.few_spheres(4), "n5": lambda: scenes.few_spheres(5),
    "concentric": concentric, "concentric_hidden": lambda: concentric(True),
    "coplanar_x": lambda: flat_in((1, 2)), "coplanar_y": lambda: flat_in((0, 2)), "coplanar_z": lambda: flat_in((0, 1)),
    "collinear": lambda: flat_in((1,)), "two_points": two_points, "clamped_ends": clamped_ends,
    "lattice": lattice, "mixed": mixed, "f32_collisions": f32_collisions,
    "huge_1e300": lambda: huge(1e300), "huge_1.5e308": lambda: huge(1.5e308), "beyond_f32": lambda: huge(1e39),
    "book1": lambda: book1_end_scene(1, scene_seed=2, image_width=32, samples=1), "mixed_scene": lambda: scenes.mixed_scene(32, 1),
    "teapot": teapot, "moving": lambda: scenes.moving_scene(32, 1),
    "r255": lambda: random_spheres(255), "r256": lambda: random_spheres(256), "r257": lambda: random_spheres(257),
    "r4095": lambda: random_spheres(4095), "r4097": lambda: random_spheres(4097), "r65537": lambda: random_spheres(65537),
}
LARGEST = 400000


def export(renderer, sc, mode, rt):
    sc.bvh_mode = mode
    flat = sc.flatten()
    renderer.upload_scene(flat)
    return flat, renderer.export_bvh(rt)


def assert_equal_trees(got, want, what):
    boxes, kids, axis = got
    assert kids.shape == want.children.shape, (what, kids.shape, want.children.shape)
    bad = np.nonzero((kids != want.children).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(kids)} wrappers differ in children, first {bad[0]}: {kids[bad[0]]} != {want.children[bad[0]]}"
    bad = np.nonzero((boxes != want.boxes).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(kids)} boxes differ, first {bad[0]}: {boxes[bad[0]]} != {want.boxes[bad[0]]}"
    assert np.array_equal(kids, want.children) and np.array_equal(boxes, want.boxes)
    assert (axis == -1).all()


# ------------------------------------------------------------------ the device against the model
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_lbvh_tree_equals_the_model(renderer, name, rt, real):
    sc = SCENES[name]()
    flat, got = export(renderer, sc, A.CR_BVH_LBVH, rt)
    want = M.build(flat, real)
    assert_equal_trees(got, want, name)
    # the scenes do hold what their names promise
    n_keys = len(np.unique(want.keys))
    if name.startswith("concentric") or name == "beyond_f32" and real == np.float32:
        assert n_keys == 1
    if name == "concentric_hidden":
        assert len(want.order) == 200
    if name == "two_points":
        assert n_keys == 2
    if name == "clamped_ends":
        assert want.n_clamped >= 3      # the three minima always (u < 0); at a maximum u may still round to 1.0
    if name == "lattice":
        assert n_keys == 17 ** 3 and len(want.order) > 2 * n_keys
    if name == "mixed":
        recs = M.prim_records(flat)
        assert len(want.order) < (recs["kind"] <= 1).sum() and ((recs["flags"][want.order] & MEM) != 0).sum() == 5 + 6
    if name == "huge_1.5e308" and real == np.float64:
        assert n_keys == 1      # hi - lo overflows on every axis: no extent to normalise by


def test_the_real_types_give_different_trees(renderer):
    sc = f32_collisions()
    flat, (b64, k64, _) = export(renderer, sc, A.CR_BVH_LBVH, A.CR_REAL_F64)
    b32, k32, _ = renderer.export_bvh(A.CR_REAL_F32)
    assert not np.array_equal(k64, k32)
    assert len(np.unique(M.build(flat, np.float32).keys)) < len(np.unique(M.build(flat, np.float64).keys))


def test_non_finite_coordinates_are_rejected(renderer):
    """cr_upload_scene takes any finite f64 coordinate (the huge scenes above) and refuses the others."""
    from crucible_amd.renderer import CrucibleError
    for bad in (np.inf, -np.inf, np.nan):
        sc = spheres([[0.0, 1.0, 2.0], [bad, 0.0, 0.0]], 0.5)
        sc.bvh_mode = A.CR_BVH_LBVH
        with pytest.raises(CrucibleError):
            renderer.upload_scene(sc.flatten())


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_largest_full_compare(renderer, rt, real):
    """400000 random spheres, children and boxes compared in full.  The size is the largest at which the model stays
    within a few seconds: measured 1.6 s per real type on one CPU core (0.6 s at 200000, 0.3 s at 65537), against
    about a second for the export itself; the times of this run are printed."""
    sc = random_spheres(LARGEST, seed=2, half=200.0)
    t0 = time.time()
    flat, got = export(renderer, sc, A.CR_BVH_LBVH, rt)
    t1 = time.time()
    want = M.build(flat, real)
    print(f"n = {LARGEST}: upload + export {t1 - t0:.2f} s, model {time.time() - t1:.2f} s")
    assert_equal_trees(got, want, "largest")


@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_million_spheres_order_and_boxes(renderer, rt, real):
    """Too large to model wrapper by wrapper; what vectorises: the leaves of the exported tree, read left to right, are
    the model's stable sorted order; every leaf box is its primitive's box; the root box is the union of them all."""
    sc = million_spheres(1, scene_seed=1, image_width=64, samples=1)
    flat, (boxes, kids, axis) = export(renderer, sc, A.CR_BVH_LBVH, rt)
    order, keys, pbox, _ = M.sort_and_keys(flat, real)
    assert len(kids) == 2 * len(order) - 1 and (axis == -1).all()
    leaf = kids[:, 0] < 0
    assert np.array_equal(kids[leaf, 0], kids[leaf, 1])
    assert np.array_equal(~kids[leaf, 0], order)        # walk order visits the leaves left to right
    assert np.array_equal(boxes[leaf], pbox.astype(np.float64))
    root = np.empty(6)
    root[0::2], root[1::2] = pbox[:, 0::2].min(axis=0), pbox[:, 1::2].max(axis=0)
    assert np.array_equal(boxes[0], root)
    # inner wrappers: children follow their parent, the left one directly
    inner = np.nonzero(~leaf)[0]
    assert np.array_equal(kids[inner, 0], inner + 1) and (kids[inner, 1] > kids[inner, 0]).all()


# ------------------------------------------------------------------ export order and rebuilds
def test_export_order_and_rebuilds(renderer):
    """The build's device buffers are reused from one build to the next: neither the order of the two exports nor the
    scenes built in between may show."""
    a, b = SCENES["mixed"](), random_spheres(4097, seed=8)
    want = {}
    for sc, tag in ((a, "a"), (b, "b")):
        sc.bvh_mode = A.CR_BVH_LBVH
        for rt, real in REALS:
            want[tag, rt] = M.build(sc.flatten(), real)
    F64, F32 = A.CR_REAL_F64, A.CR_REAL_F32
    for tag, sc, first, second in (("a", a, F32, F64), ("b", b, F64, F32), ("a", a, F64, F32), ("b", b, F32, F64), ("a", a, F32, F64)):
        renderer.upload_scene(sc.flatten())
        for rt in (first, second, first):
            assert_equal_trees(renderer.export_bvh(rt), want[tag, rt], f"scene {tag}, real type {rt}")


# ------------------------------------------------------------------ boxes of the host-built trees
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("mode", [A.CR_BVH_SAH, A.CR_BVH_SAH_ORDERED], ids=["sah", "ordered"])
@pytest.mark.parametrize("name", ["mixed", "book1", "mixed_scene", "teapot", "moving"])
def test_sah_boxes_are_the_unions_of_their_primitives(renderer, name, mode, rt, real):
    """The topology of CR_BVH_SAH / _ORDERED is a host builder's, pinned wrapper for wrapper by its own model
    (tests/sah_model.py, tests/test_gpu_sah_build.py); independently of that model, the boxes it exports are recomputed
    here from its own `children`: every wrapper's box is the union of its primitives' boxes in the real type."""
    sc = SCENES[name]()
    flat, (boxes, kids, axis) = export(renderer, sc, mode, rt)
    recs = M.prim_records(flat)
    pbox = M.prim_boxes(recs["kind"], recs["v"], real)     # by prims index (records of lists are never named)
    named = np.unique(~kids[kids < 0])
    assert np.array_equal(named, np.sort(M.visible_prims(recs)))
    want = M.union_boxes(kids, lambda i: pbox[i], real)
    bad = np.nonzero((boxes != want).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(kids)} boxes differ, first {bad[0]}: {boxes[bad[0]]} != {want[bad[0]]}"


# ------------------------------------------------------------------ the render, on the model's tree
@pytest.mark.parametrize("rt,real", REALS, ids=REAL_IDS)
def test_render_matches_the_oracle_walking_the_model_tree(renderer, oracles, rt, real):
    """The bit-exact LBVH renders elsewhere hand the oracle the EXPORTED tree; here it walks the model's, so image and
    work counters are pinned to a tree the device had no part in."""
    sc = lattice()
    sc.bvh_mode = A.CR_BVH_LBVH
    flat = sc.flatten()
    renderer.upload_scene(flat)
    img, st = renderer.render(sc.scene_cam, seed=0xC0FFEE, real_type=rt)
    want = M.build(flat, real)
    tree = (want.boxes, want.children, np.full(len(want.children), -1, dtype=np.int32))
    ref, rst = oracles[rt].render_image(sc, seed=0xC0FFEE, tree=tree)
    assert np.array_equal(img, ref), f"differing px = {(img != ref).any(axis=2).sum()}"
    for k in ("segments", "node_tests", "prim_tests", "texel_fetches"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["bvh_entries"] == len(want.children)
    assert st["prim_tests"] > 0 and (img != img[0, 0]).any()      # the camera does see the lattice
