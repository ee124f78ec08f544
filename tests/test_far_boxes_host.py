"""What the scenes of tests/far_corpus.py contain, from the oracle and numpy alone, so that tests/test_gpu_far_boxes.py
cannot pass vacuously.

The f64 megakernels may decide a box test on the box rounded to f32 only while no finite plane of the tree becomes infinite
by the rounding (screen_plane, pathtrace.hpp).  A walk that screened on such a tree anyway would count box hits that
Aabb::hit does not: more node_tests, which every GPU test pins against the oracle.  Asserted here, per far scene: the
oracle's own tree has (wrapper, primary ray) pairs on which Aabb::hit of the rounded box differs from Aabb::hit of the box,
on leaf and on inner wrappers; the scenes that must stay screenable have none.  Measured (oracle's tree, 32 x 24 x 2 primary
rays): far 975 pairs (325 on a leaf wrapper, 650 on inner ones), edge_out 684 (342, 342), keyed at its far frame 975 (650,
325); edge_in, near and keyed at frames 0 and 2: 0.

The frames are not degenerate, the oracle's tree of every scene (edited ones included) meets the linear-list cap of
tests/test_gpu_refit.py (all of them at 100 % of the pixels, in both precisions), and tests/update_model.py's box model
follows the oracle's rule where a plane is inf - inf."""
import ctypes as C

import numpy as np
import pytest

import far_corpus as F
import update_model as um
from crucible_amd import _abi as A

REALS = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
REAL_IDS = ["f64", "f32"]
SEED = 3838
MIN_PAIRS = 20
CAP = 0.995                                    # tests/test_gpu_refit.py
# (scene, frame): must the screen be unusable there?
CASES = [("far", 0, True), ("edge_in", 0, False), ("edge_out", 0, True), ("near", 0, False),
         ("keyed", 0, False), ("keyed", F.KEYED_FAR_FRAME, True), ("keyed", 2, False)]
CASE_IDS = [f"{n}-{f}" for n, f, _ in CASES]


def overflowing(boxes):
    """Per wrapper: a finite plane that is infinite in f32."""
    with np.errstate(over="ignore"):
        return (np.isfinite(boxes) & np.isinf(boxes.astype(np.float32))).any(axis=1)


@pytest.mark.parametrize("name,frame,far", CASES, ids=CASE_IDS)
def test_rounded_boxes_decide_differently_exactly_on_the_far_trees(o64, name, frame, far):
    sc = F.scene(name, frame)
    cam = sc.scene_cam
    boxes, children = um.oracle_tree(o64, sc.flatten(), cam, SEED)           # the boxes of this frame: refitted for "keyed"
    rays = F.primary_rays(o64, cam, SEED)
    assert len(rays) == F.WIDTH * F.HEIGHT * F.SAMPLES
    counts, leaf = F.screen_disagreements(boxes, children, rays)
    print(f"{name} frame {frame}: {int(counts.sum())} disagreeing (wrapper, ray) pairs, {int(counts[leaf].sum())} on leaf wrappers, "
          f"{int(counts[~leaf].sum())} on inner wrappers; {int(overflowing(boxes).sum())} of {len(boxes)} wrappers overflow")
    assert overflowing(boxes).any() == far
    if far:
        assert counts.sum() >= MIN_PAIRS and counts[leaf].sum() >= 1 and counts[~leaf].sum() >= 1, (counts, leaf)
        assert (counts[~overflowing(boxes)] == 0).all()                       # and only where a plane overflows
    else:
        assert counts.sum() == 0, counts


def test_boundary_pair_differs_in_one_plane_on_either_side_of_the_f32_range(o64):
    inside, outside = F.largest_plane("edge_in"), F.largest_plane("edge_out")
    with np.errstate(over="ignore"):
        assert not np.isinf(np.float32(inside)) and np.isinf(np.float32(outside))
    assert float(np.float32(inside)) == inside and outside > inside           # FLT_MAX itself, and a double above it
    assert np.nextafter(outside, 0.0) > inside                               # doubles between them round down to FLT_MAX ...
    with np.errstate(over="ignore"):
        assert not np.isinf(np.float32(np.nextafter(outside, 0.0)))          # ... the one below `outside` is the last to do so
    flats = [F.scene(n).flatten() for n in ("edge_in", "edge_out")]
    v = [um.prim_arrays(f)[2] for f in flats]
    diff = np.argwhere(v[0] != v[1])
    assert len(diff) == 1 and v[0][tuple(diff[0])] == inside and v[1][tuple(diff[0])] == outside
    trees = [um.oracle_tree(o64, f) for f in flats]
    assert np.array_equal(trees[0][1], trees[1][1])
    assert trees[0][0].max() == inside and trees[1][0].max() == outside
    assert np.array_equal(trees[0][0] == inside, trees[1][0] == outside) and np.array_equal(trees[0][0][trees[0][0] != inside], trees[1][0][trees[1][0] != outside])


def first_hits(o, sc, seed):
    """Per pixel and sample: the material of the primary ray's first hit, -1 for the sky ((H, W, samples) int32)."""
    cam = sc.scene_cam
    flat = sc.flatten()
    rays = F.primary_rays(o, cam, seed)
    h = o.scene_create(flat)
    try:
        o.render(h, cam, seed=seed, pix_begin=0, pix_end=1, n_threads=1)    # the boxes of the frame (tests/test_gpu_aov.py's model)
        out = np.full(len(rays), -1, dtype=np.int32)
        rec, mat = np.zeros(10, dtype=o.np_real), C.c_int32()
        for k, ray in enumerate(rays):
            orig, dirn = np.ascontiguousarray(ray[0:3]), np.ascontiguousarray(ray[3:6])
            if o.lib.oracle_world_hit(h, orig.ctypes.data_as(C.c_void_p), dirn.ctypes.data_as(C.c_void_p), o.real(ray[6]), o.real(0.001),
                                      o.real(np.inf), rec.ctypes.data_as(C.c_void_p), C.byref(mat)):
                out[k] = mat.value
    finally:
        o.scene_destroy(h)
    return out.reshape(cam.image_height, cam.image_width, cam.samples), flat


@pytest.mark.parametrize("name,frame", [(n, 0) for n in F.STATIC] + [("keyed", f) for f in F.KEYED_FRAMES],
                         ids=list(F.STATIC) + [f"keyed-{f}" for f in F.KEYED_FRAMES])
def test_frames_are_not_degenerate(o64, name, frame):
    sc = F.scene(name, frame)
    img, st = um.oracle_render_flat(o64, sc.flatten(), sc.scene_cam, seed=SEED)
    assert st["nan_pixels"] == 0 and np.isfinite(img).all()
    hits, flat = first_hits(o64, sc, SEED)
    near = sorted({flat.prims[i].material for i in range(1 + F.N_SPHERES + F.N_TRIANGLES)})
    share = np.isin(hits, near).any(axis=2).mean()
    print(f"{name} frame {frame}: {share:.3f} of the pixels hit the near cluster, {(hits < 0).all(axis=2).mean():.3f} see only sky")
    assert 0.10 <= share <= 0.90, share
    if name == "far":
        backdrop = flat.prims[flat.desc.n_prims - 1]
        assert backdrop.kind == A.CR_PRIM_TRIANGLE and abs(backdrop.v[0]) == 1e39 and backdrop.material not in near
        n = int((hits == backdrop.material).any(axis=2).sum())
        print(f"the backdrop is the first hit in {n} pixels")
        assert n >= 1


def edited_near():
    sc = F.scene("near")
    flat = sc.flatten()
    idx, rows, _ = F.hostile_edit(flat)
    return sc, um.apply_edit(flat, idx, rows)


def cap_cases():
    for name, frame, _ in CASES:
        yield f"{name}-{frame}", (lambda name=name, frame=frame: (F.scene(name, frame), None))
    yield "near-edited", edited_near


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("what,make", list(cap_cases()), ids=[w for w, _ in cap_cases()])
def test_oracle_tree_meets_the_linear_list_cap(oracles, rt, tag, what, make):
    """The bar the GPU tests hold the device's trees to is one the oracle's own tree of these scenes meets, the refitted
    frames of "keyed" and the hostile edit of "near" included: the far primitives do not put near ones out of reach."""
    sc, flat = make()
    flat = flat or sc.flatten()
    o = oracles[rt]
    tree, _ = um.oracle_render_flat(o, flat, sc.scene_cam, seed=SEED)
    truth, _ = um.oracle_render_flat(o, flat, sc.scene_cam, seed=SEED, linear_list=True)
    assert np.array_equal(np.isnan(tree), np.isnan(truth))
    same = ((tree == truth) | np.isnan(tree)).all(axis=2).mean()
    print(f"{what} {tag}: {same:.5f} of the pixels equal the linear list's")
    assert same >= CAP, same


# ---------------------------------------------------------------- the box model on the hostile rows
def same_boxes(got, want, what):
    """NaN planes in the same places, every other plane equal."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN planes differ at {np.argwhere(gn != wn)[:4].tolist()}"
    assert np.array_equal(got[~gn], want[~wn]), f"{what}: wrappers {np.unique(np.argwhere((got != want) & ~gn)[:, 0])[:8].tolist()} differ"


def test_hostile_edit_holds_what_it_promises():
    flat = F.scene("near").flatten()
    kind, _, v = um.prim_arrays(flat)
    idx, rows, back = F.hostile_edit(flat)
    assert len(set(idx.tolist())) == len(idx) and 0 not in idx
    sph = kind[idx] == A.CR_PRIM_SPHERE
    assert np.isfinite(rows[sph, :4]).all() and np.isnan(rows[sph, 4:]).all() and np.isfinite(rows[~sph]).all()   # validate_update reads these
    assert (rows[sph, 3] >= 0).all()
    r = rows[sph, 3]
    with np.errstate(over="ignore", under="ignore"):
        assert (r == 0).any() and ((r > 0) & (r.astype(np.float32) == 0) & (r >= 2.3e-308)).any() and ((r > 0) & (r < 2.2250738585072014e-308)).any()
        c = rows[sph, :3]
        for x in (1e39, -1e39, 1e300, -1e300, F.DBL_MAX):
            assert (c == x).any(), x
        grown = c + r[:, None]
    assert (np.isinf(grown) & np.isfinite(c)).any()                          # centre + radius overflows: an infinite f64 plane
    assert (np.signbit(c) & (c == 0)).any()                                   # -0.0
    tri = rows[~sph].reshape(-1, 3, 3)
    assert any((t[0] == t[1]).all() and (t[1] == t[2]).all() for t in tri)
    assert any(not (t[0] == t[1]).all() and np.allclose(np.cross(t[1] - t[0], t[2] - t[0]), 0) for t in tri)
    assert any(np.array_equal(t, np.array(F.FAR_TRIANGLE)) for t in tri)
    um.apply_edit(flat, idx, rows)
    um.apply_edit(flat, idx, back)                                            # the inverse edit: the description as it was
    assert np.array_equal(um.prim_arrays(flat)[2], v)


def test_a_plane_that_is_not_a_number_follows_the_oracles_rule():
    """Sphere::new's box is a compare and select of centre - r and centre + r, tight_enclose one of the two boxes' planes: a
    NaN on the right of a comparison is taken, on the left it is dropped.  np.minimum / np.maximum would keep it either way."""
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        lo, hi = um.prim_box(A.CR_PRIM_SPHERE, [F.DBL_MAX, 0.0, 1.0, 1e300, 0, 0, 0, 0, 0], f32)
    assert lo.dtype == f32 and lo[0] == np.inf and np.isnan(hi[0])            # inf - inf <= inf + inf fails: (centre + r, centre - r)
    assert lo[1] == -np.inf and hi[1] == np.inf and lo[2] == -np.inf and hi[2] == np.inf
    lo, hi = um.prim_box(A.CR_PRIM_SPHERE, [F.DBL_MAX, 0.0, 1.0, 1e300, 0, 0, 0, 0, 0], np.float64)
    assert lo[0] == F.DBL_MAX - 1e300 and hi[0] == np.inf and lo[1] == -1e300  # f64: an infinite plane, no NaN
    nan, one, two = np.array([np.nan]), np.array([1.0]), np.array([2.0])
    a = um.tight_enclose(one, two, nan, nan)
    assert np.isnan(a[0]) and np.isnan(a[1])                                  # NaN on the right: taken
    b = um.tight_enclose(nan, nan, one, two)
    assert b[0] == 1.0 and b[1] == 2.0                                        # NaN on the left: dropped
    c = um.tight_enclose(one, two, np.array([0.5]), np.array([3.0]))
    assert c[0] == 0.5 and c[1] == 3.0
    with np.errstate(over="ignore"):
        lo, hi = um.prim_box(A.CR_PRIM_TRIANGLE, np.array(F.FAR_TRIANGLE).reshape(9), f32)
    assert hi[1] == np.inf and lo[0] == f32(3e38) and np.isfinite(lo).all()


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("edited", [False, True], ids=["as_built", "edited"])
def test_box_model_reproduces_the_oracle_tree_of_the_hostile_edit(oracles, rt, tag, edited):
    """On the oracle's own tree of the edited description the model gives the oracle's boxes, NaN planes in the same places.
    In f32 the row with centre DBL_MAX and radius 1e300 has a plane inf - inf; a model that took minima with np.minimum
    would differ there."""
    o = oracles[rt]
    if edited:
        _, flat = edited_near()
    else:
        flat = F.scene("far").flatten()
    boxes, children = um.oracle_tree(o, flat)
    kind, _, v = um.prim_arrays(flat)
    with np.errstate(over="ignore", invalid="ignore"):
        model = um.model_boxes(children, kind, v, o.np_real)
    same_boxes(model, boxes, tag)
    has_nan = bool(np.isnan(boxes).any())
    assert has_nan == (edited and rt == A.CR_REAL_F32)
    if has_nan:
        lo = np.full((len(children), 3), np.inf, dtype=o.np_real)
        hi = np.full((len(children), 3), -np.inf, dtype=o.np_real)
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(len(children) - 1, -1, -1):                        # the model as it was: minima that keep every NaN
                for c in children[k]:
                    clo, chi = (lo[c], hi[c]) if c >= 0 else um.prim_box(kind[~c], v[~c], o.np_real)
                    lo[k], hi[k] = np.minimum(lo[k], clo), np.maximum(hi[k], chi)
        assert not np.array_equal(np.isnan(lo), np.isnan(boxes[:, 0::2])) or not np.array_equal(np.isnan(hi), np.isnan(boxes[:, 1::2]))


@pytest.mark.parametrize("rt,tag", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("frame", F.KEYED_FRAMES)
def test_refitted_boxes_of_the_keyed_scene(oracles, rt, tag, frame):
    """The oracle's refit grows every sample box by the primitive's pad before it is judged and united (refit.hpp's order).
    In f32 the rovers' travel is infinite, so is their pad, and at the far frame inf - inf makes every sample of theirs no
    number: they get no box, and no plane of the tree is a NaN that would put a leaf's other primitive out of reach."""
    sc = F.scene("keyed", frame)
    boxes, children = um.oracle_tree(oracles[rt], sc.flatten(), sc.scene_cam, SEED)
    base, _ = um.oracle_tree(oracles[rt], sc.flatten())
    assert not np.isnan(boxes).any()
    assert not np.array_equal(boxes, base)                                    # keyed primitives: the frame's boxes are not the built ones
    if rt == A.CR_REAL_F64:
        assert overflowing(boxes).any() == (frame == F.KEYED_FAR_FRAME)
    elif frame == 0:
        assert np.isinf(boxes).any()                                          # f32: an infinite pad around the waiting rovers
