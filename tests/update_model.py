"""What tests/test_update_abi.py and tests/test_gpu_update.py share: seeded edits of a flattened scene, an independent
numpy model of a wrapper tree's construction-time boxes, and oracle renders of an edited description.

The box model is the rule cr_update_primitives promises for CR_UPDATE_REFIT (include/crucible_hip.h): a primitive's box
is Sphere::new's / Triangle::new's in `real` (sphere.rs:29-30, triangle.rs:28-35), a wrapper's box the tight_enclose
(utils.rs:629-633) of its two children, bottom-up over the exported `children` array.  test_update_abi.py holds it
against the oracle's own reference-built tree before the GPU tests rely on it."""
import ctypes as C

import numpy as np

from crucible_amd import _abi as A

EDIT_SEED = 1   # of seeded_edit in both test files: moves spheres and triangles of mixed_scene and moving_scene, changes two radii


def prim_arrays(flat):
    """(kind (n,), flags (n,), v (n, 9) float64) of a FlatScene's primitive list."""
    n = flat.desc.n_prims
    kind = np.array([flat.prims[i].kind for i in range(n)], dtype=np.int32)
    flags = np.array([flat.prims[i].flags for i in range(n)], dtype=np.int32)
    v = np.array([list(flat.prims[i].v) for i in range(n)], dtype=np.float64).reshape(n, 9)
    return kind, flags, v


def seeded_edit(flat, seed, fraction=1.0 / 3.0, shift=2.5, skip=(0,)):
    """About `fraction` of the spheres and triangles (never those in `skip`: the ground) moved by up to `shift` units
    per axis, every other chosen sphere also with a new radius (x 0.6 .. 1.5), a triangle's vertices each jittered by up
    to 0.2 on top of the common move.  A triangle that is flat along an axis is always chosen: alone in a leaf its
    zero-thickness box never hits (bvh.rs:126), which no list without boxes reproduces, and the jitter tilts it -- so the
    edited scene can be held against the oracle's linear list.
    Returns (indices int32 (m,), rows float64 (m, 9)): cr_update_primitives' arguments."""
    kind, _, v = prim_arrays(flat)
    rs = np.random.RandomState(seed)
    idx, rows = [], []
    for i in range(len(kind)):
        pick = rs.uniform() < fraction
        d = rs.uniform(-shift, shift, 3)
        f = rs.uniform(0.6, 1.5)
        grow = rs.uniform() < 0.5
        jitter = rs.uniform(-0.2, 0.2, 9)
        if i in skip or kind[i] not in (A.CR_PRIM_SPHERE, A.CR_PRIM_TRIANGLE):
            continue
        row = v[i].copy()
        if kind[i] == A.CR_PRIM_SPHERE:
            if not pick:
                continue
            row[:3] += d
            if grow:
                row[3] *= f
            row[4:] = np.nan                   # a sphere reads four values: the rest must be ignored
        else:
            pts = row.reshape(3, 3)
            if not pick and (pts.max(axis=0) > pts.min(axis=0)).all():
                continue
            row += np.tile(d, 3) + jitter
        idx.append(i)
        rows.append(row)
    assert idx, "the edit chose nothing: pick another seed"
    return np.array(idx, dtype=np.int32), np.array(rows, dtype=np.float64).reshape(-1, 9)


def apply_edit(flat, idx, rows):
    """The edited description: the rows written into the FlatScene's own primitive list, as the call defines it (a
    sphere takes four values and keeps the others)."""
    for i, row in zip(idx, rows):
        p = flat.prims[int(i)]
        nv = 4 if p.kind == A.CR_PRIM_SPHERE else 9
        for k in range(nv):
            p.v[k] = float(row[k])
    return flat


def prim_box(kind, v, dtype):
    """Construction-time box (lo (3,), hi (3,)) of one primitive, computed in `dtype`.  A sphere's is Aabb::new_from_points
    (bvh.rs:44-64) of centre - r and centre + r, a compare and select: when one of them is not a number (inf - inf, an f32
    centre and radius that are both infinite) the comparison fails and the box is (centre + r, centre - r).  A triangle's is
    f64::min / f64::max over the vertices (triangle.rs:28-35), which pass over a NaN."""
    with np.errstate(over="ignore", invalid="ignore"):       # coordinates beyond the range of `dtype` become infinite, as on the device
        g = np.asarray(v, dtype=np.float64).astype(dtype)
        if kind == A.CR_PRIM_SPHERE:
            r = g[3]
            a, b = g[:3] + (-r), g[:3] + r
            ordered = a <= b
            return np.where(ordered, a, b), np.where(ordered, b, a)
    pts = g.reshape(3, 3)
    return np.fmin.reduce(pts, axis=0), np.fmax.reduce(pts, axis=0)


def tight_enclose(lo, hi, clo, chi):
    """Interval::tight_enclose (utils.rs:629-633) per axis: `a.min <= b.min ? a.min : b.min`, `a.max >= b.max ? a.max : b.max`.
    Not np.minimum / np.maximum: a comparison with a NaN fails, so the second operand's NaN is taken and the first's dropped."""
    with np.errstate(invalid="ignore"):
        return np.where(lo <= clo, lo, clo), np.where(hi >= chi, hi, chi)


def model_boxes(children, kind, v, dtype):
    """boxes (n, 6) in `dtype` (xmin, xmax, ymin, ymax, zmin, zmax) of the wrapper tree `children` (cr_export_bvh's
    shape: >= 0 a wrapper, < 0 the complement of a primitive's index; children are numbered after their parent): a
    wrapper's box is the tight_enclose of its left child's box and its right child's, in that order (bvh.rs:67-73)."""
    n = len(children)
    lo = np.full((n, 3), np.inf, dtype=dtype)
    hi = np.full((n, 3), -np.inf, dtype=dtype)
    for k in range(n - 1, -1, -1):
        for c in children[k]:
            if c >= 0:
                assert c > k
                clo, chi = lo[c], hi[c]
            else:
                clo, chi = prim_box(kind[~c], v[~c], dtype)
            lo[k], hi[k] = tight_enclose(lo[k], hi[k], clo, chi)
    boxes = np.empty((n, 6), dtype=dtype)
    boxes[:, 0::2] = lo
    boxes[:, 1::2] = hi
    return boxes


def oracle_tree(o, flat, cam=None, seed=0):
    """The oracle's own reference-built tree of `flat`: (boxes (n, 6) in the oracle's real, children (n, 2) in
    cr_export_bvh's shape).  oracle_bvh_dump numbers wrappers in walk order, marks a wrapper child -1 and names a
    primitive by its index; the wrapper indices follow from the walk order.
    cam: the boxes the oracle walks for that camera's frame -- the refitted ones with cam.refit_boxes -- instead of the
    construction-time ones (oracle_render leaves the boxes of its frame in the scene: a one-pixel render sets them)."""
    h = o.scene_create(flat)
    try:
        if cam is not None:
            o.render(h, cam, seed=seed, pix_begin=0, pix_end=1, n_threads=1)
        cap = 2 * max(1, flat.desc.n_prims) + 8
        boxes = np.zeros((cap, 6), dtype=o.np_real)
        kids = np.zeros((cap, 2), dtype=np.int32)
        n = o.lib.oracle_bvh_dump(h, boxes.ctypes.data, kids.ctypes.data, cap)
    finally:
        o.scene_destroy(h)
    boxes, kids = boxes[:n], kids[:n]
    children = np.where(kids >= 0, ~kids, 0).astype(np.int32)
    size = np.ones(n, dtype=np.int64)          # wrappers in the subtree of k, itself included
    for k in range(n - 1, -1, -1):
        nxt = k + 1
        for side in (0, 1):
            if kids[k, side] == -1:
                children[k, side] = nxt
                nxt += size[nxt]
        size[k] = nxt - k
    return boxes, children


def oracle_render_flat(o, flat, cam, *, seed, tree=None, linear_list=False, sum_order=A.CR_SUM_REFERENCE_ORDER):
    """Oracle.render_image for a description that exists only as a FlatScene (an edited one)."""
    h = o.scene_create(flat)
    try:
        if tree is not None:
            o.set_tree(h, *tree)
        if linear_list:
            o.lib.oracle_use_list(h)
        out, st = o.render(h, cam, seed=seed, sum_order=sum_order)
    finally:
        o.scene_destroy(h)
    return out.reshape(cam.image_height, cam.image_width, 3), st


def update_call(lib, handle, idx, rows, flags, n=None, group=False):
    """The raw C call (for the cases Renderer.update_primitives would refuse to build arguments for)."""
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    if n is None:
        n = 0 if rows is None else rows.size // 9
    fn = lib.cr_group_update_primitives if group else lib.cr_update_primitives
    return fn(handle, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)),
              None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_double)), n, flags)
