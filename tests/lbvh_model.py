"""A plain model of the CR_BVH_LBVH build, written from its definition: what cr_export_bvh must return for a flattened
scene and a real type.  numpy and Python integers only -- no GPU, none of the library's code.  The tests hold the device
build (tests/test_gpu_lbvh_build.py) and the host/device functions of crucible_amd/csrc/lbvh.hpp
(tests/test_lbvh_model_host.py) to it exactly; the whole build is integer arithmetic on a handful of exactly specified
f64 operations, so there is no tolerance anywhere.

The definition:
  (a) the visible primitives, in CrSceneDesc.prims order; a list's or CR_PRIM_BVH record's visible objects stand in for it;
  (b) their construction-time boxes in the real type (sphere: c + (-r) and c + r, ordered; triangle: min / max of the
      vertices);
  (c) centroids in f64 (sphere: its centre; triangle: the midpoint of its box) normalised to the bounds of the box
      midpoints 0.5 * (bmin + bmax);
  (d) 21 bits per axis, q = floor(clamp(u, 0, 1) * (2^21 - 1)), interleaved with x the most significant of each triple;
  (e) a stable sort by key, and the binary radix tree over the 96-bit words key << 32 | sorted position;
  (f) wrappers numbered in walk order (root, left subtree, right subtree), a leaf naming its primitive twice as
      ~(index in CrSceneDesc.prims), a wrapper's box the tight_enclose union of its children's.
"""
import sys
from bisect import bisect_left
from collections import namedtuple

import numpy as np

PRIM_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("flags", "<i4"), ("key_first", "<i4"), ("key_count", "<i4"),
                       ("_pad", "<i4"), ("v", "<f8", 9)])
SPHERE, TRIANGLE, LIST, BVH = 0, 1, 2, 3     # CrPrimitive.kind (include/crucible_hip.h)
HIDDEN, MEMBER = 1, 2                        # CrPrimitive.flags
CELLS = 2097151.0                            # 2^21 - 1

Tree = namedtuple("Tree", "children boxes order keys prim_boxes n_clamped")


def prim_records(flat):
    """The CrPrimitive records of a FlatScene as a structured array."""
    n = flat.desc.n_prims
    return np.frombuffer(flat.prims, dtype=PRIM_DTYPE, count=n) if n else np.zeros(0, dtype=PRIM_DTYPE)


def visible_prims(recs):
    """(a): indices into CrSceneDesc.prims of the primitives the tree is built over, in build order."""
    kind, flags = recs["kind"], recs["flags"]
    if not ((kind == LIST) | (kind == BVH)).any():
        return np.nonzero(((flags & (HIDDEN | MEMBER)) == 0))[0].astype(np.int64)
    out = []
    for i in range(len(recs)):
        if flags[i] & MEMBER:
            continue          # reached through its list
        if kind[i] in (LIST, BVH):
            first, count = int(recs["v"][i, 0]), int(recs["v"][i, 1])
            out += [k for k in range(first, first + count) if not flags[k] & HIDDEN]
        elif not flags[i] & HIDDEN:
            out.append(i)
    return np.asarray(out, dtype=np.int64)


def prim_boxes(kind, v, real):
    """(b): (m, 6) boxes [xlo, xhi, ylo, yhi, zlo, zhi] in `real`, from coordinates rounded to `real` first."""
    with np.errstate(over="ignore", invalid="ignore"):
        g = v.astype(real)
        box = np.zeros((len(g), 6), dtype=real)
        sph = kind == SPHERE
        c, r = g[sph, 0:3], g[sph, 3:4]
        l, u = c + (-r), c + r
        box[sph, 0::2] = np.where(l <= u, l, u)
        box[sph, 1::2] = np.where(l <= u, u, l)
        t = g[~sph].reshape(-1, 3, 3)            # [primitive, vertex, axis]
        box[~sph, 0::2] = t.min(axis=1)
        box[~sph, 1::2] = t.max(axis=1)
    return box


def interleave(qx, qy, qz):
    """(d): bit b of q lands at 3 b + 2 (x), 3 b + 1 (y), 3 b (z).  Python integers."""
    k = 0
    for b in range(21):
        k |= ((qx >> b) & 1) << (3 * b + 2) | ((qy >> b) & 1) << (3 * b + 1) | ((qz >> b) & 1) << (3 * b)
    return k


def cell(c, lo, inv_ext):
    """(d): one axis, Python floats (IEEE f64).  NaN compares false both ways and is clamped to 0 by definition."""
    u = (c - lo) * inv_ext
    if not (u >= 0.0):
        u = 0.0
    elif u > 1.0:
        u = 1.0
    return int(u * CELLS)


def morton_key(c, lo, inv_ext):
    """Key of one centroid: three f64 triples, scalar."""
    return interleave(*(cell(float(c[a]), float(lo[a]), float(inv_ext[a])) for a in range(3)))


def morton_keys(cen, lo, inv_ext):
    """The same over an (m, 3) array: uint64 keys and the number of coordinates that had to be clamped."""
    with np.errstate(over="ignore", invalid="ignore"):
        u = (cen - lo[None, :]) * inv_ext[None, :]
    outside = ~((u >= 0.0) & (u <= 1.0))
    u = np.where(u >= 0.0, np.where(u > 1.0, 1.0, u), 0.0)
    q = (u * CELLS).astype(np.uint64)
    keys = np.zeros(len(cen), dtype=np.uint64)
    for a in range(3):
        for b in range(21):
            keys |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return keys, int(outside.sum())


def centroid_bounds(box):
    """(c): lo and inv_ext of the box midpoints, in f64.  A sphere's centre is NOT always its box midpoint:
    (c - r) + (c + r) rounds, so the midpoint can sit an ulp off the centre the key is computed from, u then leaves
    [0, 1] by an ulp at the extremes of an axis and is clamped in (d)."""
    b = box.astype(np.float64)
    lo, inv_ext = np.zeros(3), np.zeros(3)
    with np.errstate(over="ignore", invalid="ignore"):
        mid = 0.5 * (b[:, 0::2] + b[:, 1::2])
        for a in range(3):
            m = mid[~np.isnan(mid[:, a]), a]       # a midpoint that is not a number bounds nothing
            l, h = (m.min(), m.max()) if len(m) else (np.inf, -np.inf)
            lo[a] = l if np.isfinite(l) else 0.0
            ext = h - l
            inv_ext[a] = 1.0 / ext if np.isfinite(ext) and h > l else 0.0
    return lo, inv_ext


def centroids(kind, v, box, real):
    """(c): f64 centroids -- a sphere's centre, the midpoint of a triangle's box."""
    b = box.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        cen = 0.5 * (b[:, 0::2] + b[:, 1::2])
        sph = kind == SPHERE
        cen[sph] = v[sph, 0:3].astype(real).astype(np.float64)
    return cen


def radix_splits(keys):
    """(e): the binary radix tree over key << 32 | position for keys sorted ascending, top-down: [a, b] splits after the
    last position whose word has a 0 at the highest bit in which word[a] and word[b] differ.  Returns the internal
    nodes as (a, b, split) in walk order (node, left subtree, right subtree); left = [a, split], right = [split + 1, b]."""
    words = [(int(k) << 32) | i for i, k in enumerate(keys)]
    out = []

    def rec(a, b):
        if a == b:
            return
        h = (words[a] ^ words[b]).bit_length() - 1
        # the words of [a, b] agree above bit h and are sorted: those with bit h clear come first
        first_set = bisect_left(words, ((words[a] >> h) | 1) << h, a, b + 1)
        out.append((a, b, first_set - 1))
        rec(a, first_set - 1)
        rec(first_set, b)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 1000))   # depth <= 96
    try:
        if len(words):
            rec(0, len(words) - 1)
    finally:
        sys.setrecursionlimit(old)
    return out


def sort_and_keys(flat, real):
    """(a)-(e) up to the order: (prims indices in sorted order, sorted keys, their boxes in sorted order, n clamped)."""
    recs = prim_records(flat)
    vis = visible_prims(recs)
    kind, v = recs["kind"][vis], recs["v"][vis]
    box = prim_boxes(kind, v, real)
    if len(vis) == 0:
        return vis, np.zeros(0, dtype=np.uint64), box, 0
    lo, inv_ext = centroid_bounds(box)
    keys, n_clamped = morton_keys(centroids(kind, v, box, real), lo, inv_ext)
    perm = np.argsort(keys, kind="stable")      # by (key, source position)
    return vis[perm], keys[perm], box[perm], n_clamped


def build(flat, real):
    """What cr_export_bvh must return for CR_BVH_LBVH: Tree(children (n, 2) int32, boxes (n, 6) float64 holding exact
    values of `real`, order = prims indices in sorted order, keys sorted, prim_boxes in sorted order, n_clamped)."""
    order, keys, pbox, n_clamped = sort_and_keys(flat, real)
    m = len(order)
    if m == 0:
        return Tree(np.zeros((0, 2), np.int32), np.zeros((0, 6)), order, keys, pbox, 0)
    n = 2 * m - 1
    # (f) walk order: the wrapper of [a, b] is followed by its left subtree, 2 (split - a) + 1 wrappers, then its right
    # one.  radix_splits lists the inner wrappers in that order already; the leaves fill the gaps.
    left, right, deep, leaf_at, leaf_prim = [], [], [], [], []
    it = iter(radix_splits(keys))
    todo = [(0, m - 1, 0)]
    pos = 0
    while todo:
        a, b, d = todo.pop()
        deep.append(d)
        if a == b:
            leaf_at.append(pos)
            leaf_prim.append(a)
            left.append(-1)
            right.append(-1)
        else:
            sa, sb, g = next(it)
            assert (sa, sb) == (a, b)
            left.append(pos + 1)
            right.append(pos + 2 * (g - a) + 2)
            todo.append((g + 1, b, d + 1))
            todo.append((a, g, d + 1))
        pos += 1
    assert pos == n
    children = np.stack([np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32)], axis=1)
    depth = np.asarray(deep, dtype=np.int32)
    boxes = np.zeros((n, 6), dtype=real)
    children[leaf_at] = (~order[leaf_prim]).astype(np.int32)[:, None]
    boxes[leaf_at] = pbox[leaf_prim]
    # boxes bottom-up, a depth at a time: Interval::tight_enclose keeps the left value on a tie
    inner = np.asarray(left) >= 0
    for d in range(int(depth.max()), -1, -1):
        idx = np.nonzero(inner & (depth == d))[0]
        if len(idx) == 0:
            continue
        l, r = boxes[children[idx, 0]], boxes[children[idx, 1]]
        boxes[idx, 0::2] = np.where(l[:, 0::2] <= r[:, 0::2], l[:, 0::2], r[:, 0::2])
        boxes[idx, 1::2] = np.where(l[:, 1::2] >= r[:, 1::2], l[:, 1::2], r[:, 1::2])
    return Tree(children, boxes.astype(np.float64), order, keys, pbox, n_clamped)


def union_boxes(children, leaf_box_of, real):
    """Boxes of an exported wrapper tree recomputed from its own `children`: a leaf wrapper's box is the tight_enclose
    union of the boxes of the primitives it names (leaf_box_of: prims index -> box in `real`), an inner wrapper's the
    union of its children's.  Children follow their parents in walk order, so one backward pass does it."""
    n = len(children)
    boxes = np.zeros((n, 6), dtype=real)
    for k in range(n - 1, -1, -1):
        c0, c1 = int(children[k, 0]), int(children[k, 1])
        l, r = (boxes[c0], boxes[c1]) if c0 >= 0 else (leaf_box_of(~c0), leaf_box_of(~c1))
        boxes[k, 0::2] = np.where(l[0::2] <= r[0::2], l[0::2], r[0::2])
        boxes[k, 1::2] = np.where(l[1::2] >= r[1::2], l[1::2], r[1::2])
    return boxes.astype(np.float64)
