"""A plain model of the CR_BVH_SAH / CR_BVH_SAH_ORDERED build, written from its definition: what cr_export_bvh must
return for a flattened scene and a real type.  numpy and Python integers only -- no GPU, none of the library's code.
tests/test_sah_model_host.py pins it on the CPU (hand-worked trees, a brute-force recomputation of every decision in plain
Python floats); tests/test_gpu_sah_build.py holds the library's builder to it exactly.  Every decision is a handful of
exactly specified f64 operations, so there is no tolerance anywhere.

The definition.  Inputs as for the LBVH model (tests/lbvh_model.py): the visible primitives in
CrSceneDesc.prims order, a list's or CR_PRIM_BVH record's visible objects in its place, and their construction-time
boxes in the real type.  The build orders them 0 .. n-1 and splits ranges [start, end) of that order, root = [0, n):

  (a) the wrapper's box is the union of the range's primitive boxes in `real` (on a tie the earlier value is kept, which
      can decide nothing but the sign of a zero);
  (b) a range of one or two primitives is a leaf; a leaf of one names its primitive twice;
  (c) centroids are 0.5 * (f64(bmin) + f64(bmax)); clo / chi are their bounds over the range, a centroid that is not a
      number bounding nothing; an axis is a candidate only if ext = chi - clo is > 0 and finite;
  (d) primitive p falls into bin_index((cen - clo) * (16 / ext)): t >= 16 gives 15, 0 <= t < 16 gives trunc(t), anything
      else (t not a number: 0 * inf when 16 / ext overflows, or a centroid that is none) gives 0.  The clamp is made in
      floating point, before the conversion to an integer, so every case is defined;
  (e) plane k = 0 .. 14 of an axis puts bins <= k on the left; a plane with an empty side is no candidate;
  (f) cost = area(L) * n_L + area(R) * n_R, area = 2 * ((dx*dy + dy*dz) + dz*dx) over the f64 union of the side's
      primitive boxes, every product and sum rounded on its own: the library's host code is compiled with
      -ffp-contract=off (crucible_amd/csrc/Makefile), so nothing is fused, and numpy fuses nothing either;
  (g) the winner is the first strict minimum in axis-major, plane-minor order; a cost that is not < inf never wins;
  (h) with a winner the range is stably partitioned by bin <= plane, split_axis = the axis; with none
      mid = start + span // 2, split_axis = 0;
  (i) wrappers are numbered in walk order (root, left subtree, right subtree); `children` and `boxes` as cr_export_bvh
      documents them; split_axis is the axis on inner wrappers under CR_BVH_SAH_ORDERED and -1 on leaves, all -1 under
      CR_BVH_SAH.

The formulation: all ranges of one depth are worked on together, so a 70000-primitive build takes about a second and
a tree as deep as it has primitives needs no recursion.  The two sides of every plane are reduced straight from their
member sets -- the range's primitives sorted by bin, side L of plane k is a contiguous run of them and side R the rest,
one np.minimum / np.maximum.reduceat each -- not from running prefix and suffix unions of per-bin boxes as the library does.
Box coordinates are never NaN here: cr_upload_scene takes finite f64 coordinates only, and rounding them to f32 gives
at worst infinities (a NaN needs inf - inf: a sphere with an infinite centre AND radius, which the model leaves undefined).
"""
from collections import namedtuple

import numpy as np

import lbvh_model as L

BINS = 16
SAH, ORDERED = 1, 2          # CrSceneDesc.bvh_mode (include/crucible_hip.h)

# children (n, 2) int32, boxes (n, 6) float64 holding exact values of `real`, split_axis (n,) int32 as exported for the
# mode; then what the tests look at: axis / plane (n,) the decision of every wrapper (-1, -1 on a leaf; axis 0, plane -1
# for the midpoint split), start / end (n,) its range of `order`, order = prims indices in final order, prim_boxes by
# position in the build order, vis = prims index of every position.
Tree = namedtuple("Tree", "children boxes split_axis axis plane start end order prim_boxes vis")


def bin_index(t):
    """(d): the bin of t = (cen - clo) * (16 / ext), clamped in floating point.  t may be an array or a scalar."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (t >= 0.0) & (t < float(BINS))
        k = np.where(inside, t, 0.0).astype(np.int64)        # astype truncates, and only values in [0, 16) reach it
        return np.where(t >= float(BINS), BINS - 1, k)


def area(lo, hi):
    """(f): lo, hi (..., 3) float64."""
    d = hi - lo
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return 2.0 * ((dx * dy + dy * dz) + dz * dx)


def split_level(start, end, order, bmin, bmax, cen):
    """(c)-(h) for the ranges [start[s], end[s]) of `order`, each of three or more primitives.  Returns (mid, axis, plane)
    per range and leaves `order` partitioned."""
    S = len(start)
    span = end - start
    off = np.concatenate([[0], np.cumsum(span)])                     # the ranges side by side: range s is [off[s], off[s+1])
    M = int(off[-1])
    seg = np.repeat(np.arange(S), span)
    local = np.arange(M) - off[seg]
    prim = order[start[seg] + local]
    c = cen[prim]
    clo = np.fmin.reduceat(c, off[:-1], axis=0)
    chi = np.fmax.reduceat(c, off[:-1], axis=0)
    ext = chi - clo
    cost = np.full((S, 3, BINS - 1), np.inf)
    bins = np.zeros((3, M), dtype=np.int64)
    lo_pad, hi_pad = np.full((1, 3), np.inf), np.full((1, 3), -np.inf)
    first = np.repeat(off[:-1], BINS - 1)
    last = np.repeat(off[1:], BINS - 1)
    for a in range(3):
        cand = (ext[:, a] > 0.0) & np.isfinite(ext[:, a])
        if not cand.any():
            continue
        scale = float(BINS) / ext[:, a]
        bins[a] = bin_index((c[:, a] - clo[seg, a]) * scale[seg])
        key = seg * BINS + bins[a]
        by_bin = prim[np.argsort(key, kind="stable")]
        count = np.bincount(key, minlength=S * BINS).reshape(S, BINS)
        n_left = np.cumsum(count, axis=1)[:, :BINS - 1]               # (S, 15): left of plane k
        n_right = span[:, None] - n_left
        # A plane whose own bin is empty cuts where the plane below it cuts: the same two sides, the same cost bit for bit,
        # so never the FIRST minimum; with nothing at or below it, it has an empty side.  Only the others are evaluated.
        # This is a shortcut reasoned from (e)-(g), not part of the definition: what justifies it is the brute force of
        # tests/test_sah_model_host.py, which evaluates all 45 planes of every wrapper and must find the same winner.
        use = np.nonzero((cand[:, None] & (count[:, :BINS - 1] > 0) & (n_right > 0)).ravel())[0]
        if len(use) == 0:
            continue
        n_l, n_r = n_left.ravel()[use], n_right.ravel()[use]
        smin = np.ascontiguousarray(np.concatenate([bmin[by_bin], lo_pad]).T)      # (3, M + 1): each coordinate a row
        smax = np.ascontiguousarray(np.concatenate([bmax[by_bin], hi_pad]).T)
        # side L of (s, k) is the run [first, cut) of the range sorted by bin, side R is [cut, last): reduceat reduces
        # [i0, i1), [i1, i2), ... so of every three results the first two are the sides (the third is one element)
        runs = np.stack([first[use], first[use] + n_l, last[use]], axis=1).ravel()
        lo, hi = np.minimum.reduceat(smin, runs, axis=1).T, np.maximum.reduceat(smax, runs, axis=1).T
        cst = area(lo[0::3], hi[0::3]) * n_l + area(lo[1::3], hi[1::3]) * n_r
        cost_a = np.full(S * (BINS - 1), np.inf)
        cost_a[use] = np.where(cst < np.inf, cst, np.inf)
        cost[:, a, :] = cost_a.reshape(S, BINS - 1)
    flat = cost.reshape(S, 3 * (BINS - 1))
    best = np.argmin(flat, axis=1)                                    # the first of equal minima
    won = flat[np.arange(S), best] < np.inf
    axis = np.where(won, best // (BINS - 1), 0)
    plane = np.where(won, best % (BINS - 1), -1)
    goes_left = np.where(won[seg], bins[axis[seg], np.arange(M)] <= plane[seg], local < (span // 2)[seg])
    n_go = np.add.reduceat(goes_left.astype(np.int64), off[:-1])
    order[start[seg] + local] = prim[np.argsort(seg * 2 + (~goes_left), kind="stable")]
    return start + n_go, axis, plane


def topology(pbox):
    """The node graph over primitive boxes (m, 6) in `real`, m >= 1: per node (in order of creation) start, end, left,
    right (-1 on a leaf), axis, plane, and its box; and the final order."""
    m = len(pbox)
    b = pbox.astype(np.float64)
    bmin, bmax = np.ascontiguousarray(b[:, 0::2]), np.ascontiguousarray(b[:, 1::2])
    rmin, rmax = np.ascontiguousarray(pbox[:, 0::2]), np.ascontiguousarray(pbox[:, 1::2])
    cen = 0.5 * (bmin + bmax)
    order = np.arange(m)
    cols = {k: [] for k in ("start", "end", "left", "right", "axis", "plane", "lo", "hi")}
    start, end, n_nodes = np.array([0]), np.array([m]), 0
    while len(start):
        S = len(start)
        n_nodes += S
        span = end - start
        off = np.concatenate([[0], np.cumsum(span)])
        seg = np.repeat(np.arange(S), span)
        prim = order[start[seg] + np.arange(int(off[-1])) - off[seg]]
        lo = np.minimum.reduceat(rmin[prim], off[:-1], axis=0)        # (a), before this depth partitions anything
        hi = np.maximum.reduceat(rmax[prim], off[:-1], axis=0)
        inner = span > 2
        left, axis, plane = np.full(S, -1), np.full(S, -1), np.full(S, -1)
        if inner.any():
            mid, axis[inner], plane[inner] = split_level(start[inner], end[inner], order, bmin, bmax, cen)
            k = int(inner.sum())
            left[inner] = n_nodes + 2 * np.arange(k)                  # the next depth: left, right, left, right ...
            nxt_start = np.stack([start[inner], mid], axis=1).ravel()
            nxt_end = np.stack([mid, end[inner]], axis=1).ravel()
        else:
            nxt_start = nxt_end = np.zeros(0, dtype=np.int64)
        for key, val in (("start", start), ("end", end), ("left", left), ("right", np.where(left >= 0, left + 1, -1)),
                         ("axis", axis), ("plane", plane), ("lo", lo), ("hi", hi)):
            cols[key].append(val)
        start, end = nxt_start, nxt_end
    return {k: np.concatenate(v) for k, v in cols.items()}, order


def build(flat, real, mode=ORDERED):
    """What cr_export_bvh must return for CR_BVH_SAH (mode 1) / CR_BVH_SAH_ORDERED (mode 2): a Tree."""
    recs = L.prim_records(flat)
    vis = L.visible_prims(recs)
    pbox = L.prim_boxes(recs["kind"][vis], recs["v"][vis], real)
    return build_boxes(pbox, vis, mode)


def build_boxes(pbox, vis, mode=ORDERED):
    """The same from the primitive boxes (m, 6) in their real type and the prims index of each."""
    m = len(vis)
    empty = np.zeros(0, dtype=np.int32)
    if m == 0:
        return Tree(np.zeros((0, 2), np.int32), np.zeros((0, 6)), empty, empty, empty, empty, empty, vis, pbox, vis)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g, order = topology(pbox)
    n = len(g["start"])
    # (i) walk order, with an explicit stack: a tree may be as deep as it has primitives
    number = np.zeros(n, dtype=np.int64)
    left, right = g["left"].tolist(), g["right"].tolist()
    stack, at = [0], 0
    while stack:
        node = stack.pop()
        number[node] = at
        at += 1
        if left[node] >= 0:
            stack.append(right[node])
            stack.append(left[node])
    assert at == n
    by_number = np.argsort(number)
    g = {k: v[by_number] for k, v in g.items()}
    inner = g["left"] >= 0
    children = np.zeros((n, 2), dtype=np.int32)
    children[inner, 0] = number[g["left"][inner]]
    children[inner, 1] = number[g["right"][inner]]
    children[~inner, 0] = ~vis[order[g["start"][~inner]]]
    children[~inner, 1] = ~vis[order[g["end"][~inner] - 1]]
    boxes = np.zeros((n, 6))
    boxes[:, 0::2], boxes[:, 1::2] = g["lo"], g["hi"]
    axis = g["axis"].astype(np.int32)
    split_axis = axis if mode == ORDERED else np.full(n, -1, dtype=np.int32)
    return Tree(children, boxes, split_axis, axis, g["plane"].astype(np.int32), g["start"].astype(np.int32),
                g["end"].astype(np.int32), vis[order], pbox, vis)
