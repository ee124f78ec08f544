"""The expected frame tree of CR_REFIT_REBUILD, from the oracle and tests/sah_model.py alone -- none of
the library's code.

The per-primitive motion boxes come from the oracle's refit: it is handed (oracle_set_tree) a comb tree in which every
visible primitive sits alone in a one-primitive wrapper, a wrapper naming it twice, renders one pixel at one sample with
refit_boxes = 1 at the frame, and the wrapper boxes are read back (oracle_bvh_dump).  A one-primitive wrapper's refitted
box is the box of that primitive over the frame's ray times (refit_rec).  sah_model.build_boxes over those boxes is the
tree cr_export_render_bvh must return: a leaf's box is the union of its primitives' motion boxes and an inner wrapper's
the union of its children's, which is what a refit derives for that topology."""
import copy

import numpy as np

import lbvh_model as L
import sah_model as M


def comb_tree(vis):
    """children (2m - 1, 2) of the comb over the primitives `vis` (prims indices), and the wrapper of each: wrapper 2i is
    inner with the leaf 2i + 1 of primitive i on the left and the rest of the comb on the right; the last primitive's
    leaf closes it."""
    m = len(vis)
    kids = np.zeros((2 * m - 1, 2), dtype=np.int32)
    leaf = np.zeros(m, dtype=np.int64)
    for i in range(m - 1):
        kids[2 * i] = (2 * i + 1, 2 * i + 2)
        kids[2 * i + 1] = (~int(vis[i]), ~int(vis[i]))
        leaf[i] = 2 * i + 1
    kids[2 * (m - 1)] = (~int(vis[-1]), ~int(vis[-1]))
    leaf[m - 1] = 2 * (m - 1)
    return kids, leaf


def oracle_motion_boxes(o, flat, cam, vis=None):
    """(m, 6) boxes in the oracle's real type (xmin, xmax, ymin, ymax, zmin, zmax), one per visible primitive in prims
    order, over the ray times of cam's frame; and vis."""
    if vis is None:
        vis = L.visible_prims(L.prim_records(flat))
    kids, leaf = comb_tree(vis)
    one = copy.copy(cam)
    one.image_width = one.image_height = 1
    one.samples, one.max_depth = 1, 1
    one.refit_boxes = True
    h = o.scene_create(flat)
    try:
        o.set_tree(h, np.zeros((len(kids), 6)), kids)
        o.render(h, one, seed=1, n_threads=1)
        boxes = np.zeros((len(kids), 6), dtype=o.np_real)
        dumped = np.zeros((len(kids), 2), dtype=np.int32)
        n = o.lib.oracle_bvh_dump(h, boxes.ctypes.data, dumped.ctypes.data, len(kids))
    finally:
        o.scene_destroy(h)
    assert n == len(kids)
    assert (dumped[leaf, 0] == vis).all() and (dumped[leaf, 1] == vis).all()     # the dump's walk order is the comb's
    return boxes[leaf], vis


def frame_tree(o, flat, cam, mode):
    """The sah_model.Tree the library must walk for cam's frame under refit_boxes = "rebuild"."""
    pbox, vis = oracle_motion_boxes(o, flat, cam)
    return M.build_boxes(pbox, vis, mode & 0xFF)
