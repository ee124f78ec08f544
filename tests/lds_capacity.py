"""Scenes that fill the LDS to the byte: the arithmetic a launch's residency rests on, restated
on the CPU from the design document, and a scene builder whose table sizes are chosen record by record.  Nothing here loads
the HIP library or touches a device: tests/test_lds_capacity_host.py holds every number to the headers (through
tests/record_sizes_check.cpp, tests/residency_check.cpp and tests/tree_check.cpp), tests/test_gpu_lds_capacity.py renders
the scenes.

A ROW is what decides the bytes of a scene that sits in LDS whole: the precision, the tree order and which record stands
for a wrapper there.  A THRESHOLD is the largest layout a kind of launch stages whole: 160 KB less what the launch puts
behind the scene."""
import ctypes as C
from collections import namedtuple
from functools import lru_cache

import numpy as np

from crucible_amd import _abi as A
from crucible_amd.scene import LERP, LOCAL, FlatScene, Scene, Sphere

LDS = 160 * 1024          # a CU's LDS, and the handle's lds_limit
WINDOW = 128 * 1024       # lds_top_bytes: the window of a tree that does not fit whole
SIDE_LIMIT = 16 * 1024    # lds_side_limit: materials + textures behind a window
MAX_BLOCK = 1024          # MaxBlock<real>::value, the block the comparisons budget for

F64, F32 = A.CR_REAL_F64, A.CR_REAL_F32

# bytes of one record (records.hpp; tests/record_sizes_check.cpp prints the compiler's)
SIZES = {
    F64: dict(entry=64, entry_o=96, screen=32, screen_o=64, prim=96, mat=48, tex=48),
    F32: dict(entry=32, entry_o=64, screen=32, screen_o=64, prim=48, mat=32, tex=32),
}

# name -> (real type, ordered tree, the field of SIZES that a wrapper takes in LDS, the environment of its handle)
Row = namedtuple("Row", "name rt ordered record env")
ROWS = {r.name: r for r in (
    Row("f64", F64, False, "screen", {}),                                   # SCREEN records in LDS (the default)
    Row("f64-wrappers", F64, False, "entry", {"CRUCIBLE_SCREEN_LDS": "0"}),
    Row("f32", F32, False, "entry", {}),
    Row("f64-ordered", F64, True, "screen_o", {}),
    Row("f32-ordered", F32, True, "entry_o", {}),                           # an ordered f32 tree has no screening records
)}
UNORDERED = [n for n, r in ROWS.items() if not r.ordered]


def r16(x):
    return (x + 15) & ~15


def fx_lds_bytes(block, tile_log2):
    """The relaxed sums' slots: two per wave of 3 64-bit words per pixel of a 2^tile_log2-pixel tile (launch_plan.hpp)"""
    return (block // 64) * 2 * (3 << tile_log2) * 8


def aov_lds_bytes(block):
    """The guide slots: per wave 16 pixels x 8 words of 8 bytes"""
    return (block // 64) * 1024


def queue_state_bytes(rt):
    """queue.hpp:33 queue_state_bytes<real>() (the header needs HIP, so the formula is restated): 1024 slots of a ray (7 reals),
    a hit (a real and an int), an rng word, pixel / sample / depth (12 bytes) and an accumulator (3 reals); two rings of 1024
    words; QC_WORDS = 16 control words."""
    real = 8 if rt == F64 else 4
    return 1024 * (7 * real + real + 4 + 8 + 12 + 3 * real) + 2 * 1024 * 4 + 16 * 4


# the largest scene layout each kind of launch stages whole
T_REFERENCE = LDS                                           # reference order: nothing behind the scene
T_RELAXED = LDS - fx_lds_bytes(MAX_BLOCK, 4)                # render_typed: the 16-pixel tile's slots (frames, views, regions, adaptive passes)
T_GUIDE = LDS - aov_lds_bytes(MAX_BLOCK)                    # aov_typed
T_TILE_8X8 = LDS - fx_lds_bytes(MAX_BLOCK, 6)               # plan_tile: the last fx_off that keeps the 8 x 8 tile (1 spp)
T_TILE_8X4 = LDS - 16 * 2 * 96 * 8                          # ... the 8 x 4 tile (2-3 spp): 16 waves, 2 slots, 3 x 32 words of 8 bytes
THRESHOLDS = {"reference": T_REFERENCE, "relaxed": T_RELAXED, "guide": T_GUIDE, "tile8x8": T_TILE_8X8, "tile8x4": T_TILE_8X4}


def queue_threshold(rt):
    """render_queue: lds_bytes + 16 + state <= 160 KB"""
    return LDS - 16 - queue_state_bytes(rt)


@lru_cache(maxsize=None)
def tree_size(n):
    """Wrappers of the reference tree over n primitives (median split, leaves of one or two): odd for every n >= 1"""
    if n <= 2:
        return 1 if n > 0 else 0
    return 1 + tree_size(n // 2) + tree_size(n - n // 2)


Layout = namedtuple("Layout", "prims mats texs bytes end")


def scene_layout(record_bytes, prim_bytes, mat_bytes, tex_bytes, with_prims=True, with_side=True):
    """records | primitives | materials | textures, every table at a multiple of 16 bytes; a table that is
    not staged takes no room; `bytes` ends the last table and end = r16(bytes) is where a launch's own data begins."""
    bytes_ = record_bytes
    prims = mats = texs = r16(record_bytes)
    if with_prims:
        bytes_ = prims + prim_bytes
        mats = texs = prims + r16(prim_bytes)
    if with_side:
        texs = mats + r16(mat_bytes)
        bytes_ = texs + tex_bytes
    return Layout(prims, mats, texs, bytes_, r16(bytes_))


def side_table_bytes(rt, n_mats, n_texs):
    s = SIZES[rt]
    return scene_layout(0, 0, n_mats * s["mat"], n_texs * s["tex"], False, True).end


def layout_of(row, n, wrappers, n_mats, n_texs, with_side=True):
    """LDS bytes of the scene whole, under `row` (a name or a Row)"""
    row = ROWS[row] if isinstance(row, str) else row
    s = SIZES[row.rt]
    return scene_layout(wrappers * s[row.record], n * s["prim"], n_mats * s["mat"], n_texs * s["tex"], True, with_side).end


def predict(layout_bytes, threshold):
    """scene_in_lds: RES_LDS = 1 when the layout fits, else RES_TOP = 2 (every scene here has wrappers and a window)"""
    return 1 if layout_bytes <= threshold else 2


# ---------------------------------------------------------------------------------------------------- the scene
MIN_MATS, MIN_TEXS, MAX_FILL = 3, 3, 64


class CapacityScene(Scene):
    """Scene whose flatten() returns the hand-built description (tests/scenes.py ArrayScene does the same)"""

    def __init__(self, flat, samples, depth):
        super().__init__(1.6, 32, 24, 180.0, 1)
        cam = self.scene_cam
        assert (cam.image_width, cam.image_height) == (32, 20)
        cam.set_samples(samples)
        cam.set_max_depth(depth)
        cam.look_from((0.0, 2.5, 9.0))
        cam.look_at((0.0, 0.5, 0.0))
        cam.set_vfov(40.0)
        self._flat = flat

    def flatten(self):
        self._flat.desc.bvh_mode = self.bvh_mode
        return self._flat


def _vec(*x):
    return (C.c_double * len(x))(*x)


def capacity_textures(n_textures):
    """n_textures >= 3 records, every one live: the last is the ground's checker, its even / odd children the two before
    it, and so on down a binary tree stored root last (node j of the tree at index n - 1 - j, its children the nodes
    2 j + 1 and 2 j + 2): children have smaller indices, the depth is log2(n), a node without children is a solid colour."""
    assert n_textures >= MIN_TEXS
    recs = [None] * n_textures
    for j in range(n_textures):
        a, b = 2 * j + 1, 2 * j + 2
        if a >= n_textures:
            rec = A.CrTexture(A.CR_TEX_SOLID, -1, -1, -1, _vec(((3 * j) % 8 + 1) / 16.0, ((5 * j) % 8 + 4) / 16.0, ((7 * j) % 8 + 8) / 16.0), 0.0)
        else:
            b = b if b < n_textures else a
            rec = A.CrTexture(A.CR_TEX_CHECKER, n_textures - 1 - a, n_textures - 1 - b, -1, _vec(0, 0, 0), 1.0 / (0.25 * (1 + j % 4)))
        recs[n_textures - 1 - j] = rec
    return recs


def capacity_materials(n_materials, ground_texture):
    """n_materials >= 3: 0 the marker's metal, then dielectrics and metals in turn, last the ground's Lambertian"""
    assert n_materials >= MIN_MATS
    mats = [A.CrMaterial(A.CR_MAT_METAL, -1, _vec(0.9, 0.6, 0.2), 0.125)]
    for k in range(1, n_materials - 1):
        if k % 2:
            mats.append(A.CrMaterial(A.CR_MAT_DIELECTRIC, -1, _vec(1, 1, 1), 1.5 if k % 4 == 1 else 1.25))
        else:
            mats.append(A.CrMaterial(A.CR_MAT_METAL, -1, _vec((k % 7 + 2) / 16.0, (k % 5 + 8) / 16.0, (k % 3 + 12) / 16.0), (k % 4) / 16.0))
    mats.append(A.CrMaterial(A.CR_MAT_LAMBERTIAN, ground_texture, _vec(0, 0, 0), 1.0))
    return mats


def capacity_spheres(n):
    """(n, 4) centres and radii, n >= 3.  Row 0 the ground: its box has the least minimum on every axis, so every sort of the
    median split keeps it first and it is the primitive at leaf position 0.  Row n - 1 the marker: the greatest minimum on
    every axis, so it is the primitive at the last leaf position; it is half a unit in radius, several pixels wide.  Between
    them a grid of small spheres above the ground.  Every coordinate is a small dyadic number: the boxes, and so the tree,
    are the same in f32 and f64."""
    assert n >= 3
    g = n - 2
    cols = int(np.ceil(np.sqrt(1.6 * g)))
    rows = -(-g // cols)
    s = 0.25
    while cols * s > 5.0 or rows * s > 4.5:
        s /= 2
    k = np.arange(g)
    i, j = k % cols, k // cols
    v = np.zeros((n, 4))
    v[0] = (0.0, -100.0, 0.0, 100.0)
    v[1:n - 1, 0] = -3.25 + i * s
    v[1:n - 1, 1] = 0.25 + ((7 * i + 3 * j) % 5) * s / 4
    v[1:n - 1, 2] = -3.0 + j * s
    v[1:n - 1, 3] = 0.375 * s
    v[n - 1] = (3.0, 1.0, 2.5, 0.5)
    assert v[1:n - 1, 0].max() < 2.0 and v[1:n - 1, 2].max() < 1.75 and (v[1:n - 1, 1] - v[1:n - 1, 3]).max() < 0.5
    return v


def capacity_scene(n_spheres, n_materials, n_textures, samples=3, depth=6, keyed=False, bvh_mode=A.CR_BVH_REFERENCE):
    """A ground sphere, a grid of small spheres and the marker, all in view of a 32 x 20 camera at depth 6.  Every record of
    the three tables is live: the grid's spheres take the materials 1 .. n_materials - 2 in turn (dielectrics and metals),
    the marker alone has material 0, the ground alone the last material, a Lambertian on the last texture, under which every
    other texture hangs.  keyed: the marker moves inside the exposure (the ANIM kernels)."""
    v = capacity_spheres(n_spheres)
    texs = capacity_textures(n_textures)
    mats = capacity_materials(n_materials, n_textures - 1)
    keys = []
    if keyed:
        moving = Sphere.new(tuple(v[-1, :3]), v[-1, 3], None)
        moving.timeline.translate_point((0.0, 0.25, 0.0), 0.015625, LERP, LOCAL)
        keys = moving.timeline.keyframes()
    prims = []
    fill = max(1, n_materials - 2)
    for k in range(n_spheres):
        mat = n_materials - 1 if k == 0 else (0 if k == n_spheres - 1 else 1 + (k - 1) % fill)
        last = k == n_spheres - 1
        prims.append(A.CrPrimitive(A.CR_PRIM_SPHERE, mat, 0, 0, len(keys) if last else 0, 0, _vec(*v[k], 0, 0, 0, 0, 0)))
    flat = FlatScene(prims, mats, texs, [], keys, A.CR_SKY_DEFAULT, -1)
    sc = CapacityScene(flat, samples, depth)
    sc.bvh_mode = bvh_mode
    sc.shape = (n_spheres, n_materials, n_textures)
    return sc


# ---------------------------------------------------------------------------------------------------- the search
Found = namedtuple("Found", "n wrappers mats texs bytes")


def fit_fillers(row, n, wrappers, threshold, over, with_side=True, max_fill=MAX_FILL):
    """The material and texture counts (each at least the scene's minimum, at most max_fill more) that bring the layout of n
    primitives and `wrappers` wrappers nearest to the threshold: from below (over=False: the largest layout <= threshold), or
    from above (the smallest > threshold).  None where no counts land on that side."""
    if not with_side:
        b = layout_of(row, n, wrappers, MIN_MATS, MIN_TEXS, False)
        return Found(n, wrappers, MIN_MATS, MIN_TEXS, b) if (b > threshold) == over else None
    best = None
    tex = SIZES[ROWS[row].rt]["tex"]
    for m in range(MIN_MATS, MIN_MATS + max_fill + 1):
        # the texture count that lands nearest: the layout grows by one texture record a step
        t0 = (threshold - layout_of(row, n, wrappers, m, 0)) // tex
        for t in (t0 - 1, t0, t0 + 1, t0 + 2):
            t = min(max(t, MIN_TEXS), MIN_TEXS + max_fill)
            b = layout_of(row, n, wrappers, m, t)
            if (b > threshold) != over:
                continue
            if best is None or (b < best.bytes if over else b > best.bytes):
                best = Found(n, wrappers, m, t, b)
    return best


@lru_cache(maxsize=None)
def find(row, threshold, with_side=True):
    """(at, over) for an unordered row: the largest layout <= threshold and the smallest > threshold among the scenes of n
    spheres, n within 16 of the largest count that fits with the fewest side records, and up to MAX_FILL filler materials and
    textures.  with_side=False: the geometry-only layout (wrappers | primitives) of the wavefront pipeline; the side tables
    stay at their minimum.
    tree_size is constant over long runs of n (1023 wrappers from 768 to 1024 spheres), and with 64-byte wrappers every
    layout of such a run is the same multiple of 48 away from the next: where the search cannot come within 32 bytes of
    the threshold on both sides, it looks 96 counts down with up to 128 fillers of each kind (f64-wrappers at 147456)."""
    assert not ROWS[row].ordered, "an ordered tree's wrapper count comes from the device"
    n_max = 3
    while layout_of(row, n_max + 1, tree_size(n_max + 1), MIN_MATS, MIN_TEXS, with_side) <= threshold:
        n_max += 1
    for reach, max_fill in ((16, MAX_FILL), (96, 2 * MAX_FILL)):
        at = over = None
        for n in range(max(3, n_max - reach), n_max + 2):
            a = fit_fillers(row, n, tree_size(n), threshold, False, with_side, max_fill)
            o = fit_fillers(row, n, tree_size(n), threshold, True, with_side, max_fill)
            if a and (at is None or a.bytes > at.bytes):
                at = a
            if o and (over is None or o.bytes < over.bytes):
                over = o
        if not with_side or (at and over and threshold - at.bytes <= 32 and over.bytes - threshold <= 32):
            break
    return at, over


def scene_of(found, **kw):
    return capacity_scene(found.n, found.mats, found.texs, **kw)
