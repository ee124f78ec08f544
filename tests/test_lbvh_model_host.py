"""tests/lbvh_model.py, the plain model the device-built LBVH tree is held to (tests/test_gpu_lbvh_build.py), pinned on
the CPU before any GPU sees it:
  * its top-down radix tree against lbvh_children of crucible_amd/csrc/lbvh.hpp compiled for the host (Karras'
    bottom-up binary searches -- the two share nothing but the definition of the tree);
  * its Morton key against lbvh_key, at random triples and at every edge of the clamp and of the cells;
  * its primitive boxes against the oracle's reference-mode tree of one-primitive scenes, f32 and f64.
Every comparison is exact."""
import subprocess

import numpy as np
import pytest

import lbvh_model as M
import scenes
from crucible_amd import _abi as A
from test_lbvh_host import compile_lbvh_check


@pytest.fixture(scope="module")
def lbvh_check(tmp_path_factory):
    return compile_lbvh_check(tmp_path_factory.mktemp("lbvh_check"))


# ------------------------------------------------------------------ topology
def key_sets():
    """(name, sorted uint64 keys): the four families tests/lbvh_check.cpp draws, and the edges of the tie-break."""
    rng = np.random.RandomState(7)
    r63 = lambda n: (rng.randint(0, 2 ** 31, n).astype(np.uint64) << np.uint64(32) | rng.randint(0, 2 ** 32, n, dtype=np.int64).astype(np.uint64))

    def family(mode, n):
        if mode == 0:
            return r63(n)                                                          # unique keys
        if mode == 1:
            return rng.randint(0, 7, n).astype(np.uint64)                          # heavy duplicates
        if mode == 2:
            return np.full(n, 42, dtype=np.uint64)                                 # all keys equal
        return rng.randint(0, 3, n).astype(np.uint64) << np.uint64(60) | rng.randint(0, 4, n).astype(np.uint64)   # clustered
    sets = []
    for trial in range(400):
        n = 2 + int(rng.randint(0, 40 if trial < 300 else 5000))
        sets.append((f"family{trial % 4}-n{n}", family(trial % 4, n)))
    for mode in range(4):
        for n in (2, 3):
            for rep in range(4):
                sets.append((f"family{mode}-n{n}", family(mode, n)))
    for run in (255, 256, 257, 70000):
        sets.append((f"run{run}", np.full(run, 0x123456789ABCDEF, dtype=np.uint64)))
        sets.append((f"run{run}-zero", np.zeros(run, dtype=np.uint64)))
        sets.append((f"run{run}-between", np.concatenate([r63(5), np.full(run, 1 << 62, dtype=np.uint64), r63(7)])))
        sets.append((f"two-runs-{run}", np.concatenate([np.full(run, 9, dtype=np.uint64), np.full(run + 1, 10, dtype=np.uint64)])))
    for base in (0, 0x2AAAAAAAAAAAAAAA, (1 << 63) - 2):
        for bit in (0, 62):
            for n in (2, 3, 4, 17, 256, 1000):
                pick = rng.randint(0, 2, n).astype(np.uint64)
                pick[0], pick[-1] = 0, 1      # both values present
                sets.append((f"only-bit{bit}-n{n}", np.uint64(base) ^ (pick << np.uint64(bit))))
    sets.append(("bit0-and-bit62", np.array([0, 1, 1 << 62, (1 << 62) | 1] * 3, dtype=np.uint64)))
    return [(name, np.sort(k)) for name, k in sets]


def karras_splits(ch, n):
    """lbvh_children's output (node i: left, right; a child < 0 is ~position) as the (a, b, split) ranges of its
    internal nodes in walk order -- the form of lbvh_model.radix_splits."""
    ch = ch.tolist()
    out = []

    def walk(c):
        if c < 0:
            return ~c, ~c
        assert len(out) < n - 1, "more internal nodes reached than exist: not a tree"
        at = len(out)
        out.append(None)
        la, lb = walk(ch[c][0])
        ra, rb = walk(ch[c][1])
        assert lb + 1 == ra, "the left child is the lower range"
        out[at] = (la, rb, lb)
        return la, rb
    assert walk(0) == (0, n - 1)
    return out


def test_radix_tree_equals_lbvh_children(lbvh_check, tmp_path):
    sets = key_sets()
    assert len(sets) >= 400
    path = tmp_path / "keys.bin"
    with open(path, "wb") as f:
        for _, k in sets:
            f.write(np.uint64(len(k)).tobytes())
            f.write(k.astype("<u8").tobytes())
    out = subprocess.run([lbvh_check, "children", str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr
    ch = np.frombuffer(out.stdout, dtype="<i4").reshape(-1, 2)
    assert len(ch) == sum(len(k) - 1 for _, k in sets)
    at = 0
    for name, k in sets:
        n = len(k)
        assert karras_splits(ch[at:at + n - 1], n) == M.radix_splits(k), name
        at += n - 1


# ------------------------------------------------------------------ keys
def key_rows():
    """Rows (centroid, lo, inv_ext) of f64 triples."""
    rng = np.random.RandomState(11)
    rows = []
    n = 4000
    lo = rng.uniform(-5, 5, (n, 3))
    ext = rng.uniform(0.1, 10, (n, 3))
    c = lo + ext * rng.uniform(-0.05, 1.05, (n, 3))         # some beyond either end
    rows.append(np.concatenate([c, lo, 1.0 / ext], axis=1))
    c = rng.uniform(0, 1, (n, 3))                            # the unit cube itself
    rows.append(np.concatenate([c, np.zeros((n, 3)), np.ones((n, 3))], axis=1))
    tiny, big, inf, nan = 5e-324, 1.7976931348623157e308, np.inf, np.nan
    below = lambda x: np.nextafter(x, -inf)
    above = lambda x: np.nextafter(x, inf)
    edge = [0.0, -0.0, 1.0, below(0.0), above(0.0), below(1.0), above(1.0), nan, inf, -inf, tiny, -tiny, 2.2250738585072014e-308,
            1e-310, big, -big, 0.5, below(0.5), above(0.5)]
    e = []
    for x in edge:                       # the value on each axis in turn, the others mid-range
        for a in range(3):
            cc = [0.25, 0.5, 0.75]
            cc[a] = x
            e.append(cc + [0.0] * 3 + [1.0] * 3)
    for x in edge:                       # ... as lo, as inv_ext
        e.append([0.3, 0.6, 0.9] + [x, 0.0, 0.0] + [1.0] * 3)
        e.append([0.3, 0.6, 0.9] + [0.0] * 3 + [1.0, x, 1.0])
        e.append([x, x, x] + [x, x, x] + [1.0, inf, 0.0])     # c - lo = 0 or NaN, times 1, inf, 0
    # u exactly 0 and 1 and an ulp outside through a scaled axis: lo = 2, extent 4
    for x in (2.0, 6.0, below(2.0), above(6.0), below(6.0), above(2.0)):
        e.append([x, 4.0, 4.0, 2.0, 2.0, 2.0, 0.25, 0.25, 0.25])
    e.append([1.0, 2.0, 3.0] + [0.0] * 3 + [0.0] * 3)         # inv_ext 0: an axis without extent
    e.append([big, -big, big] + [-big, -big, -big] + [0.0] * 3)
    e.append([big, -big, big] + [-big, big, 0.0] + [1e-308] * 3)   # c - lo overflows
    rows.append(np.array(e))
    # cell boundaries k / (2^21 - 1), k = 1 .. 2^21 - 1, an ulp either side: the first, the last, and a sample
    ks = np.unique(np.concatenate([[1, 2, 2097150, 2097151], rng.randint(1, 2097152, 400)])).astype(np.float64)
    for a in range(3):
        for x in (ks / M.CELLS, below(ks / M.CELLS), above(ks / M.CELLS)):
            cc = np.tile([0.25, 0.5, 0.75], (len(ks), 1))
            cc[:, a] = x
            rows.append(np.concatenate([cc, np.zeros((len(ks), 3)), np.ones((len(ks), 3))], axis=1))
    return np.concatenate(rows, axis=0)


def test_morton_key_equals_lbvh_key(lbvh_check, tmp_path):
    rows = key_rows()
    assert len(rows) > 8000
    path = tmp_path / "rows.bin"
    rows.astype("<f8").tofile(path)
    out = subprocess.run([lbvh_check, "keys", str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr
    theirs = np.frombuffer(out.stdout, dtype="<u8")
    assert len(theirs) == len(rows)
    mine = np.array([M.morton_key(r[0:3], r[3:6], r[6:9]) for r in rows], dtype=np.uint64)
    bad = np.nonzero(mine != theirs)[0]
    assert len(bad) == 0, [(rows[i].tolist(), hex(mine[i]), hex(theirs[i])) for i in bad[:5]]
    # the model's array form (what build() uses) is the same function; rows sharing lo and inv_ext go through it together
    for block in (rows[4000:8000], rows[-1200:]):
        keys, _ = M.morton_keys(block[:, 0:3], block[0, 3:6], block[0, 6:9])
        assert (block[:, 3:9] == block[0, 3:9]).all()
        assert np.array_equal(keys, np.array([M.morton_key(r[0:3], r[3:6], r[6:9]) for r in block], dtype=np.uint64))


def test_interleave_places_x_highest():
    assert M.interleave(0x1FFFFF, 0, 0) == 0x4924924924924924
    assert M.interleave(0, 0x1FFFFF, 0) == 0x2492492492492492
    assert M.interleave(0, 0, 0x1FFFFF) == 0x1249249249249249
    assert M.interleave(1, 0, 0) == 4 and M.interleave(0, 1, 0) == 2 and M.interleave(0, 0, 1) == 1
    assert M.interleave(1 << 20, 0, 0) == 1 << 62


# ------------------------------------------------------------------ boxes
def box_corpus():
    """(kind, v[9]) of single primitives."""
    rng = np.random.RandomState(5)
    third, tenth = 1.0 / 3.0, 0.1
    out = []
    sph = [(0.0, 0.0, 0.0, 1.0), (1.0, 2.0, 3.0, -0.5), (tenth, third, -tenth, -third), (1.0, 2.0, 3.0, 0.0), (-0.0, 0.0, -0.0, 0.0),
           (-0.0, -0.0, -0.0, -0.0), (tenth, third, 0.7, 0.3), (1e8, -1e8, 16777217.0, 0.3), (16777217.0, 33554433.0, -16777219.0, 1.0),
           (1e-50, -1e-50, 1e-320, 1e-46), (1.0, 1.0, 1.0, 1e-9), (3e38, -3e38, 1e38, 1e38), (0.1, 0.2, 0.3, 1e30),
           (1.0000000596046448, 1.0000001192092896, 0.9999999701976776, 2.9802322387695312e-08)]
    for s in sph:
        out.append((M.SPHERE, list(s) + [0.0] * 5))
    for _ in range(150):
        c, r = rng.uniform(-100, 100, 3) * 10.0 ** rng.randint(-6, 6), rng.uniform(-1, 3) * 10.0 ** rng.randint(-6, 6)
        out.append((M.SPHERE, list(c) + [r] + [0.0] * 5))
    tri = [(0, 0, 0, 1, 0, 0, 0, 1, 0), (0, 2, 0, 1, 2, 0, 0.5, 2, 1), (3, 0, 0, 3, 1, 0, 3, 0.5, 1), (0, 0, -1, 1, 0, -1, 0, 1, -1),
           (1, 1, 1, 1, 1, 1, 1, 1, 1), (-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0), (0.0, 0.0, 0.0, -0.0, -0.0, -0.0, 1.0, -1.0, 0.0),
           (tenth, third, 0.7, third, 0.7, tenth, 0.7, tenth, third), (16777217.0, 16777216.0, 16777218.0, 16777219.0, 1e-50, -1e-50, 0, 1e-320, 5),
           (1.0000000596046448, 1.0, 1.0000001192092896, 1.0, 1.0000000596046448, 1.0, 0.9999999701976776, 1.0, 1.0),
           (-3e38, 3e38, 0, 3e38, -3e38, 1, 0, 0, 2)]
    for t in tri:
        out.append((M.TRIANGLE, [float(x) for x in t]))
    for _ in range(150):
        out.append((M.TRIANGLE, list(rng.uniform(-100, 100, 9) * 10.0 ** rng.randint(-6, 6))))
    return out


@pytest.mark.parametrize("rt,real", [(A.CR_REAL_F64, np.float64), (A.CR_REAL_F32, np.float32)], ids=["f64", "f32"])
def test_prim_boxes_equal_the_oracle(oracles, rt, real):
    """A one-primitive wrapper's box is the primitive's box: the oracle's reference-mode tree of a one-primitive scene
    against the model's box, and against the model's whole build of that scene."""
    o = oracles[rt]
    corpus = box_corpus()
    different_in_f32 = 0
    for kind, v in corpus:
        flat = scenes.ArrayScene([kind], np.array([v])).flatten()
        h = o.scene_create(flat)
        try:
            oboxes = np.zeros((4, 6), dtype=o.np_real)
            okids = np.zeros((4, 2), dtype=np.int32)
            n = o.lib.oracle_bvh_dump(h, oboxes.ctypes.data, okids.ctypes.data, 4)
        finally:
            o.scene_destroy(h)
        assert n == 1 and okids[0].tolist() == [0, 0]
        box = M.prim_boxes(np.array([kind]), np.array([v]), real)
        assert box.dtype == real and np.array_equal(box[0], oboxes[0]), (kind, v, box[0], oboxes[0])
        tree = M.build(flat, real)
        assert np.array_equal(tree.boxes, oboxes[:1].astype(np.float64)) and tree.children.tolist() == [[~0, ~0]]
        different_in_f32 += not np.array_equal(M.prim_boxes(np.array([kind]), np.array([v]), np.float32).astype(np.float64),
                                               M.prim_boxes(np.array([kind]), np.array([v]), np.float64))
    assert different_in_f32 > 100      # the corpus does tell the two real types apart


# ------------------------------------------------------------------ the model's own bookkeeping
def test_model_splices_lists_and_skips_hidden():
    """(a) and (f) on a hand-made record array: hidden primitives and hidden members are left out, a list's and a
    CR_PRIM_BVH record's visible members stand where the record stands, leaves name CrSceneDesc.prims indices."""
    S, T, L, B, H, Mb = M.SPHERE, M.TRIANGLE, M.LIST, M.BVH, M.HIDDEN, M.MEMBER
    kind = [S, L, S, S, T, S, B, S, S, S]
    flags = [0, 0, Mb, Mb | H, Mb, H, 0, Mb | H, Mb, 0]
    v = np.zeros((10, 9))
    v[:, 0] = np.arange(10)         # x = index: sorted order is index order
    v[:, 3] = 0.25
    v[4] = [4, 0, 0, 4.5, 1, 0, 3.5, 0, 1]
    v[1, :2] = [2, 3]
    v[6, :2] = [7, 2]
    flat = scenes.ArrayScene(kind, v, flags).flatten()
    assert M.visible_prims(M.prim_records(flat)).tolist() == [0, 2, 4, 8, 9]
    for real in (np.float32, np.float64):
        t = M.build(flat, real)
        assert t.order.tolist() == [0, 2, 4, 8, 9]
        leaves = t.children[t.children[:, 0] < 0]
        assert (leaves[:, 0] == leaves[:, 1]).all() and (~leaves[:, 0]).tolist() == [0, 2, 4, 8, 9]
        assert len(t.children) == 9 and t.children[0, 0] == 1
        assert np.array_equal(t.boxes[0], [-0.25, 9.25, -0.25, 1.0, -0.25, 1.0])
    empty = M.build(scenes.ArrayScene([S], np.zeros((1, 9)), [H]).flatten(), np.float64)
    assert len(empty.children) == 0 and len(empty.boxes) == 0
