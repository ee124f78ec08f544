"""Scenes whose wrapper boxes leave the f32 range, for tests/test_far_boxes_host.py and tests/test_gpu_far_boxes.py.

The f64 megakernels decide most box tests on f32 screening records, which are valid only while every finite f64 box plane
is finite in f32 too (screen_plane, crucible_amd/csrc/pathtrace.hpp); otherwise the tree must be walked without the screen.
Every scene here is a small near cluster in front of the camera -- a ground sphere, twelve spheres and four triangles, all
three materials, a checker -- plus primitives far outside the f32 range:

  far       a triangle whose box is x [3e38, 3.3e38], y [-1e38, 3.5e38], z [-1e38, 1e38] (only the upper y plane becomes
            infinite in f32: the f32 box is hit by rays that miss the f64 box), a sphere wholly beyond the range (centre
            (1e39, 0, 0), radius 1e38: [inf, inf] in f32) and a backdrop triangle from x = -1e39 to x = 1e39 behind the
            cluster, which primary rays hit
  edge_in   the cluster and the far triangle with its upper y plane exactly FLT_MAX: every plane is an f32
  edge_out  the same with the smallest double that rounds to infinity in f32: one plane too far
  near      the cluster alone: the scene the hostile edits of hostile_edit are applied to
  keyed     the cluster and three spheres whose timelines carry them beyond 1e39 and back (keyed_scene)

The camera stands at (0, 0, 5) and looks along (6, 7.5, -1) with a focus distance of about that length, so that the
unnormalised primary directions are of that size: along them the far triangle's f64 box is missed (x is entered at
t = 5e37, y left at t = 4.7e37) and its f32 box, whose y slab never ends, is hit."""
import numpy as np

from crucible_amd import _abi as A
from crucible_amd.scene import LERP, LOCAL, NERP, CheckerTexture, Dielectric, Lambertian, Metal, Scene, Sphere, Triangle

FLT_MAX = 3.4028234663852886e38
OVER_FLT_MAX = 3.4028235677973366e38        # the smallest double that rounds to inf in f32: FLT_MAX + half an ulp of it
DBL_MAX = 1.7976931348623157e308
WIDTH, HEIGHT, SAMPLES, DEPTH = 32, 24, 2, 6
EYE = np.array([0.0, 0.0, 5.0])
VIEW = np.array([6.0, 7.5, -1.0])
FAR_TRIANGLE = ((3e38, -1e38, -1e38), (3.3e38, 3.5e38, 1e38), (3.1e38, 0.0, 0.0))
FAR_SPHERE = ((1e39, 0.0, 0.0), 1e38)
# four more triangles inside FAR_TRIANGLE's box, every plane of theirs an f32, each reaching below the cluster in y and z
# as FAR_TRIANGLE does: whatever axis a builder sorts on, the five lie together at one end, so the tree has inner wrappers
# that hold far primitives only and whose box is FAR_TRIANGLE's (four companions: the count at which the reference's
# median splits of the static scenes leave such a wrapper, test_far_boxes_host.py asserts it)
FAR_COMPANIONS = tuple(((3.02e38 + k * 1e36, -0.9e38 + k * 2e36, -0.9e38 + k * 1e36), (3.25e38 - k * 1e36, 2.5e38 - k * 3e36, 0.5e38 + k * 1e36),
                        (3.15e38, 1e38 - k * 1e36, -0.5e38)) for k in range(4))
N_SPHERES, N_TRIANGLES = 12, 4               # of the cluster, after the ground: primitives 1 .. 12 and 13 .. 16
STATIC = ("far", "edge_in", "edge_out")
KEYED_FRAMES = (0, 1, 2)                      # near, far, near
KEYED_FAR_FRAME = 1


def view_basis():
    """(w, right, up): the unit view direction and the image's axes for vup = (0, 1, 0)."""
    w = VIEW / np.linalg.norm(VIEW)
    right = np.cross(w, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    return w, right, np.cross(right, w)


def t3(p):
    return tuple(float(x) for x in p)


def cluster(sc):
    """Primitive 0 the ground, 1 .. 12 spheres, 13 .. 16 triangles: around the focus point EYE + VIEW."""
    w, right, up = view_basis()
    focus = EYE + VIEW
    checker = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.7, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    mats = [Lambertian.new_from_color((0.8, 0.25, 0.2), 1.0), Metal.new((0.8, 0.8, 0.9), 0.05), Dielectric.new(1.5),
            Lambertian.new_from_texture(CheckerTexture.new_from_color(0.3, (0.9, 0.9, 0.2), (0.2, 0.2, 0.6)), 0.9),
            Metal.new((0.9, 0.7, 0.3), 0.2)]
    # the ground: a sphere of radius 100 whose top lies 1.2 units below the focus point in the image
    sc.add_element(Sphere.new(t3(focus - 101.2 * up), 100.0, checker), "ground")
    rs = np.random.RandomState(38)
    for k in range(N_SPHERES):
        c = focus + rs.uniform(-2.6, 2.6) * right + rs.uniform(-1.0, 1.6) * up + rs.uniform(-1.5, 2.5) * w
        sc.add_element(Sphere.new(t3(c), float(rs.uniform(0.25, 0.55)), mats[k % len(mats)]), f"s{k}")
    for k in range(N_TRIANGLES):
        c = focus + rs.uniform(-2.4, 2.4) * right + rs.uniform(-0.8, 1.4) * up + rs.uniform(1.0, 3.0) * w
        pts = [c + rs.uniform(-0.8, 0.8, 3) for _ in range(3)]
        sc.add_element(Triangle.new(t3(pts[0]), t3(pts[1]), t3(pts[2]), mats[(k + 1) % len(mats)]), f"t{k}")


def base_scene(frame_rate=24, shutter=180.0):
    sc = Scene.new_image(WIDTH / HEIGHT, WIDTH, frame_rate, shutter, 1)
    cam = sc.scene_cam
    cam.image_width, cam.image_height = WIDTH, HEIGHT
    cam.set_samples(SAMPLES)
    cam.set_max_depth(DEPTH)
    cam.look_from(t3(EYE))
    cam.look_at(t3(EYE + VIEW))
    cam.set_vfov(36.0)
    cam.set_focus_dist(float(np.linalg.norm(VIEW)))
    cluster(sc)
    return sc


BACKDROP_MATERIAL = Metal.new((0.6, 0.7, 0.9), 0.0)


def add_backdrop(sc):
    """x from -1e39 to 1e39 along a line 9 units behind the focus point and above it in the image, the apex below it."""
    w, _, up = view_basis()
    base, apex = EYE + VIEW + 9.0 * w + 4.0 * up, EYE + VIEW + 7.0 * w - 0.5 * up
    sc.add_element(Triangle.new((-1e39, base[1], base[2]), (1e39, base[1], base[2]), t3(apex), BACKDROP_MATERIAL), "backdrop")


def add_far_triangles(sc, top=None):
    """FAR_TRIANGLE (top: another upper y plane for it) and its companions."""
    a, b, c = FAR_TRIANGLE
    if top is not None:
        b = (b[0], top, b[2])
    mat = Metal.new((0.9, 0.9, 0.9), 0.1)
    sc.add_element(Triangle.new(a, b, c, mat), "far_triangle")
    for k, (a, b, c) in enumerate(FAR_COMPANIONS):
        sc.add_element(Triangle.new(a, b, c, mat), f"far_companion{k}")


def static_scene(name):
    sc = base_scene()
    if name == "far":
        add_far_triangles(sc)
        sc.add_element(Sphere.new(*FAR_SPHERE, Lambertian.new_from_color((0.3, 0.7, 0.3), 1.0)), "far_sphere")
        add_backdrop(sc)
    elif name in ("edge_in", "edge_out"):
        add_far_triangles(sc, FLT_MAX if name == "edge_in" else OVER_FLT_MAX)
    else:
        assert name == "near", name
    return sc


def largest_plane(name):
    return {"edge_in": FLT_MAX, "edge_out": OVER_FLT_MAX}[name]


N_ROVERS = 3
GRID = 2.0 ** 100                              # every far offset of the rovers is a multiple: their sums are exact


def rover_offsets():
    """(jump, travel, leave, back): the rovers' four translations.  The jump takes them to a staging point, the travel through
    FAR_TRIANGLE's box -- from its corner (3e38, -1e38, -1e38) at a quarter of the way to (3.3e38, 3.5e38, 1e38) at seven
    eighths --, `leave` on to x = 2.3e39, and `back` is minus their sum exactly."""
    a, b = np.array(FAR_TRIANGLE[0]), np.array(FAR_TRIANGLE[1])
    travel = np.round((b - a) / 0.625 / GRID) * GRID
    jump = np.round((a - 0.25 * travel) / GRID) * GRID
    leave = np.round(np.array([2e39, 0.0, 0.0]) / GRID) * GRID
    return jump, travel, leave, -((jump + travel) + leave)


def keyed_scene(frame=0, refit=True):
    """1 fps with a 180 degree shutter: frame f draws ray times in [f, f + 1/2].  Three spheres, the rovers, stand together at
    the far upper corner of the cluster (last on every axis, so that the reference's tree keeps them in a subtree of their
    own).  At t = 0.8 they jump to a staging point (NERP), travel from there until t = 1.6 (LERP) -- during frame 1 through
    FAR_TRIANGLE's box, which their refitted boxes then are: finite in x and z, beyond FLT_MAX in y --, go on to x = 2.3e39
    until t = 1.9 (LERP) and jump back at t = 1.95 (NERP) by exactly what they travelled.  Next to 3e38 the cluster's own
    coordinates are less than half a unit in the last place, so the way back ends at the origin, beside the camera, not in
    the cluster.  With refit_boxes = 1 frames 0 and 2 have no plane beyond the f32 range and frame 1 has; in f32 the travel
    is infinite in y, and from frame 1 on the rovers are nowhere.  A fourth keyed sphere moves inside the cluster from
    t = 0.6 on: during frame 0 every primitive rests where it was built, so the construction-time boxes are that frame's
    boxes and a render without refit can be held to the linear list."""
    sc = base_scene(frame_rate=1, shutter=180.0)
    w, right, up = view_basis()
    corner = EYE + VIEW + 3.2 * w + 2.2 * right + 1.2 * up
    jump, travel, leave, back = rover_offsets()
    for k in range(N_ROVERS):
        alias = f"rover{k}"
        sc.add_element(Sphere.new(t3(corner + 0.5 * k * (w + right)), 0.3, Lambertian.new_from_color((0.9, 0.5, 0.1 + 0.2 * k), 1.0)), alias)
        sc.translate_point(t3(jump), 0.8, NERP, LOCAL, alias)
        sc.translate_point(t3(travel), 1.6, LERP, LOCAL, alias)
        sc.translate_point(t3(leave), 1.9, LERP, LOCAL, alias)
        sc.translate_point(t3(back), 1.95, NERP, LOCAL, alias)
    sc.translate_point((0.0, 0.0, 0.0), 0.6, NERP, LOCAL, "s3")           # nothing moves during frame 0
    sc.translate_point(t3(0.8 * right + 0.3 * up), 2.5, LERP, LOCAL, "s3")
    sc.scene_cam.frame = frame
    sc.scene_cam.refit_boxes = refit
    return sc


def scene(name, frame=0):
    return keyed_scene(frame) if name == "keyed" else static_scene(name)


# ---------------------------------------------------------------- hostile edits of the "near" scene
def hostile_edit(flat):
    """(indices, rows, inverse rows) for cr_update_primitives on the flattened "near" scene.  Every value the call reads is
    finite, so validate_update accepts the rows: a sphere of radius 0, one of radius 1e-46 (zero in f32, 1 / r infinite)
    and one of a subnormal f64 radius, centres at +-1e39, +-1e300 and at DBL_MAX with a radius that makes centre + radius
    overflow to an infinite plane, a centre of -0.0, a triangle of three equal vertices, one of collinear vertices and
    FAR_TRIANGLE written over a near triangle; the unread tail of every sphere row is NaN.  The inverse rows are the
    primitives' values as uploaded."""
    idx, rows = [], []
    v0 = np.array([list(flat.prims[i].v) for i in range(flat.desc.n_prims)], dtype=np.float64)

    def sphere(i, centre=None, radius=None):
        assert flat.prims[i].kind == A.CR_PRIM_SPHERE
        row = v0[i].copy()
        if centre is not None:
            row[:3] = centre
        if radius is not None:
            row[3] = radius
        row[4:] = np.nan
        idx.append(i)
        rows.append(row)

    def triangle(i, pts):
        assert flat.prims[i].kind == A.CR_PRIM_TRIANGLE
        idx.append(i)
        rows.append(np.array(pts, dtype=np.float64).reshape(9))

    sphere(1, radius=0.0)
    sphere(2, radius=1e-46)
    sphere(3, radius=1e-310)
    sphere(4, centre=(1e39, v0[4, 1], v0[4, 2]))
    sphere(5, centre=(v0[5, 0], -1e39, v0[5, 2]))
    sphere(6, centre=(v0[6, 0], v0[6, 1], 1e300))
    sphere(7, centre=(-1e300, -1e300, -1e300))
    sphere(8, centre=(DBL_MAX, 0.0, 0.0), radius=1e300)
    sphere(9, centre=(-0.0, -0.0, -0.0), radius=0.5)
    first = 1 + N_SPHERES
    triangle(first, [v0[first, 0:3]] * 3)
    triangle(first + 1, [v0[first + 1, 0:3], v0[first + 1, 0:3] + (0.5, 0.25, -0.125), v0[first + 1, 0:3] + (1.0, 0.5, -0.25)])
    triangle(first + 2, FAR_TRIANGLE)
    idx = np.array(idx, dtype=np.int32)
    rows = np.array(rows, dtype=np.float64)
    back = v0[idx].copy()
    back[flat_kinds(flat)[idx] == A.CR_PRIM_SPHERE, 4:] = np.nan
    return idx, rows, back


def flat_kinds(flat):
    return np.array([flat.prims[i].kind for i in range(flat.desc.n_prims)], dtype=np.int32)


# ---------------------------------------------------------------- what the host test measures
def primary_rays(o, cam, seed):
    """(W * H * samples, 8) rows of oracle_camera_ray: origin, unnormalised direction, time, draws."""
    import ctypes as C
    cd = cam.desc()
    p = cam.params(seed, o.real_type, 0, None, 0, A.CR_SUM_DEFAULT)
    out = np.zeros((cam.image_height, cam.image_width, cam.samples, 8), dtype=o.np_real)
    for j in range(cam.image_height):
        for i in range(cam.image_width):
            for s in range(cam.samples):
                o.lib.oracle_camera_ray(C.byref(cd), C.byref(p), i, j, s, out[j, i, s].ctypes.data_as(C.c_void_p))
    return out.reshape(-1, 8)


def screen_disagreements(boxes, children, rays):
    """Per wrapper: the number of rays for which Aabb::hit (walk_corpus.aabb_hit_ref, the whole interval [0.001, inf)) on the
    box rounded to f32 differs from Aabb::hit on the f64 box, both computed in f64.  Returns (counts (n,), is_leaf (n,))."""
    import walk_corpus as wc
    boxes = np.asarray(boxes, dtype=np.float64)
    with np.errstate(over="ignore"):
        rounded = boxes.astype(np.float32).astype(np.float64)
    counts = np.zeros(len(boxes), dtype=np.int64)
    tmax = np.full((len(rays), 1), np.inf)
    od = np.asarray(rays[:, 0:6], dtype=np.float64)
    for k in range(len(boxes)):
        a = wc.aabb_hit_ref(np.concatenate([np.tile(boxes[k], (len(rays), 1)), od, tmax], axis=1))
        b = wc.aabb_hit_ref(np.concatenate([np.tile(rounded[k], (len(rays), 1)), od, tmax], axis=1))
        counts[k] = int((a != b).sum())
    return counts, (np.asarray(children) < 0).all(axis=1)
