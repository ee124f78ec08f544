"""Small scenes used by the parity tests and by tests/golden/make_golden.py."""
import numpy as np

from crucible_amd.scene import (LERP, LOCAL, NERP, WORLD, BVHWrapper, CheckerTexture, Dielectric, HitList, ImageTexture, Lambertian,
                                Metal, RTWImage, Scene, SolidColor, Sphere, Triangle)


def small_image(w=16, h=8, seed=3):
    rs = np.random.RandomState(seed)
    return RTWImage(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8))


def mixed_scene(width=64, samples=4, sky=True, animate=False, depth=12):
    """Triangles + spheres, all three materials, solid / checker / nested checker / image textures,
    spherical sky, defocus blur; optional keyframes on camera, spheres and a triangle pair."""
    sc = Scene.new_image(16.0 / 9.0, width, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((6.0, 2.5, 5.0))
    cam.look_at((0.0, 0.6, 0.0))
    cam.set_vfov(35.0)
    cam.set_defocus_angle(0.8)
    cam.set_focus_dist(7.5)
    img = small_image()
    nested = CheckerTexture.new_from_textures(1.5, CheckerTexture.new_from_color(0.25, (0.9, 0.1, 0.1), (0.1, 0.1, 0.9)),
                                              ImageTexture(img))
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, Lambertian.new_from_texture(nested, 1.0)), "ground")
    sc.add_element(Sphere.new((0.0, 1.0, 0.0), 1.0, Dielectric.new(1.5)), "glass")
    sc.add_element(Sphere.new((0.0, 1.0, 0.0), 0.6, Dielectric.new(1.0 / 1.5)), "bubble")
    sc.add_element(Sphere.new((-2.2, 0.8, 0.5), 0.8, Lambertian.new_from_texture(ImageTexture(img), 0.85)), "globe")
    sc.add_element(Sphere.new((2.2, 0.7, -0.3), 0.7, Metal.new((0.8, 0.6, 0.2), 0.3)), "brass")
    sc.add_element(Sphere.new((1.0, 0.3, 2.0), 0.3, Metal.new((0.9, 0.9, 0.9), 0.0)), "mirror")
    sc.add_element(Sphere.new((-1.0, 0.25, 2.2), 0.25, Lambertian.new_from_color((0.2, 0.7, 0.3), 0.6)), "matte")
    # a quad (two triangles, one alias each) and a tetrahedron behind the spheres
    m_quad = Metal.new((0.7, 0.7, 0.9), 0.1)
    sc.add_element(Triangle.new((-3.0, 0.0, -2.5), (3.0, 0.0, -2.5), (3.0, 3.0, -2.5), m_quad), "quad_a")
    sc.add_element(Triangle.new((-3.0, 0.0, -2.5), (3.0, 3.0, -2.5), (-3.0, 3.0, -2.5), m_quad), "quad_b")
    m_tet = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.4, (0.9, 0.9, 0.2), (0.2, 0.2, 0.2)), 1.0)
    p = [(3.2, 0.0, 1.5), (4.2, 0.0, 1.2), (3.7, 0.0, 2.3), (3.7, 1.0, 1.7)]
    for k, (a, b, c) in enumerate([(0, 1, 3), (1, 2, 3), (2, 0, 3), (0, 2, 1)]):
        sc.add_element(Triangle.new(p[a], p[b], p[c], m_tet), f"tet{k}")
    # an axis-aligned flat triangle alone in its BVH leaf never hits (zero-thickness box, bvh.rs:126): keep one
    sc.add_element(Triangle.new((-4.0, 0.01, 3.0), (-3.0, 0.01, 3.0), (-3.5, 0.01, 4.0), Metal.new((1.0, 0.2, 0.2), 0.0)), "flat")
    if sky:
        rs = np.random.RandomState(11)
        sc.load_spherical_skybox(RTWImage(rs.randint(60, 256, size=(16, 32, 3)).astype(np.uint8)))
    if animate:
        sc.cam_translate_point((7.0, 3.0, 4.0), 0.02, LERP, WORLD, "from")
        sc.cam_translate_point((0.2, 0.5, 0.0), 0.015, LERP, WORLD, "at")
        sc.translate_point((0.3, 0.2, 0.0), 0.01, LERP, LOCAL, "brass")
        sc.translate_point((0.0, 0.1, 0.1), 0.012, NERP, LOCAL, "mirror")
        sc.scale_r(0.4, 0.02, LERP, "matte")
        sc.scale_r(0.9, 0.005, NERP, "globe")
        sc.translate_point((0.0, 0.3, 0.0), 0.018, LERP, LOCAL, "tet0")
    return sc


def few_spheres(n, width=48, samples=3):
    """n = 0, 1, 2, 3 ... primitives: the BVH edge cases (empty list, span-1 root, span-2 root, first sort)."""
    sc = Scene.new_image(16.0 / 9.0, width, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(8)
    cam.look_from((0.0, 1.0, 6.0))
    cam.look_at((0.0, 0.5, 0.0))
    cam.set_vfov(40.0)
    mats = [Lambertian.new_from_color((0.8, 0.3, 0.3), 1.0), Metal.new((0.8, 0.8, 0.8), 0.1), Dielectric.new(1.5),
            Lambertian.new_from_texture(CheckerTexture.new_from_color(0.5, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9)), 1.0),
            Lambertian.new_from_texture(SolidColor((0.3, 0.3, 0.9)), 0.5)]
    for k in range(n):
        x = (k - (n - 1) / 2.0) * 1.3
        sc.add_element(Sphere.new((x, 0.5 + 0.1 * (k % 3), -0.2 * k), 0.5, mats[k % len(mats)]), f"s{k}")
    return sc


def moving_scene(width=96, samples=6, frame=0, null_motion=False, depth=8):
    """Keyframed primitives that leave their construction-time boxes: 1 fps with a 360 degree shutter, so frame f
    draws ray times in [f, f + 1].  A sphere sweeping 6 units (LERP), one jumping mid-shutter (NERP), one growing
    (radius LERP) then snapping small (radius NERP), a late mover (frame 2), a moving triangle pair, static
    neighbours.  null_motion: the same keys with zero offsets / unchanged radii (refit must then change nothing)."""
    sc = Scene.new_image(16.0 / 9.0, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((0.0, 3.0, 9.0))
    cam.look_at((0.0, 0.7, 0.0))
    cam.set_vfov(35.0)
    cam.frame = frame
    k = 0.0 if null_motion else 1.0
    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, ground), "ground")
    sc.add_element(Sphere.new((-3.0, 0.5, 0.0), 0.5, Lambertian.new_from_color((0.8, 0.2, 0.2), 1.0)), "runner")
    sc.add_element(Sphere.new((0.0, 0.5, -2.0), 0.5, Metal.new((0.8, 0.8, 0.9), 0.05)), "jumper")
    sc.add_element(Sphere.new((2.5, 0.3, 1.5), 0.3, Lambertian.new_from_color((0.2, 0.3, 0.8), 1.0)), "grower")
    sc.add_element(Sphere.new((-2.0, 0.4, 2.5), 0.4, Dielectric.new(1.5)), "late")
    sc.add_element(Sphere.new((3.5, 0.6, -1.0), 0.6, Metal.new((0.9, 0.7, 0.3), 0.2)), "still_a")
    sc.add_element(Sphere.new((-4.0, 0.7, -1.5), 0.7, Lambertian.new_from_color((0.3, 0.7, 0.3), 1.0)), "still_b")
    m_tri = Metal.new((0.7, 0.7, 0.9), 0.1)
    sc.add_element(Triangle.new((-1.0, 0.0, 3.0), (0.0, 0.0, 3.2), (-0.5, 1.2, 3.1), m_tri), "tri_a")
    sc.add_element(Triangle.new((0.0, 0.0, 3.2), (1.0, 0.0, 3.0), (0.5, 1.2, 3.1), m_tri), "tri_b")
    sc.translate_point((6.0 * k, 0.0, 0.0), 1.0, LERP, LOCAL, "runner")
    sc.translate_point((0.0, 1.5 * k, 0.5 * k), 0.5, NERP, LOCAL, "jumper")
    sc.scale_r(0.3 + 0.9 * k, 0.75, LERP, "grower")
    sc.scale_r(0.3 + 0.2 * k, 1.5, NERP, "grower")
    sc.translate_point((0.0, 0.0, -3.0 * k), 2.0, NERP, LOCAL, "late")
    sc.translate_point((4.0 * k, 0.5 * k, 0.0), 3.0, LERP, LOCAL, "late")
    for alias in ("tri_a", "tri_b"):
        sc.translate_point((1.5 * k, 0.8 * k, -1.0 * k), 1.0, LERP, LOCAL, alias)
    return sc


def nan_window_scene(frame, samples=16):
    """moving_scene at 37 x 29 pixels whose camera has no basis for the ray times in [0.97, 1): look_from jumps onto look_at
    at t = 0.97 and back at t = 1 (NERP keys).  Frame 0 draws ray times in [0, 1), so the samples whose time falls into the
    window miss with a NaN direction and the gradient sky makes their colour NaN -- flags beside ordinary magnitudes, in some
    pixels and some samples only; every other frame is ordinary."""
    sc = moving_scene(samples=samples, frame=frame)
    sc.scene_cam.image_width, sc.scene_cam.image_height = 37, 29
    sc.cam_translate_point((0.0, 0.7, 0.0), 0.97, NERP, WORLD, "from")
    sc.cam_translate_point((0.0, 3.0, 9.0), 1.0, NERP, WORLD, "from")
    return sc


def scaled_scene(width=96, samples=6, frame=0, depth=8):
    """Triangles under every non-sphere scale builder (scene_animator.rs:38-229): ScaleX / ScaleY / ScaleZ keys, LERP and
    NERP, scale_point and scale_all_uniform (whose Z key wins, timeline/mod.rs:249-255), mixed with translations; 1 fps
    with a 360 degree shutter, so frame f draws ray times in [f, f + 1] and the keys change inside the exposure.
    Default sky, solid and checker textures only: nothing goes through acos/atan2/asin, so renders are bit-exact."""
    sc = Scene.new_image(16.0 / 9.0, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((1.0, 3.0, 9.0))
    cam.look_at((0.5, 1.0, 0.0))
    cam.set_vfov(38.0)
    cam.frame = frame
    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, ground), "ground")
    sc.add_element(Sphere.new((-3.0, 0.6, 1.0), 0.6, Dielectric.new(1.5)), "glass")
    sc.add_element(Sphere.new((3.4, 0.5, 1.5), 0.5, Metal.new((0.8, 0.8, 0.9), 0.0)), "mirror")
    m_quad = Metal.new((0.7, 0.7, 0.9), 0.1)
    sc.add_element(Triangle.new((0.5, 0.0, -2.0), (2.5, 0.0, -2.0), (2.5, 2.0, -2.2), m_quad), "quad_a")
    sc.add_element(Triangle.new((0.5, 0.0, -2.0), (2.5, 2.0, -2.2), (0.5, 2.0, -2.2), m_quad), "quad_b")
    m_tet = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.4, (0.9, 0.9, 0.2), (0.2, 0.2, 0.2)), 1.0)
    p = [(1.0, 0.0, 1.5), (2.0, 0.0, 1.2), (1.5, 0.0, 2.3), (1.5, 1.0, 1.7)]
    for k, (a, b, c) in enumerate([(0, 1, 3), (1, 2, 3), (2, 0, 3), (0, 2, 1)]):
        sc.add_element(Triangle.new(p[a], p[b], p[c], m_tet), f"tet{k}")
    m_fin = Lambertian.new_from_color((0.8, 0.3, 0.2), 1.0)
    sc.add_element(Triangle.new((-1.5, 0.0, 0.5), (-0.5, 0.0, 0.8), (-1.0, 1.5, 0.6), m_fin), "fin")
    for alias in ("quad_a", "quad_b"):
        sc.scale_x(1.5, 1.0, LERP, alias)                 # X wins until the Y key starts
        sc.scale_y(0.3, 0.5, NERP, alias)                 # from t = 0.5: y' = 0.3 * x + y (row 1, column 0)
        sc.scale_y(-0.2, 2.5, LERP, alias)
    for k in range(4):
        sc.scale_all_uniform(1.3, 1.0, LERP, f"tet{k}")   # X, Y, Z keys over [0, 1]: Z is last and wins
        sc.translate_point((0.4, 0.0, -0.5), 1.5, LERP, LOCAL, f"tet{k}")
        sc.scale_z(0.8, 2.0, NERP, f"tet{k}")
    sc.scale_point((0.5, 2.0, 1.5), 0.25, NERP, "fin")
    sc.translate_point((-0.5, 0.3, 0.0), 0.75, NERP, LOCAL, "fin")
    sc.scale_x(2.0, 1.75, LERP, "fin")
    return sc


def list_scene(width=96, samples=6, frame=0, depth=8, variant="mixed"):
    """HitList elements among ordinary ones (Scene::add_element keeps a list as one object of the BVH build,
    scene/mod.rs:164-166, bvhwrapper.rs:18-22): lists grown by add() (their box is the union, hidden objects
    included), a list from HitList::new(vec) (box stays Aabb::default(): sorted last, its wrapper box never shrinks the
    interval), an empty list, lists of one and two objects, a list inside a list, a hidden object, keyed objects
    (their timelines are filled before they join the list: objects of a list have no alias).
    variant "only_lists": every element is a list; "one_list": the world is a single add()-built list (a span-1
    root: the reference walks the list twice)."""
    sc = Scene.new_image(16.0 / 9.0, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((0.5, 3.0, 9.5))
    cam.look_at((0.0, 0.8, 0.0))
    cam.set_vfov(36.0)
    cam.frame = frame
    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    red, blue = Lambertian.new_from_color((0.8, 0.2, 0.2), 1.0), Lambertian.new_from_color((0.2, 0.3, 0.8), 0.9)
    steel, brass, glass = Metal.new((0.8, 0.8, 0.9), 0.05), Metal.new((0.9, 0.7, 0.3), 0.2), Dielectric.new(1.5)

    # a row of spheres grown by add(); the third is hidden, the fourth moves inside the exposure
    row = HitList.default()
    for k in range(5):
        s = Sphere.new((-4.0 + 1.1 * k, 0.45, 1.0 + 0.3 * k), 0.45, [red, steel, blue, brass, glass][k])
        s.hide = k == 2
        if k == 3:
            s.timeline.translate_point((0.0, 0.8, 0.0), 0.5, LERP, LOCAL)
            s.timeline.scale_sphere(0.6, 1.5, NERP)
        row.add(s)
    # a small mesh (tetrahedron) built the way load_obj does, one triangle scaled by a key
    p = [(1.0, 0.0, 1.5), (2.2, 0.0, 1.2), (1.6, 0.0, 2.5), (1.6, 1.3, 1.7)]
    mesh = HitList.default()
    for k, (a, b, c) in enumerate([(0, 1, 3), (1, 2, 3), (2, 0, 3), (0, 2, 1)]):
        t = Triangle.new(p[a], p[b], p[c], Lambertian.new_from_texture(CheckerTexture.new_from_color(0.4, (0.9, 0.9, 0.2), (0.2, 0.2, 0.2)), 1.0))
        if k == 1:
            t.timeline.scale_x(1.2, 1.0, LERP)
        mesh.add(t)
    # HitList::new(vec): the box stays empty
    loose = HitList.new([Sphere.new((3.2, 0.6, -0.5), 0.6, steel), Sphere.new((3.0, 1.6, -0.6), 0.35, red),
                         Triangle.new((2.0, 0.0, -2.0), (4.5, 0.0, -2.2), (3.2, 2.5, -2.4), brass)])
    # a list inside a list, both grown by add()
    inner = HitList.default()
    inner.add(Sphere.new((-1.0, 0.3, 3.0), 0.3, glass))
    inner.add(Sphere.new((-0.3, 0.3, 3.3), 0.3, blue))
    outer = HitList.default()
    outer.add(Sphere.new((-1.8, 0.35, 3.4), 0.35, brass))
    outer.add(inner)
    outer.add(Triangle.new((-2.5, 0.0, 2.4), (-1.2, 0.0, 2.2), (-1.8, 1.1, 2.3), steel))
    single = HitList.default()
    single.add(Sphere.new((0.2, 0.5, 0.0), 0.5, steel))
    pair = HitList.default()
    pair.add(Sphere.new((0.4, 1.6, -2.5), 0.5, red))
    pair.add(Sphere.new((-0.8, 1.4, -2.5), 0.4, glass))

    if variant == "one_list":
        sc.add_element(row, "row")
        return sc
    if variant != "only_lists":
        sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, ground), "ground")
        sc.add_element(Sphere.new((-3.2, 0.7, -1.5), 0.7, blue), "still")
        sc.add_element(Triangle.new((-5.0, 0.0, -3.0), (-2.5, 0.0, -3.2), (-3.8, 2.2, -3.1), steel), "fin")
        sc.add_element(Sphere.new((4.6, 0.4, 1.8), 0.4, red), "hidden_top")
        sc.hide_element("hidden_top")
        sc.translate_point((0.0, 0.0, 1.5), 1.0, LERP, LOCAL, "still")
    sc.add_element(row, "row")
    sc.add_element(mesh, "mesh")
    sc.add_element(HitList.default(), "nothing")
    sc.add_element(loose, "loose")
    sc.add_element(outer, "outer")
    sc.add_element(single, "single")
    sc.add_element(pair, "pair")
    return sc


def wrapped_scene(width=96, samples=6, frame=0, depth=8, variant="mixed"):
    """BVHWrapper elements (`scene.add_element(BVHWrapper::new_wrapper(list), ..)`, scene/mod.rs:161-163): the outer build
    sorts a wrapper by its root box and a leaf wrapper that holds it walks into it (bvhwrapper.rs:96-126).
    "mixed": wrappers beside spheres, a triangle and a list -- leaves holding (primitive, wrapper), (wrapper, list) ...;
    "only": the world is one wrapper (a span-1 root: the reference walks it twice); "pair": two wrappers (a span-2 root
    of two sub-trees); "small": wrappers of one and of two objects, one without a visible object (an empty list)."""
    sc = Scene.new_image(16.0 / 9.0, width, 1, 360.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((0.5, 3.0, 9.5))
    cam.look_at((0.0, 0.8, 0.0))
    cam.set_vfov(36.0)
    cam.frame = frame
    rs = np.random.RandomState(12)
    mats = [Lambertian.new_from_color((0.8, 0.2, 0.2), 1.0), Metal.new((0.8, 0.8, 0.9), 0.05), Dielectric.new(1.5),
            Lambertian.new_from_texture(CheckerTexture.new_from_color(0.4, (0.9, 0.9, 0.2), (0.2, 0.2, 0.2)), 1.0)]

    def cluster(cx, cz, n, keyed=False, hidden=False):
        objs = []
        for k in range(n):
            if k % 4 == 3:
                c = np.array([cx + rs.uniform(-1, 1), rs.uniform(0.2, 1.0), cz + rs.uniform(-1, 1)])
                o = Triangle.new(*(tuple(c + rs.uniform(-0.4, 0.4, 3)) for _ in range(3)), mats[k % 4])
            else:
                o = Sphere.new((cx + rs.uniform(-1.2, 1.2), rs.uniform(0.2, 0.9), cz + rs.uniform(-1.2, 1.2)), rs.uniform(0.15, 0.35), mats[k % 4])
            if keyed and k == 1:
                o.timeline.translate_point((0.0, 0.9, 0.0), 0.5, LERP, LOCAL)
            if hidden and k == 2:
                o.hide = True      # new_wrapper drops it
            objs.append(o)
        return objs
    big = BVHWrapper.new_wrapper(HitList.new(cluster(-2.0, 0.5, 17, keyed=True, hidden=True)))
    other = BVHWrapper.new_wrapper(HitList.new(cluster(2.5, -0.5, 9)))
    if variant == "only":
        sc.add_element(big, "big")
        return sc
    if variant == "pair":
        sc.add_element(big, "big")
        sc.add_element(other, "other")
        return sc
    ground = Lambertian.new_from_texture(CheckerTexture.new_from_color(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), 1.0)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, ground), "ground")
    if variant == "small":
        sc.add_element(BVHWrapper.new_wrapper(HitList.new(cluster(-2.0, 1.0, 1))), "one")
        sc.add_element(BVHWrapper.new_wrapper(HitList.new(cluster(1.5, 0.0, 2))), "two")
        gone = cluster(0.0, 2.0, 3)
        for o in gone:
            o.hide = True
        sc.add_element(BVHWrapper.new_wrapper(HitList.new(gone)), "none")
        return sc
    sc.add_element(big, "big")
    sc.add_element(Sphere.new((0.0, 0.6, 2.5), 0.6, mats[2]), "glass")
    sc.add_element(other, "other")
    row = HitList.default()
    for o in cluster(-0.5, -2.5, 5):
        row.add(o)
    sc.add_element(row, "row")
    sc.add_element(Triangle.new((-5.0, 0.0, -3.0), (-2.5, 0.0, -3.2), (-3.8, 2.2, -3.1), mats[1]), "fin")
    sc.add_element(BVHWrapper.new_wrapper(HitList.new(cluster(4.5, 2.0, 3))), "third")
    sc.translate_point((0.0, 0.0, 1.0), 1.0, LERP, LOCAL, "glass")
    return sc


def deep_metal_scene(width=8, samples=4, depth=50, sky=True):
    """Paths that bounce many times: a ring of near-white mirrors around the camera between a mirror floor and a
    mirror ceiling, one matte and one glass sphere among them -- long attenuation products, the case where the two product orders of
    CR_SUM_REFERENCE_ORDER and CR_SUM_RELAXED differ most."""
    sc = Scene.new_image(2.0, width, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((0.0, 1.0, 0.0))
    cam.look_at((0.0, 1.0, -1.0))
    cam.set_vfov(70.0)
    sc.add_element(Sphere.new((0.0, -1000.0, 0.0), 1000.0, Metal.new((0.97, 0.95, 0.99), 0.02)), "floor")
    sc.add_element(Sphere.new((0.0, 103.0, 0.0), 100.0, Metal.new((0.98, 0.97, 0.99), 0.05)), "ceiling")
    for k in range(8):
        a = 2.0 * np.pi * k / 8.0
        mat = Metal.new((0.99, 0.9 + 0.01 * k, 0.95), 0.01 * (k % 3))
        if k == 3:
            mat = Lambertian.new_from_color((0.9, 0.8, 0.7), 1.0)
        if k == 6:
            mat = Dielectric.new(1.5)
        sc.add_element(Sphere.new((3.0 * np.sin(a), 1.0, -3.0 * np.cos(a)), 1.4, mat), f"m{k}")
    if sky:
        rs = np.random.RandomState(5)
        sc.load_spherical_skybox(RTWImage(rs.randint(100, 256, size=(8, 16, 3)).astype(np.uint8)))
    return sc


def white_sky_scene(width=2, samples=1):
    """Nothing but a uniform white spherical sky (every texel 255, so every sample's colour is exactly 1.0): the largest
    fixed-point words each scale allows."""
    sc = Scene.new_image(2.0, width, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(4)
    sc.load_spherical_skybox(RTWImage(np.full((4, 8, 3), 255, dtype=np.uint8)))
    return sc


class ArrayScene(Scene):
    """A scene given as arrays of CrPrimitive fields: kind (n,), v (n, 9) and flags (n,), every sphere and triangle with
    one of two materials (matte, metal).  For the tree tests, which need tens of thousands of primitives, list records
    with chosen flags, and values the Sphere / Triangle classes refuse; `elements` stays empty."""

    def __init__(self, kind, v, flags=None, width=48, samples=2):
        import ctypes as C

        from crucible_amd import _abi as A
        from crucible_amd.scene import FlatScene
        super().__init__(16.0 / 9.0, width, 24, 180.0, 1)
        cam = self.scene_cam
        cam.set_samples(samples)
        cam.set_max_depth(6)
        n = len(kind)
        dt = np.dtype([("kind", "<i4"), ("material", "<i4"), ("flags", "<i4"), ("key_first", "<i4"), ("key_count", "<i4"),
                       ("_pad", "<i4"), ("v", "<f8", 9)])
        recs = np.zeros(max(1, n), dtype=dt)
        recs["kind"][:n] = kind
        recs["v"][:n] = v
        recs["flags"][:n] = 0 if flags is None else flags
        recs["material"][:n] = np.where(np.asarray(kind) <= 1, np.arange(n) % 2, 0)
        flat = FlatScene.__new__(FlatScene)
        flat._np = recs
        flat.prims = (A.CrPrimitive * len(recs)).from_buffer(recs)
        flat.textures = (A.CrTexture * 1)(A.CrTexture(A.CR_TEX_SOLID, -1, -1, -1, (C.c_double * 3)(0.7, 0.4, 0.3), 0.0))
        flat.materials = (A.CrMaterial * 2)(A.CrMaterial(A.CR_MAT_LAMBERTIAN, 0, (C.c_double * 3)(0, 0, 0), 1.0),
                                            A.CrMaterial(A.CR_MAT_METAL, -1, (C.c_double * 3)(0.8, 0.8, 0.9), 0.1))
        flat.images = (A.CrImage * 1)()
        flat.keys = (A.CrKeyframe * 1)()
        flat._image_arrays = []
        flat.desc = A.CrSceneDesc(n, 2, 1, 0, 0, A.CR_SKY_DEFAULT, -1, 0, flat.prims, flat.materials, flat.textures,
                                  flat.images, flat.keys)
        self._flat = flat

    def flatten(self):
        self._flat.desc.bvh_mode = self.bvh_mode
        return self._flat


def sah_spheres(centres, radii):
    centres = np.asarray(centres, dtype=np.float64)
    v = np.zeros((len(centres), 9))
    v[:, 0:3] = centres
    v[:, 3] = radii
    return ArrayScene(np.zeros(len(centres), dtype=np.int32), v)


# ---- binned-SAH trees worked out by hand (tests/test_sah_model_host.py, tests/test_gpu_sah_build.py): per scene its
# maker, then children, split_axis (CR_BVH_SAH_ORDERED) and the winning plane of every wrapper in walk order.
# Spheres of radius 1/4 on small dyadic coordinates: every box, centroid, area and cost below is exact in f32 and f64.
# area of a run of j unit-spaced spheres along one axis: the box is (j - 1/2) x 1/2 x 1/2, area 2 j - 1/2.
SAH_HAND = {
    # ext 2, 16 / ext = 8: bins 0, 8, 16 -> 15.  {0}|{1,2} costs 1.5 + 2 * 3.5 = 8.5 at planes 0..7, {0,1}|{2} costs 8.5 at
    # planes 8..14: the tie goes to plane 0.
    "collinear3": (lambda: sah_spheres([[0, 0, 0], [1, 0, 0], [2, 0, 0]], 0.25),
                   [[1, 2], [~0, ~0], [~1, ~2]], [0, -1, -1], [0, -1, -1]),
    # x: {p0,p2}|{p1,p3} at every plane, z: {p0,p1}|{p2,p3}; either side is 1/2 x 1/2 x 3/2, area 3.5, cost 14: x wins
    "square_xz": (lambda: sah_spheres([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], 0.25),
                  [[1, 2], [~0, ~2], [~1, ~3]], [0, -1, -1], [0, -1, -1]),
    # bins 0, 4, 8, 12, 15.  1|4: 1.5 + 4 * 7.5 = 31.5; 2|3 (planes 4..7): 2 * 3.5 + 3 * 5.5 = 23.5; 3|2 (planes 8..11): 23.5;
    # 4|1: 31.5.  The lower plane, 4: {0,1}|{2,3,4}; then {2,3,4} is collinear3 again.
    "line5": (lambda: sah_spheres([[k, 0, 0] for k in range(5)], 0.25),
              [[1, 2], [~0, ~1], [3, 4], [~2, ~2], [~3, ~4]], [0, -1, 0, -1, -1], [4, -1, 0, -1, -1]),
    # one centre, radii 1/4 .. 1: no axis has an extent, mid = start + span // 2, split_axis 0
    "one_centre3": (lambda: sah_spheres([[0.5, -1.25, 2.0]] * 3, [0.25, 0.5, 0.75]),
                    [[1, 2], [~0, ~0], [~1, ~2]], [0, -1, -1], [-1, -1, -1]),
    "one_centre4": (lambda: sah_spheres([[0.5, -1.25, 2.0]] * 4, [0.25, 0.5, 0.75, 1.0]),
                    [[1, 2], [~0, ~1], [~2, ~3]], [0, -1, -1], [-1, -1, -1]),
    # y = 0, 1.875, 2: t = 0, 15, 16.  The centroid at chi is clamped into bin 15 beside its neighbour: no plane parts them.
    "at_chi": (lambda: sah_spheres([[0, 2.0, 0], [0, 0, 0], [0, 1.875, 0]], 0.25),
               [[1, 2], [~1, ~1], [~0, ~2]], [1, -1, -1], [0, -1, -1]),
}


def subnormal_extent_scene():
    """Six triangles flat along x, at x = 0 (thin in y) and x = 1e-310 (tall in y) alternately, all long in z with
    centroids a unit apart.  In f64 the x extent of the centroids is 1e-310 and 16 / ext overflows: t = 0 * inf = NaN for
    the first group (bin 0) and inf for the second (bin 15).  That split -- thin | tall -- is the cheapest, so the tree
    rests on bin_index's two clamps.  In f32 both x are 0 and only z is a candidate."""
    rows = []
    for i in range(6):
        x, h, z = (0.0, 1.0, float(i // 2)) if i % 2 == 0 else (1e-310, 5.0, float(i // 2))
        rows.append([x, -h, z, x, h, z, x, -h, z + 10.0])
    return ArrayScene(np.full(6, 1, dtype=np.int32), np.array(rows))


# (real_type, tag, sum_order) cases of the bit-exact GPU suites: both precisions in the reference order (ids "f64" and
# "f32", as the suites had them) and in CR_SUM_RELAXED, the library default ("f64-relaxed", "f32-relaxed"), each held to
# the oracle in the same order.  Use as @pytest.mark.parametrize("rt,tag,order", REAL_ORDERS, ids=REAL_ORDER_IDS).
def _real_orders():
    from crucible_amd import _abi as A
    reals = [(A.CR_REAL_F64, "f64"), (A.CR_REAL_F32, "f32")]
    cases = [(rt, tag, A.CR_SUM_REFERENCE_ORDER) for rt, tag in reals] + [(rt, tag, A.CR_SUM_RELAXED) for rt, tag in reals]
    return cases, [tag if order == A.CR_SUM_REFERENCE_ORDER else tag + "-relaxed" for _, tag, order in cases]


REAL_ORDERS, REAL_ORDER_IDS = _real_orders()


def mirror_box_scene(size=80.0, gap=1e-4, samples=2, depth=70000, albedo=0.99999):
    """Paths of tens of thousands of bounces: the camera inside a closed box of 12 mirror triangles (Metal, fuzz 0,
    albedo just below 1), `size` units wide.  One of the two triangles of the top face is drawn short by `gap` of its
    edge, which leaves a small triangle of the face out: the way to the sky.  (A path also leaves where it meets a wall
    within 0.001 of an edge -- the hit interval starts there -- which is why the box is large.)  The corners are moved off
    the axis-aligned box by up to 1 % of its size: a triangle flat along an axis has a box without thickness and never hits
    when it is alone in its leaf (bvh.rs:126), and walls that are not quite parallel spread the bounce counts.
    4 x 4 pixels: every path has a lane of one workgroup, so a reference-order attenuation stack of max_depth records
    stays below 1 GB."""
    sc = Scene.new_image(1.0, 4, 24, 180.0, 1)
    cam = sc.scene_cam
    cam.set_samples(samples)
    cam.set_max_depth(depth)
    cam.look_from((0.07 * size, -0.03 * size, 0.05 * size))
    cam.look_at((0.4 * size, 0.31 * size, -0.5 * size))
    cam.set_vfov(80.0)
    h = 0.5 * size
    rs = np.random.RandomState(7)
    c = {(i, j, k): (h * i + 0.01 * size * rs.uniform(-1, 1), h * j + 0.01 * size * rs.uniform(-1, 1), h * k + 0.01 * size * rs.uniform(-1, 1))
         for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)}
    mirror = Metal.new((albedo, albedo, albedo), 0.0)
    faces = []
    for axis in range(3):
        for side in (-1, 1):
            q = []
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                key = [a, b]
                key.insert(axis, side)
                q.append(c[tuple(key)])
            faces.append(q)
    n = 0
    for f, q in enumerate(faces):
        sc.add_element(Triangle.new(q[0], q[1], q[2], mirror), f"w{n}")
        last = q[3]
        if f == 3:   # the top face (y = +size / 2): its second triangle stops short of the corner
            last = tuple(q[3][k] + gap * (q[0][k] - q[3][k]) for k in range(3))
        sc.add_element(Triangle.new(q[0], q[2], last, mirror), f"w{n + 1}")
        n += 2
    return sc


def extent_scene(width, height, samples, keyed=False):
    """A row of five spheres seen as a width x height image whose long side spans about 8 units at the focus distance,
    however thin the other side is (65537 x 1: a strip one pixel high across the row), so that the far ends of the long
    side still meet spheres, the ground and the sky.  keyed: the camera moves between frames (a frame batch's frames differ)."""
    sc = few_spheres(5, samples=samples)
    sc.add_element(Sphere.new((0.0, -100.0, 0.0), 100.0, Lambertian.new_from_color((0.5, 0.6, 0.4), 1.0)), "ground")
    cam = sc.scene_cam
    cam.image_width, cam.image_height = int(width), int(height)
    cam.set_max_depth(4)
    cam.look_at((0.0, 0.45, 0.0))
    import math
    vh = 8.0 * min(1.0, height / width)   # the viewport's height at the focus distance (10): its width is vh * width / height
    cam.set_vfov(math.degrees(2.0 * math.atan(vh / 20.0)))
    if keyed:
        sc.cam_translate_point((0.4, 1.3, 6.2), 0.03, LERP, WORLD, "from")
        sc.cam_translate_point((0.1, 0.5, 0.0), 0.06, NERP, WORLD, "at")
    return sc


def keyed_camera_scene(n_from=300, n_at=212, amp=0.3, width=8):
    """n_from + n_at camera keyframes (CrHandle::kMaxCamKeys is 512): translations of look_from and look_at, LERP and NERP
    in turn, every one with its own end time (a LERP key starts where the previous key of its axis ended, so 151 start times are
    distinct among the 300 look_from keys and the rest tie with a NERP key), spread over [0, 0.09] -- frame 1 at 24 fps with a 180 degree shutter draws
    ray times in [1/24, 1/16], so keys lie before, inside and after the exposure.  amp scales every displacement (another
    amp: another key set of the same shape)."""
    sc = few_spheres(4, width=width, samples=3)
    cam = sc.scene_cam
    cam.image_width, cam.image_height = width, width
    cam.frame = 1
    rs = np.random.RandomState(99)
    for tl, base, n, dt in ((cam.look_from_tl, (0.0, 1.0, 6.0), n_from, 0.0009), (cam.look_at_tl, (0.0, 0.5, 0.0), n_at, 0.0012)):
        for k in range(n):
            axis, step = k % 3, k // 3
            t = dt * (step + 1) + 0.0001 * axis
            value = base[axis] + amp * rs.uniform(-1.0, 1.0)
            (tl.translate_x, tl.translate_y, tl.translate_z)[axis](value, t, LERP if (step + axis) % 2 == 0 else NERP, WORLD)
    return sc
