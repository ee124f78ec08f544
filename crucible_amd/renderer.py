"""ctypes binding of libcrucible_hip.so (include/crucible_hip.h).

This is the only route to pixels in the package: if the HIP library is missing
or no GPU is present, construction raises -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRUCIBLE_HIP_LIB") or os.path.join(_HERE, "libcrucible_hip.so")   # override: diagnostic builds only
_lib = None


class CrucibleError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"crucible_hip error {code}: {msg}")
        self.code = code


def load_library():
    """dlopen the in-tree library and bind every symbol the header declares."""
    global _lib
    if _lib is None:
        # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64; if this
        # library pulled in /opt/rocm's copies first, torch would later load a second runtime that finds no
        # GPU.  Importing torch first makes both share one (measured on the MI355X box, ROCm 7.2 + torch 2.10).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "or `make -C crucible_amd/csrc`")
        _lib = A.bind(C.CDLL(LIB_PATH))
        if _lib.cr_abi_version() != A.CR_ABI_VERSION:
            raise RuntimeError("libcrucible_hip.so ABI version mismatch")
    return _lib


def np_real(real_type):
    return np.float64 if real_type == A.CR_REAL_F64 else np.float32


def update_arrays(indices, values):
    """(index pointer or None, contiguous (n, 9) float64 rows, n) for cr_update_primitives; the index array stays
    alive through the returned pointer object."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, 9)
    if indices is None:
        return None, v, len(v)
    idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    if idx.size != len(v):
        raise ValueError(f"update_primitives: {idx.size} indices for {len(v)} rows")
    ptr = idx.ctypes.data_as(C.POINTER(C.c_int32))
    ptr._keep = idx
    return ptr, v, len(v)


def _table(records, ctype):
    """(ctypes array or None, count) of a table argument: None stays None (the table is kept); a ctypes array passes
    through; any other sequence of `ctype` records is copied.  An empty table is still a table (one unused record)."""
    if records is None:
        return None, 0
    if isinstance(records, C.Array) and records._type_ is ctype:
        return records, len(records)
    records = list(records)
    return (ctype * max(1, len(records)))(*records), len(records)


def material_arrays(materials=None, textures=None, assign=None):
    """cr_update_materials' arguments after the handle: (materials, n_materials, textures, n_textures, prim_index,
    prim_material, n_assign).  materials / textures: None (kept) or the whole new table, a sequence of A.CrMaterial /
    A.CrTexture.  assign: None, a mapping {primitive index: material index} or a pair (indices, materials)."""
    mats, n_m = _table(materials, A.CrMaterial)
    texs, n_t = _table(textures, A.CrTexture)
    if assign is None:
        return mats, n_m, texs, n_t, None, None, 0
    if hasattr(assign, "items"):
        assign = (list(assign.keys()), list(assign.values()))
    idx = np.ascontiguousarray(assign[0], dtype=np.int32).reshape(-1)
    mat = np.ascontiguousarray(assign[1], dtype=np.int32).reshape(-1)
    if idx.size != mat.size:
        raise ValueError(f"update_materials: {idx.size} indices for {mat.size} materials")
    ptrs = []
    for a in (idx, mat):
        ptr = a.ctypes.data_as(C.POINTER(C.c_int32))
        ptr._keep = a
        ptrs.append(ptr)
    return mats, n_m, texs, n_t, ptrs[0], ptrs[1], int(idx.size)


def shading_arrays(flat):
    """material_arrays of "this description, same geometry": both tables of the flattened scene `flat` (what Scene.flatten
    makes for upload_scene) and the material of every sphere and triangle."""
    d = getattr(flat, "desc", flat)
    mats = C.cast(d.materials, C.POINTER(A.CrMaterial * max(1, d.n_materials))).contents
    texs = C.cast(d.textures, C.POINTER(A.CrTexture * max(1, d.n_textures))).contents
    words = C.sizeof(A.CrPrimitive) // 4
    if d.n_prims > 0:
        rec = np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_int32)), shape=(d.n_prims, words))
        idx = np.flatnonzero((rec[:, 0] == A.CR_PRIM_SPHERE) | (rec[:, 0] == A.CR_PRIM_TRIANGLE)).astype(np.int32)
        assign = (idx, rec[idx, 1].copy())
    else:
        assign = None
    out = material_arrays(None, None, assign)
    return (mats, d.n_materials, texs, d.n_textures) + out[4:]


def image_arrays(rgb8, rect=None):
    """cr_update_image's arguments after the image index: (x0, y0, width, height, bytes pointer).  rgb8: (height, width, 3)
    uint8; rect = (x0, y0, width, height), or None: the array's own size at (0, 0)."""
    px = np.ascontiguousarray(rgb8, dtype=np.uint8)
    if rect is None:
        if px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("update_image: rgb8 must be (height, width, 3) when no rect is given")
        rect = (0, 0, px.shape[1], px.shape[0])
    x0, y0, w, h = (int(v) for v in rect)
    if px.size != max(0, w) * max(0, h) * 3:
        raise ValueError(f"update_image: {px.size} bytes for a {w} x {h} rectangle")
    ptr = px.ctypes.data_as(C.POINTER(C.c_uint8))
    ptr._keep = px
    return x0, y0, w, h, ptr


class Renderer:
    """One CrHandle (one HIP device).  Mirrors the call `Camera::render(&skybox, &world, fname)`
    (reference src/camera/mod.rs:270) split into upload_scene / render / write_ppm."""

    def __init__(self, device=0, sum_order=A.CR_SUM_DEFAULT):
        self.lib = load_library()
        # CrRenderParams.sum_order of this renderer's renders unless a call names its own: CR_SUM_DEFAULT is the
        # library's choice (relaxed), CR_SUM_REFERENCE_ORDER the parity mode the bit-exact tests run in
        self.sum_order = sum_order
        h = C.c_void_p()
        rc = self.lib.cr_create(device, C.byref(h))
        if rc != A.CR_OK:
            raise CrucibleError(rc, (self.lib.cr_last_error(None) or b"").decode())
        self.h = h

    def _check(self, rc):
        if rc != A.CR_OK:
            raise CrucibleError(rc, (self.lib.cr_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            self.lib.cr_destroy(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()

    def upload_scene(self, flat):
        self._check(self.lib.cr_upload_scene(self.h, C.byref(flat.desc)))

    def update_primitives(self, indices, values, rebuild=False):
        """cr_update_primitives: new CrPrimitive.v rows (n, 9) for the primitives `indices` (positions in the uploaded
        description; None: 0..n-1) of the scene on this handle.  A sphere reads four values of its row.
        rebuild=False refits the boxes of the trees already built, topology unchanged; rebuild=True has the trees
        rebuilt at next use, as a fresh upload of the edited scene would."""
        idx, v, n = update_arrays(indices, values)
        self._check(self.lib.cr_update_primitives(self.h, idx, v.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                  A.CR_UPDATE_REBUILD if rebuild else A.CR_UPDATE_REFIT))

    def update_materials(self, materials=None, textures=None, assign=None):
        """cr_update_materials: replace the material and / or texture table of the scene on this handle (None: kept;
        else the whole new table) and give primitives another material (assign: {primitive index: material index} or
        a pair of sequences).  The tree is not rebuilt; the handle then behaves as after an upload of the edited
        description."""
        self._check(self.lib.cr_update_materials(self.h, *material_arrays(materials, textures, assign)))

    def update_shading(self, flat):
        """This description, same geometry: both tables of the flattened scene `flat` and the material of every sphere
        and triangle, through cr_update_materials."""
        self._check(self.lib.cr_update_materials(self.h, *shading_arrays(flat)))

    def update_image(self, index, rgb8, rect=None):
        """cr_update_image: new texels for the rectangle rect = (x0, y0, width, height) of image `index` of the last
        upload (None: the whole (height, width, 3) array at the image's origin)."""
        self._check(self.lib.cr_update_image(self.h, index, *image_arrays(rgb8, rect)))

    def set_sky(self, kind, image=-1):
        """cr_set_sky: A.CR_SKY_DEFAULT, or A.CR_SKY_SPHERICAL with the index of an uploaded image."""
        self._check(self.lib.cr_set_sky(self.h, kind, image))

    def _args(self, cam, seed, real_type, sample_begin=0, sample_count=None, output_sum=False, sum_order=None):
        """(CrCameraDesc, CrRenderParams) of a call; sum_order=None: this renderer's."""
        return cam.desc(), cam.params(seed, real_type, sample_begin, sample_count, output_sum, self.sum_order if sum_order is None else sum_order)

    def _call(self, name, args, *rest, want_stats, stats=A.CrStats):
        """The entry point `name` with (handle, camera, params, *rest, stats or a null pointer), checked.  Returns the
        stats struct (zeros without want_stats)."""
        cd, p = args
        st = stats()
        self._check(getattr(self.lib, name)(self.h, C.byref(cd), C.byref(p), *rest, C.byref(st) if want_stats else None))
        return st

    def render(self, cam, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False,
               want_stats=True, sum_order=None):
        """Render into a host array (H, W, 3) of f32/f64 -- of uint64 words with output_sum=A.CR_OUTPUT_FIXED_SUM.
        Returns (image, stats dict)."""
        out, _ = frame_arrays((cam.image_height, cam.image_width), out_dtype(output_sum, real_type))
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_host", args, host_ptr(out), want_stats=want_stats)
        return out, st.as_dict()

    def render_device(self, cam, d_ptr, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                      output_sum=False, want_stats=False, sum_order=None):
        """Render into device memory at `d_ptr` (W*H*3 reals, or uint64 words with output_sum=A.CR_OUTPUT_FIXED_SUM).
        Asynchronous unless want_stats."""
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_device", args, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_frames(self, cam, frames, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                      output_sum=False, want_stats=True, sum_order=None):
        """cr_render_frames_host: the frames `frames` (frame indices; cam.frame is not used) in one launch, as an
        (F, H, W, 3) host array of f32/f64 -- of uint64 words with output_sum=A.CR_OUTPUT_FIXED_SUM.  Frame k equals
        render() at frame frames[k] bit for bit.  Needs CR_SUM_RELAXED.  Returns (frames array, stats dict)."""
        fr, fr_ptr = frame_list(frames)
        out, _ = frame_arrays((max(1, fr.size), cam.image_height, cam.image_width), out_dtype(output_sum, real_type))
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_frames_host", args, fr_ptr, fr.size, host_ptr(out), want_stats=want_stats)
        return out, st.as_dict()

    def render_frames_device(self, cam, frames, d_ptr, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                             sample_count=None, output_sum=False, want_stats=False, sum_order=None):
        """cr_render_frames_device: the frames `frames` into device memory at `d_ptr` (F*W*H*3 reals, or uint64 words
        with output_sum=A.CR_OUTPUT_FIXED_SUM), frame after frame.  Asynchronous unless want_stats."""
        fr, fr_ptr = frame_list(frames)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_frames_device", args, fr_ptr, fr.size, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov(self, cam, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                   output_sum=False, want_stats=True):
        """cr_render_aov_host: the first-hit guide layers `layers` (a CR_AOV_* mask, or names such as
        ("albedo", "depth")) of the primary rays of render() with the same camera and params.  Returns (dict of host
        arrays keyed "albedo" (H, W, 3), "normal" (H, W, 3; decode 2 e - 1), "depth" (H, W), "coverage" (H, W) -- the
        requested ones --, stats dict)."""
        layers = aov_mask(layers)
        H, W = cam.image_height, cam.image_width
        buf, planes = guide_buffer(layers, real_type, W, H)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._call("cr_render_aov_host", args, layers, host_ptr(buf), want_stats=want_stats)
        return guide_planes(buf, planes, W, H), st.as_dict()

    def render_aov_device(self, cam, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                          sample_count=None, output_sum=False, want_stats=False):
        """cr_render_aov_device: the requested planes, one after the other in ascending bit order, into device memory at
        `d_ptr`.  Asynchronous unless want_stats."""
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._call("cr_render_aov_device", args, aov_mask(layers), C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_frames(self, cam, frames, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                          sample_count=None, output_sum=False, want_stats=True):
        """cr_render_aov_frames_host: the guide layers `layers` of the frames `frames` (frame indices; cam.frame is not
        used) in one launch.  Returns (list of per-frame dicts shaped like render_aov's, stats dict of the whole call);
        frame k equals render_aov() at frame frames[k] bit for bit."""
        layers = aov_mask(layers)
        fr, fr_ptr = frame_list(frames)
        H, W = cam.image_height, cam.image_width
        buf, planes = guide_buffer(layers, real_type, W, H, fr.size)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._call("cr_render_aov_frames_host", args, layers, fr_ptr, fr.size, host_ptr(buf), want_stats=want_stats)
        return [guide_planes(buf, planes, W, H, k) for k in range(fr.size)], st.as_dict()

    def render_aov_frames_device(self, cam, frames, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32,
                                 sample_begin=0, sample_count=None, output_sum=False, want_stats=False):
        """cr_render_aov_frames_device: frame after frame into device memory at `d_ptr`, each frame's requested planes
        one after the other in ascending bit order.  Asynchronous unless want_stats."""
        fr, fr_ptr = frame_list(frames)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._call("cr_render_aov_frames_device", args, aov_mask(layers), fr_ptr, fr.size, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def _views_call(self, name, cams, frames, params_of, *rest, want_stats):
        """The views entry point `name` with (handle, the cameras' descriptors, their number, frames or a null pointer, the
        params of cams[0], *rest, stats or a null pointer), checked.  Returns the stats struct."""
        descs, keep = view_table(cams)
        fr, fr_ptr = frame_list(frames)
        p = params_of(cams[0]) if cams else None
        st = A.CrStats()
        self._check(getattr(self.lib, name)(self.h, descs, len(cams) if cams is not None else 0, fr_ptr, C.byref(p) if p is not None else None, *rest,
                                            C.byref(st) if want_stats else None))
        del keep
        return st

    def render_views(self, cams, frames=None, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                     output_sum=False, want_stats=True, sum_order=None):
        """cr_render_views_host: the cameras `cams` (one image size; samples, depth, frame rate and shutter are cams[0]'s) in
        one launch, as a (V, H, W, 3) host array shaped like render_frames'.  frames: one frame index per view, None: cams[0].frame
        for every view.  View k equals render() of cams[k] at frame frames[k] bit for bit.  Needs CR_SUM_RELAXED.  Returns
        (views array, stats dict of the whole call)."""
        n = len(cams) if cams else 0
        H, W = (cams[0].image_height, cams[0].image_width) if n else (1, 1)
        out, _ = frame_arrays((max(1, n), H, W), out_dtype(output_sum, real_type))
        params = lambda c: c.params(seed, real_type, sample_begin, sample_count, output_sum, self.sum_order if sum_order is None else sum_order)
        st = self._views_call("cr_render_views_host", cams, frames, params, host_ptr(out), want_stats=want_stats)
        return out, st.as_dict()

    def render_views_device(self, cams, d_ptr, frames=None, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                            output_sum=False, want_stats=False, sum_order=None):
        """cr_render_views_device: view after view into device memory at `d_ptr` (V*W*H*3 reals, or uint64 words with
        output_sum=A.CR_OUTPUT_FIXED_SUM).  Asynchronous unless want_stats."""
        params = lambda c: c.params(seed, real_type, sample_begin, sample_count, output_sum, self.sum_order if sum_order is None else sum_order)
        st = self._views_call("cr_render_views_device", cams, frames, params, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_views(self, cams, frames=None, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                         sample_count=None, output_sum=False, want_stats=True):
        """cr_render_aov_views_host: the guide layers `layers` of the cameras `cams` in one launch.  Returns (list of per-view
        dicts shaped like render_aov's, stats dict of the whole call); view k equals render_aov() of cams[k] at frame
        frames[k] bit for bit."""
        layers = aov_mask(layers)
        n = len(cams) if cams else 0
        H, W = (cams[0].image_height, cams[0].image_width) if n else (1, 1)
        buf, planes = guide_buffer(layers, real_type, W, H, n)
        params = lambda c: c.params(seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._views_call("cr_render_aov_views_host", cams, frames, params, layers, host_ptr(buf), want_stats=want_stats)
        return [guide_planes(buf, planes, W, H, k) for k in range(n)], st.as_dict()

    def render_aov_views_device(self, cams, d_ptr, frames=None, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32,
                                sample_begin=0, sample_count=None, output_sum=False, want_stats=False):
        """cr_render_aov_views_device: view after view into device memory at `d_ptr`, each view's requested planes one after
        the other in ascending bit order.  Asynchronous unless want_stats."""
        params = lambda c: c.params(seed, real_type, sample_begin, sample_count, output_sum, A.CR_SUM_DEFAULT)
        st = self._views_call("cr_render_aov_views_device", cams, frames, params, aov_mask(layers), C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_region(self, cam, region, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False,
                      want_stats=True, sum_order=None):
        """cr_render_region_host: the pixels `region` = (x0, y0, w, h) of the frame `cam` describes, as an (h, w, 3) host
        array of f32/f64 -- of uint64 words with output_sum=A.CR_OUTPUT_FIXED_SUM.  Pixel (i, j) equals pixel
        (x0 + i, y0 + j) of render() bit for bit; region=None passes a null pointer (the library refuses it).  Needs
        CR_SUM_RELAXED.  Returns (image, stats dict of the region's samples)."""
        reg, (w, h) = region_arg(region)
        out, _ = frame_arrays((max(1, h), max(1, w)), out_dtype(output_sum, real_type))
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_region_host", args, reg, host_ptr(out), want_stats=want_stats)
        return out, st.as_dict()

    def render_region_device(self, cam, region, d_ptr, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                             output_sum=False, want_stats=False, sum_order=None):
        """cr_render_region_device: the region into device memory at `d_ptr` (w*h*3 reals, or uint64 words with
        output_sum=A.CR_OUTPUT_FIXED_SUM).  Asynchronous unless want_stats."""
        reg, _ = region_arg(region)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_region_device", args, reg, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_region(self, cam, region, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                          sample_count=None, output_sum=False, want_stats=True, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_region_host: render_aov's planes over the pixels `region` = (x0, y0, w, h): a dict of (h, w, 3) /
        (h, w) host arrays, each the crop of render_aov's plane bit for bit, and the stats dict of the region's samples."""
        layers = aov_mask(layers)
        reg, (w, h) = region_arg(region)
        w, h = max(1, w), max(1, h)
        buf, planes = guide_buffer(layers, real_type, w, h)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_region_host", args, layers, reg, host_ptr(buf), want_stats=want_stats)
        return guide_planes(buf, planes, w, h), st.as_dict()

    def render_aov_region_device(self, cam, region, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0,
                                 sample_count=None, output_sum=False, want_stats=False, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_region_device: the region's requested planes, one after the other in ascending bit order, into
        device memory at `d_ptr`.  Asynchronous unless want_stats."""
        reg, _ = region_arg(region)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_region_device", args, aov_mask(layers), reg, C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_counts(self, cam, counts, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False, want_stats=True,
                          sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_host: render_aov's planes with pixel p taking the samples [0, n_p), n_p the value of the
        (H, W) int32 plane `counts` clamped to [0, cam.samples] -- with render_adaptive's counts, the guide layers of
        that adaptive frame.  A pixel with n_p >= 1 equals render_aov() at samples = n_p bit for bit (up to 2047
        samples); n_p == 0 gives 0 and +inf depth.  counts=None passes a null pointer (the library refuses it).
        Returns (dict of planes as render_aov, stats dict: samples == segments == the sum of n_p)."""
        layers = aov_mask(layers)
        H, W = cam.image_height, cam.image_width
        plane = count_plane(counts, (H, W))
        buf, planes = guide_buffer(layers, real_type, W, H)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_host", args, layers, host_ptr(plane), host_ptr(buf), want_stats=want_stats)
        return guide_planes(buf, planes, W, H), st.as_dict()

    def render_aov_counts_device(self, cam, d_counts, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False,
                                 want_stats=False, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_device: the plane at device pointer `d_counts` (W*H int32), the requested planes into device
        memory at `d_ptr` as render_aov_device lays them out.  Asynchronous unless want_stats."""
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_device", args, aov_mask(layers), dev_ptr(d_counts), C.c_void_p(d_ptr), want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_counts_frames(self, cam, frames, counts, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False,
                                 want_stats=True, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_frames_host: the frames `frames` in one launch, frame k at the plane counts[k] ((n, H, W)
        int32, as render_adaptive_frames returns it).  Returns (list of per-frame dicts, stats dict of the whole call);
        frame k equals render_aov_counts() at frame frames[k] with counts[k] bit for bit."""
        layers = aov_mask(layers)
        fr, fr_ptr = frame_list(frames)
        H, W = cam.image_height, cam.image_width
        plane = count_plane(counts, (max(1, fr.size), H, W))
        buf, planes = guide_buffer(layers, real_type, W, H, fr.size)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_frames_host", args, layers, fr_ptr, fr.size, host_ptr(plane), host_ptr(buf), want_stats=want_stats)
        return [guide_planes(buf, planes, W, H, k) for k in range(fr.size)], st.as_dict()

    def render_aov_counts_frames_device(self, cam, frames, d_counts, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                                        output_sum=False, want_stats=False, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_frames_device: the planes at `d_counts` (n*W*H int32, frame after frame), the frames into
        device memory at `d_ptr` as render_aov_frames_device lays them out.  Asynchronous unless want_stats."""
        fr, fr_ptr = frame_list(frames)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_frames_device", args, aov_mask(layers), fr_ptr, fr.size, dev_ptr(d_counts), C.c_void_p(d_ptr),
                        want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_aov_counts_region(self, cam, region, counts, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None, output_sum=False,
                                 want_stats=True, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_region_host: render_aov_counts over the pixels `region` = (x0, y0, w, h) with the (h, w) int32
        plane `counts` of the region (as render_adaptive_region returns it): with the crop of a frame's plane, the crop of
        render_aov_counts' planes bit for bit."""
        layers = aov_mask(layers)
        reg, (w, h) = region_arg(region)
        w, h = max(1, w), max(1, h)
        plane = count_plane(counts, (h, w))
        buf, planes = guide_buffer(layers, real_type, w, h)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_region_host", args, layers, reg, host_ptr(plane), host_ptr(buf), want_stats=want_stats)
        return guide_planes(buf, planes, w, h), st.as_dict()

    def render_aov_counts_region_device(self, cam, region, d_counts, d_ptr, layers=A.CR_AOV_ALL, *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                                        output_sum=False, want_stats=False, sum_order=A.CR_SUM_DEFAULT):
        """cr_render_aov_counts_region_device: the region's plane at `d_counts` (w*h int32), its requested planes into device
        memory at `d_ptr`.  Asynchronous unless want_stats."""
        reg, _ = region_arg(region)
        args = self._args(cam, seed, real_type, sample_begin, sample_count, output_sum, sum_order)
        st = self._call("cr_render_aov_counts_region_device", args, aov_mask(layers), reg, dev_ptr(d_counts), C.c_void_p(d_ptr),
                        want_stats=want_stats)
        return st.as_dict() if want_stats else None

    def render_tiled(self, cam, tile=(1024, 1024), *, seed, real_type=A.CR_REAL_F32, sample_begin=0, sample_count=None,
                     output_sum=False, sum_order=None, adaptive=None):
        """A whole frame assembled from render_region() calls over tiles of `tile` = (tw, th) pixels (edge tiles are
        smaller): render()'s frame bit for bit, and the way to a frame of more than 2^26 pixels (up to 2^31 - 1).  Returns
        (image (H, W, 3), stats dict: the regions' counters, samples, nan_pixels and kernel_ms summed; the rest from the
        last region).

        adaptive=dict(tolerance=, min_samples=, pass_samples=, block=16): each tile through render_adaptive_region()
        instead -- render_adaptive()'s frame and counts bit for bit.  The tile's sides must be multiples of `block`
        (ValueError otherwise: the tiles' blocks would not be the frame's and the result would depend on the tiling).
        Returns (image, counts (H, W) int32, stats dict shaped like render_adaptive's: the counters, samples, nan_pixels,
        kernel_ms, judge_ms, passes, blocks and blocks_stopped summed over the calls; the rest from the last)."""
        tw, th = int(tile[0]), int(tile[1])
        if tw < 1 or th < 1:
            raise ValueError("render_tiled: tile sizes must be positive")
        if adaptive is not None:
            return self._render_tiled_adaptive(cam, tw, th, dict(adaptive), seed=seed, real_type=real_type, sample_begin=sample_begin,
                                               sample_count=sample_count, output_sum=output_sum, sum_order=sum_order)
        H, W = cam.image_height, cam.image_width
        out = np.empty((H, W, 3), dtype=out_dtype(output_sum, real_type))
        total = None
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                w, h = min(tw, W - x0), min(th, H - y0)
                img, st = self.render_region(cam, (x0, y0, w, h), seed=seed, real_type=real_type, sample_begin=sample_begin,
                                             sample_count=sample_count, output_sum=output_sum, sum_order=sum_order)
                out[y0:y0 + h, x0:x0 + w] = img
                total = add_stats(total, st)
        return out, total

    def _render_tiled_adaptive(self, cam, tw, th, adaptive, *, seed, real_type, sample_begin, sample_count, output_sum, sum_order):
        """render_tiled(adaptive=...): the checks need no device and come before the first call."""
        block = int(adaptive.pop("block", 16) or 16)
        if tw % block or th % block:
            raise ValueError(f"render_tiled: an adaptive tile's sides must be multiples of the block's ({block}): {tw}x{th} "
                             "would make the frame depend on the tiling")
        if sample_begin != 0 or sample_count is not None or output_sum:
            raise ValueError("render_tiled: an adaptive frame takes all samples of a pixel and comes as means")
        H, W = cam.image_height, cam.image_width
        out = np.empty((H, W, 3), dtype=np_real(real_type))
        counts = np.empty((H, W), dtype=np.int32)
        total = None
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                w, h = min(tw, W - x0), min(th, H - y0)
                img, cnt, st = self.render_adaptive_region(cam, (x0, y0, w, h), seed=seed, real_type=real_type, block=block,
                                                           sum_order=sum_order, **adaptive)
                out[y0:y0 + h, x0:x0 + w] = img
                counts[y0:y0 + h, x0:x0 + w] = cnt
                total = add_stats(total, st)
        return out, counts, total

    def render_adaptive(self, cam, *, seed, real_type=A.CR_REAL_F32, tolerance, min_samples, pass_samples, block=16,
                        want_counts=True, want_stats=True, sum_order=None):
        """cr_render_adaptive_host: the frame to a noise target -- cam.samples is the maximum per pixel, blocks of `block`
        (8, 16 or 32) pixels square stop once the mean absolute difference of their two half-frame means is at most
        `tolerance` (the exact rule: include/crucible_hip.h).  Needs CR_SUM_RELAXED.  Returns (image (H, W, 3), counts
        (H, W) int32 or None, stats dict: passes, blocks, blocks_stopped, judge_ms, and the render's CrStats under
        "render")."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        out, counts = frame_arrays((cam.image_height, cam.image_width), np_real(real_type), want_counts)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_host", args, C.byref(ap), host_ptr(out), host_ptr(counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return out, counts, st.as_dict()

    def render_adaptive_device(self, cam, d_ptr, d_counts=None, *, seed, real_type=A.CR_REAL_F32, tolerance, min_samples,
                               pass_samples, block=16, want_stats=True, sum_order=None):
        """cr_render_adaptive_device: the frame into device memory at `d_ptr` (W*H*3 reals) and, if given, the counts at
        `d_counts` (W*H int32).  Synchronous.  Returns the stats dict of render_adaptive."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_device", args, C.byref(ap), C.c_void_p(d_ptr), dev_ptr(d_counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return st.as_dict()

    def render_adaptive_frames(self, cam, frames, *, seed, real_type=A.CR_REAL_F32, tolerance, min_samples, pass_samples, block=16,
                               want_counts=True, want_stats=True, sum_order=None):
        """cr_render_adaptive_frames_host: the frames `frames` (frame indices; cam.frame is not used) to a noise target
        under one pass loop -- a pass renders the active tiles of all frames in one launch.  Frame k and its counts are
        render_adaptive() at frame frames[k] bit for bit.  Returns (images (n, H, W, 3), counts (n, H, W) int32 or None,
        stats dict of the whole call, shaped like render_adaptive's)."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        fr, fr_ptr = frame_list(frames)
        out, counts = frame_arrays((max(1, fr.size), cam.image_height, cam.image_width), np_real(real_type), want_counts)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_frames_host", args, C.byref(ap), fr_ptr, fr.size, host_ptr(out), host_ptr(counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return out, counts, st.as_dict()

    def render_adaptive_frames_device(self, cam, frames, d_ptr, d_counts=None, *, seed, real_type=A.CR_REAL_F32, tolerance,
                                      min_samples, pass_samples, block=16, want_stats=True, sum_order=None):
        """cr_render_adaptive_frames_device: the frames into device memory at `d_ptr` (n*W*H*3 reals, frame after frame)
        and, if given, the counts at `d_counts` (n*W*H int32).  Synchronous.  Returns the stats dict of render_adaptive."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        fr, fr_ptr = frame_list(frames)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_frames_device", args, C.byref(ap), fr_ptr, fr.size, C.c_void_p(d_ptr), dev_ptr(d_counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return st.as_dict()

    def render_adaptive_region(self, cam, region, *, seed, real_type=A.CR_REAL_F32, tolerance, min_samples, pass_samples, block=16,
                               want_counts=True, want_stats=True, sum_order=None):
        """cr_render_adaptive_region_host: the pixels `region` = (x0, y0, w, h) of the frame `cam` describes to a noise
        target, judged as if the region were the frame (blocks anchored at its origin).  A region whose origin lies on
        multiples of `block` and whose right and bottom edge lie on such multiples or on the frame's edge gives
        render_adaptive()'s pixels and counts bit for bit; region=None passes a null pointer (the library refuses it).
        Returns (image (h, w, 3), counts (h, w) int32 or None, stats dict shaped like render_adaptive's, over the region's
        blocks)."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        reg, (w, h) = region_arg(region)
        out, counts = frame_arrays((max(1, h), max(1, w)), np_real(real_type), want_counts)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_region_host", args, C.byref(ap), reg, host_ptr(out), host_ptr(counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return out, counts, st.as_dict()

    def render_adaptive_region_device(self, cam, region, d_ptr, d_counts=None, *, seed, real_type=A.CR_REAL_F32, tolerance,
                                      min_samples, pass_samples, block=16, want_stats=True, sum_order=None):
        """cr_render_adaptive_region_device: the region into device memory at `d_ptr` (w*h*3 reals) and, if given, its
        counts at `d_counts` (w*h int32).  Synchronous.  Returns the stats dict of render_adaptive_region."""
        ap = adaptive_arg(tolerance, min_samples, pass_samples, block)
        reg, _ = region_arg(region)
        args = self._args(cam, seed, real_type, sum_order=sum_order)
        st = self._call("cr_render_adaptive_region_device", args, C.byref(ap), reg, C.c_void_p(d_ptr), dev_ptr(d_counts),
                        want_stats=want_stats, stats=A.CrAdaptiveStats)
        return st.as_dict()

    def fixed_sums_to_rgb(self, d_sums, d_out, *, width, height, samples, real_type=A.CR_REAL_F32):
        """cr_fixed_sums_to_rgb: summed CR_OUTPUT_FIXED_SUM words of a whole frame (device pointer, W*H*3 uint64) ->
        its per-pixel means at device pointer `d_out` (W*H*3 reals), exactly the relaxed frame.  Asynchronous on the
        handle's stream."""
        self._check(self.lib.cr_fixed_sums_to_rgb(self.h, C.c_void_p(d_sums), width, height, samples, real_type,
                                                  C.c_void_p(d_out)))

    def export_bvh(self, real_type=A.CR_REAL_F32):
        """The wrapper tree the device walks: (boxes (n, 6) f64, children (n, 2) i32, split_axis (n,) i32), see
        cr_export_bvh."""
        return self._export(self.lib.cr_export_bvh, real_type)

    def _export(self, fn, real_type):
        n = C.c_int32()
        self._check(fn(self.h, real_type, None, None, None, 0, C.byref(n)))
        boxes = np.zeros((max(1, n.value), 6), dtype=np.float64)
        kids = np.zeros((max(1, n.value), 2), dtype=np.int32)
        axis = np.full(max(1, n.value), -1, dtype=np.int32)
        self._check(fn(self.h, real_type, boxes.ctypes.data_as(C.c_void_p), kids.ctypes.data_as(C.c_void_p),
                       axis.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return boxes[:n.value], kids[:n.value], axis[:n.value]

    def export_render_bvh(self, real_type=A.CR_REAL_F32):
        """cr_export_render_bvh: the tree the last render or guide pass of `real_type` walked, with the boxes it walked,
        in export_bvh's layout -- the frame tree after a refit_boxes="rebuild" render, the refitted boxes after
        refit_boxes=True."""
        return self._export(self.lib.cr_export_render_bvh, real_type)

    def frame_build_info(self, real_type=A.CR_REAL_F32):
        """cr_frame_build_info: build_info's dict for the last frame-tree build (refit_boxes="rebuild"); n_wrappers is
        0 while there is no frame tree.  Builds nothing."""
        info = A.CrBuildInfo()
        self._check(self.lib.cr_frame_build_info(self.h, real_type, C.byref(info)))
        return info.as_dict()

    def build_info(self, real_type=A.CR_REAL_F32):
        """cr_build_info: which builder made the tree of `real_type` and what it went through, as a dict (bvh_mode,
        built_on_device, n_wrappers, device_rounds, large_nodes, small_subtrees, small_threshold, tree_ms, total_ms).
        Builds the tree if it is not built yet."""
        info = A.CrBuildInfo()
        self._check(self.lib.cr_build_info(self.h, real_type, C.byref(info)))
        return info.as_dict()

    def last_kernel_ms(self):
        ms = C.c_double()
        self._check(self.lib.cr_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def synchronize(self):
        self._check(self.lib.cr_synchronize(self.h))

    def stream(self):
        return self.lib.cr_stream(self.h)

    def write_ppm(self, path, img):
        img = np.ascontiguousarray(img)
        rt = A.CR_REAL_F64 if img.dtype == np.float64 else A.CR_REAL_F32
        rc = self.lib.cr_write_ppm(path.encode(), img.ctypes.data_as(C.c_void_p), rt, img.shape[1], img.shape[0])
        if rc != A.CR_OK:
            raise CrucibleError(rc, "cannot write " + path)

    def write_image(self, path, img):
        """P3 (.ppm, the reference's format), P6 (.pbm6 / .p6.ppm) or PNG by extension; same bytes per channel."""
        img = np.ascontiguousarray(img)
        rt = A.CR_REAL_F64 if img.dtype == np.float64 else A.CR_REAL_F32
        fn = self.lib.cr_write_png if path.endswith(".png") else (self.lib.cr_write_ppm_binary if path.endswith(".p6.ppm") else self.lib.cr_write_ppm)
        rc = fn(path.encode(), img.ctypes.data_as(C.c_void_p), rt, img.shape[1], img.shape[0])
        if rc != A.CR_OK:
            raise CrucibleError(rc, "cannot write " + path)


def out_dtype(output_sum, real_type):
    """A render's output words: reals, or uint64 with output_sum=A.CR_OUTPUT_FIXED_SUM."""
    return np.uint64 if output_sum == A.CR_OUTPUT_FIXED_SUM else np_real(real_type)


def frame_arrays(dims, dtype, want_counts=False):
    """The host output of a render or an adaptive call over `dims` = (H, W), (F, H, W) or a region's (h, w): (colours
    dims + (3,), the int32 count plane(s) `dims` or None)."""
    return np.empty(tuple(dims) + (3,), dtype=dtype), (np.empty(tuple(dims), dtype=np.int32) if want_counts else None)


def guide_buffer(layers, real_type, w, h, n=1):
    """(flat host buffer for the planes of the mask `layers` over n frames of w x h pixels, [(name, channels)] of the planes
    in buffer order)."""
    planes = [(name, c) for name, bit, c in A.AOV_LAYERS if layers & bit]
    return np.empty(max(1, n * w * h * sum(c for _, c in planes)), dtype=np_real(real_type)), planes


def guide_planes(buf, planes, w, h, k=0):
    """Frame k of a guide buffer as a dict of named planes: (h, w, 3) or (h, w) views into `buf`."""
    out, o = {}, k * w * h * sum(c for _, c in planes)
    for name, c in planes:
        out[name] = buf[o:o + w * h * c].reshape((h, w, 3) if c == 3 else (h, w))
        o += w * h * c
    return out


_SUMMED = ("samples", "segments", "node_tests", "prim_tests", "texel_fetches", "nan_pixels", "kernel_ms")


def add_stats(total, st):
    """A tile's stats dict added into the running `total` (None before the first tile): counters, samples, nan_pixels
    and times summed, the rest from the last tile.  An adaptive call's dict carries the render's under "render"."""
    if total is None:
        return dict(st)
    for k in ("judge_ms", "passes", "blocks", "blocks_stopped"):
        if k in st:
            total[k] += st[k]
    into, new = total.get("render", total), st.get("render", st)
    for k in _SUMMED:
        into[k] += new[k]
    for k in ("upload_ms", "bvh_entries", "scene_in_lds"):
        into[k] = new[k]
    return total


def count_plane(counts, shape):
    """A count plane as the contiguous int32 array of `shape` that the guide calls at a count plane read; None stays None
    (a null pointer, which the library refuses)."""
    if counts is None:
        return None
    plane = np.ascontiguousarray(counts, dtype=np.int32)
    if plane.shape != tuple(shape):
        raise ValueError(f"count plane of shape {plane.shape}, expected {tuple(shape)}")
    return plane


def host_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dev_ptr(d):
    return C.c_void_p(d) if d else None


def frame_list(frames):
    """(int32 array, pointer to it) of a batch's frame indices; None stays a null pointer (the library refuses it)."""
    if frames is None:
        return np.zeros(0, dtype=np.int32), None
    fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
    return fr, fr.ctypes.data_as(C.POINTER(C.c_int32))


def view_table(cams):
    """(contiguous CrCameraDesc array of the cameras `cams`, what keeps its key arrays alive); None or an empty list stays a
    null pointer (the library refuses it)."""
    if not cams:
        return None, None
    descs = [c.desc() for c in cams]
    table = (A.CrCameraDesc * len(descs))()
    for k, d in enumerate(descs):
        C.memmove(C.byref(table, k * C.sizeof(A.CrCameraDesc)), C.byref(d), C.sizeof(A.CrCameraDesc))
    return table, descs


def region_arg(region):
    """(pointer to a CrRegion or None, (w, h)) from (x0, y0, w, h); None stays a null pointer (the library refuses it)."""
    if region is None:
        return None, (1, 1)
    x0, y0, w, h = (int(v) for v in region)
    reg = A.CrRegion(x0, y0, w, h)
    return C.pointer(reg), (w, h)


def adaptive_arg(tolerance, min_samples, pass_samples, block=16):
    """A CrAdaptiveParams from the mirrors' arguments: `block` is the block's side in pixels (8, 16, 32; 0 or None: the
    library's default); any other side goes through as a block_log2 the library refuses."""
    block = int(block or 0)
    log2 = {0: 0, 8: 3, 16: 4, 32: 5}.get(block, -1)
    return A.CrAdaptiveParams(int(min_samples), int(pass_samples), log2, 0, float(tolerance))


def aov_mask(layers):
    """A CR_AOV_* mask from a mask or from layer names."""
    if isinstance(layers, (int, np.integer)):
        return int(layers)
    bits = {n: bit for n, bit, _ in A.AOV_LAYERS}
    return sum(bits[n] for n in set(layers))


def write_pfm(path, plane):
    """cr_write_pfm: a (H, W) or (H, W, 3) f32 / f64 array as a portable float map (needs no GPU)."""
    lib = load_library()
    a = np.ascontiguousarray(plane)
    if a.dtype != np.float64:
        a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim not in (2, 3):
        raise ValueError("write_pfm: a plane is (H, W) or (H, W, 3)")
    rt = A.CR_REAL_F64 if a.dtype == np.float64 else A.CR_REAL_F32
    rc = lib.cr_write_pfm(path.encode(), a.ctypes.data_as(C.c_void_p), rt, a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2])
    if rc != A.CR_OK:
        raise CrucibleError(rc, "cannot write " + path)


def quantize_rgb8(img):
    """impl Display for Color (reference src/utils.rs:422-437) over a whole image -> uint8 (H, W, 3)."""
    lib = load_library()
    img = np.ascontiguousarray(img)
    rt = A.CR_REAL_F64 if img.dtype == np.float64 else A.CR_REAL_F32
    out = np.empty(img.shape, dtype=np.uint8)
    rc = lib.cr_quantize_rgb8(img.ctypes.data_as(C.c_void_p), rt, img.size // 3, out.ctypes.data_as(C.c_void_p))
    if rc != A.CR_OK:
        raise CrucibleError(rc, "quantize")
    return out
