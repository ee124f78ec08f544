"""ctypes mirror of include/crucible_hip.h (the C ABI).  Plain data only."""
import ctypes as C

CR_ABI_VERSION = 4

CR_OK, CR_ERR_INVALID_ARG, CR_ERR_NO_DEVICE, CR_ERR_HIP, CR_ERR_NO_SCENE, CR_ERR_IO, CR_ERR_NAN, CR_ERR_UNSUPPORTED, CR_ERR_PEER = range(9)
CR_REAL_F32, CR_REAL_F64 = 0, 1
CR_PRIM_SPHERE, CR_PRIM_TRIANGLE, CR_PRIM_LIST, CR_PRIM_BVH = 0, 1, 2, 3
CR_PRIM_HIDDEN, CR_PRIM_MEMBER, CR_LIST_EMPTY_BOX = 1, 2, 4
CR_MAT_LAMBERTIAN, CR_MAT_METAL, CR_MAT_DIELECTRIC = 0, 1, 2
CR_TEX_SOLID, CR_TEX_CHECKER, CR_TEX_IMAGE = 0, 1, 2
CR_SKY_DEFAULT, CR_SKY_SPHERICAL = 0, 1
CR_BVH_REFERENCE, CR_BVH_SAH, CR_BVH_SAH_ORDERED, CR_BVH_LBVH = 0, 1, 2, 3
CR_BVH_BUILD_DEVICE = 0x100   # OR-ed into bvh_mode: the SAH modes build on the device
CR_KEY_TX, CR_KEY_TY, CR_KEY_TZ, CR_KEY_RADIUS, CR_KEY_SCALE_X, CR_KEY_SCALE_Y, CR_KEY_SCALE_Z = 0, 1, 2, 3, 4, 5, 6
CR_MAX_CHECKER_DEPTH = 32
CR_KEY_NERP, CR_KEY_LERP = 0, 1
CR_SUM_DEFAULT, CR_SUM_REFERENCE_ORDER, CR_SUM_RELAXED = 0, 1, 2
CR_UPDATE_REFIT, CR_UPDATE_REBUILD = 0, 1   # cr_update_primitives flags
CR_REFIT_OFF, CR_REFIT_BOXES, CR_REFIT_REBUILD = 0, 1, 2   # CrRenderParams.refit_boxes


def refit_code(value):
    """CrRenderParams.refit_boxes from what the mirrors accept: False / True / "rebuild" (or one of the codes)."""
    if isinstance(value, str):
        if value != "rebuild":
            raise ValueError(f"refit_boxes: {value!r} is not False, True or 'rebuild'")
        return CR_REFIT_REBUILD
    if value is True or value is False or value is None:
        return CR_REFIT_BOXES if value else CR_REFIT_OFF
    return int(value)
CR_AOV_ALBEDO, CR_AOV_NORMAL, CR_AOV_DEPTH, CR_AOV_COVERAGE = 1, 2, 4, 8   # cr_render_aov_* layers
CR_AOV_ALL = 15
# the planes of a guide-layer buffer in their order (ascending bit): name, bit, channels
AOV_LAYERS = (("albedo", CR_AOV_ALBEDO, 3), ("normal", CR_AOV_NORMAL, 3), ("depth", CR_AOV_DEPTH, 1), ("coverage", CR_AOV_COVERAGE, 1))
CR_OUTPUT_FIXED_SUM = 2   # CrRenderParams.output_sum: 0 mean, 1 sum in reals, 2 fixed-point words (uint64)


class CrPrimitive(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("flags", C.c_int32), ("key_first", C.c_int32),
                ("key_count", C.c_int32), ("_pad", C.c_int32), ("v", C.c_double * 9)]


class CrMaterial(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", C.c_double * 3), ("param", C.c_double)]


class CrTexture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("even", C.c_int32), ("odd", C.c_int32), ("image", C.c_int32),
                ("color", C.c_double * 3), ("inv_scale", C.c_double)]


class CrImage(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb8", C.POINTER(C.c_uint8))]


class CrKeyframe(C.Structure):
    _fields_ = [("channel", C.c_int32), ("interp", C.c_int32), ("t0", C.c_double), ("t1", C.c_double),
                ("a", C.c_double), ("b", C.c_double)]


class CrSceneDesc(C.Structure):
    _fields_ = [("n_prims", C.c_int32), ("n_materials", C.c_int32), ("n_textures", C.c_int32),
                ("n_images", C.c_int32), ("n_keys", C.c_int32), ("sky_kind", C.c_int32), ("sky_image", C.c_int32),
                ("bvh_mode", C.c_int32), ("prims", C.POINTER(CrPrimitive)), ("materials", C.POINTER(CrMaterial)),
                ("textures", C.POINTER(CrTexture)), ("images", C.POINTER(CrImage)), ("keys", C.POINTER(CrKeyframe))]


class CrCameraDesc(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("vfov_degrees", C.c_double),
                ("defocus_angle_degrees", C.c_double), ("focus_dist", C.c_double), ("look_from", C.c_double * 3),
                ("look_at", C.c_double * 3), ("vup", C.c_double * 3), ("from_key_count", C.c_int32),
                ("at_key_count", C.c_int32), ("from_keys", C.POINTER(CrKeyframe)), ("at_keys", C.POINTER(CrKeyframe))]


class CrRenderParams(C.Structure):
    _fields_ = [("samples", C.c_int32), ("sample_begin", C.c_int32), ("sample_count", C.c_int32),
                ("max_depth", C.c_int32), ("seed", C.c_uint64), ("frame", C.c_int32), ("real_type", C.c_int32),
                ("frame_rate", C.c_double), ("shutter_angle", C.c_double), ("output_sum", C.c_int32),
                ("refit_boxes", C.c_int32), ("sum_order", C.c_int32), ("_reserved", C.c_int32)]


class CrStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("node_tests", C.c_uint64),
                ("prim_tests", C.c_uint64), ("texel_fetches", C.c_uint64), ("nan_pixels", C.c_uint64),
                ("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("bvh_entries", C.c_int32),
                ("scene_in_lds", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrRegion(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class CrAdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_int32), ("pass_samples", C.c_int32), ("block_log2", C.c_int32), ("_reserved", C.c_int32),
                ("tolerance", C.c_double)]


class CrAdaptiveStats(C.Structure):
    _fields_ = [("render", CrStats), ("judge_ms", C.c_double), ("passes", C.c_int32), ("blocks", C.c_int32),
                ("blocks_stopped", C.c_int32), ("_pad", C.c_int32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("render", "_pad")}
        d["render"] = self.render.as_dict()
        return d


class CrBuildInfo(C.Structure):
    _fields_ = [("bvh_mode", C.c_int32), ("built_on_device", C.c_int32), ("n_wrappers", C.c_int32),
                ("device_rounds", C.c_int32), ("large_nodes", C.c_int32), ("small_subtrees", C.c_int32),
                ("small_threshold", C.c_int32), ("_pad", C.c_int32), ("tree_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


class CrGroupStats(C.Structure):
    _fields_ = [("render", CrStats), ("reduce_ms", C.c_double), ("members", C.c_int32), ("used_rccl", C.c_int32)]


CR_GROUP_ID_BYTES = 128

# every symbol include/crucible_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "cr_abi_version": (C.c_int32, []),
    "cr_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    "cr_destroy": (None, [C.c_void_p]),
    "cr_upload_scene": (C.c_int32, [C.c_void_p, C.POINTER(CrSceneDesc)]),
    "cr_render_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_void_p,
                                     C.POINTER(CrStats)]),
    "cr_render_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_void_p,
                                   C.POINTER(CrStats)]),
    "cr_render_frames_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                            C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_frames_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                          C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32, C.c_void_p,
                                         C.POINTER(CrStats)]),
    "cr_render_aov_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32, C.c_void_p,
                                       C.POINTER(CrStats)]),
    "cr_render_aov_frames_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_frames_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                              C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_views_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(CrRenderParams),
                                           C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_views_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(CrRenderParams),
                                         C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_views_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(CrRenderParams),
                                               C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_views_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(CrRenderParams),
                                             C.c_int32, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_region_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.POINTER(CrRegion),
                                            C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_region_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.POINTER(CrRegion),
                                          C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_region_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                C.POINTER(CrRegion), C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_region_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                              C.POINTER(CrRegion), C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32, C.c_void_p,
                                                C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32, C.c_void_p,
                                              C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_frames_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                       C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_frames_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                     C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_region_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                       C.POINTER(CrRegion), C.c_void_p, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_aov_counts_region_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_int32,
                                                     C.POINTER(CrRegion), C.c_void_p, C.c_void_p, C.POINTER(CrStats)]),
    "cr_render_adaptive_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                              C.POINTER(CrAdaptiveParams), C.c_void_p, C.c_void_p, C.POINTER(CrAdaptiveStats)]),
    "cr_render_adaptive_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                            C.POINTER(CrAdaptiveParams), C.c_void_p, C.c_void_p, C.POINTER(CrAdaptiveStats)]),
    "cr_render_adaptive_frames_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                                     C.POINTER(CrAdaptiveParams), C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                                     C.c_void_p, C.POINTER(CrAdaptiveStats)]),
    "cr_render_adaptive_frames_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                                   C.POINTER(CrAdaptiveParams), C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                                   C.c_void_p, C.POINTER(CrAdaptiveStats)]),
    "cr_render_adaptive_region_device": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                                     C.POINTER(CrAdaptiveParams), C.POINTER(CrRegion), C.c_void_p, C.c_void_p,
                                                     C.POINTER(CrAdaptiveStats)]),
    "cr_render_adaptive_region_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams),
                                                   C.POINTER(CrAdaptiveParams), C.POINTER(CrRegion), C.c_void_p, C.c_void_p,
                                                   C.POINTER(CrAdaptiveStats)]),
    "cr_export_bvh": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.POINTER(C.c_int32)]),
    "cr_build_info": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(CrBuildInfo)]),
    "cr_export_render_bvh": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(C.c_int32)]),
    "cr_frame_build_info": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(CrBuildInfo)]),
    "cr_update_primitives": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.c_int32]),
    "cr_update_materials": (C.c_int32, [C.c_void_p, C.POINTER(CrMaterial), C.c_int32, C.POINTER(CrTexture), C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]),
    "cr_update_image": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "cr_set_sky": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "cr_last_kernel_ms": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
    "cr_synchronize": (C.c_int32, [C.c_void_p]),
    "cr_stream": (C.c_void_p, [C.c_void_p]),
    "cr_write_ppm": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cr_write_ppm_binary": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cr_write_png": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cr_write_pfm": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "cr_quantize_rgb8": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "cr_fixed_sums_to_rgb": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "cr_last_error": (C.c_char_p, [C.c_void_p]),
    "cr_group_shard": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cr_group_create": (C.c_int32, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]),
    "cr_group_unique_id": (C.c_int32, [C.c_void_p]),
    "cr_group_create_rank": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cr_group_destroy": (None, [C.c_void_p]),
    "cr_group_local_size": (C.c_int32, [C.c_void_p]),
    "cr_group_size": (C.c_int32, [C.c_void_p]),
    "cr_group_rank": (C.c_int32, [C.c_void_p]),
    "cr_group_handle": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "cr_group_upload_scene": (C.c_int32, [C.c_void_p, C.POINTER(CrSceneDesc)]),
    "cr_group_update_primitives": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32,
                                               C.c_int32]),
    "cr_group_update_materials": (C.c_int32, [C.c_void_p, C.POINTER(CrMaterial), C.c_int32, C.POINTER(CrTexture), C.c_int32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]),
    "cr_group_update_image": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "cr_group_set_sky": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "cr_group_render": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_void_p,
                                    C.POINTER(CrGroupStats)]),
    "cr_group_render_host": (C.c_int32, [C.c_void_p, C.POINTER(CrCameraDesc), C.POINTER(CrRenderParams), C.c_void_p,
                                         C.POINTER(CrGroupStats)]),
    "cr_group_last_error": (C.c_char_p, [C.c_void_p]),
}


def bind(lib, symbols=SYMBOLS):
    """Attach restype/argtypes; raises AttributeError if a declared symbol is missing."""
    for name, (res, args) in symbols.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
