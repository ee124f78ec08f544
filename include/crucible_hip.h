/*
 * crucible_hip.h -- C ABI of the MI355X (gfx950) path-tracing integrator that
 * stands in for Crucible's per-pixel render loop.
 *
 * The reference (kylittle/Crucible, Rust) has no FFI.  The seam this ABI
 * replaces is
 *
 *     pub fn Camera::render(&mut self, skybox: &Skybox, world: &Hittables,
 *                           fname: &str) -> Result<(), std::io::Error>
 *                                              (src/camera/mod.rs:270-317)
 *
 * called only from Scene::render_image (src/scene/mod.rs:332-347) right after
 * BVHWrapper::new_wrapper(self.elements.clone()) (src/scene/mod.rs:333).
 * Everything under that call -- cast_ray / ray_color / Hittables::hit /
 * Materials::scatter / Textures::value / the sky lookup -- runs on the GPU
 * behind the entry points below.  Scene building, asset decoding and the PPM
 * text output stay on the host side of the boundary.
 *
 * Rust-callable by construction: #[repr(C)] PODs, caller-owned memory, int32
 * status codes, no unwinding, no global state besides the opaque handle.  The
 * binding a Crucible maintainer would add is shown in INTEGRATION.md.
 *
 * All scene numbers cross the boundary as f64 (the reference's scalar type,
 * src/utils.rs:72-74).  The library computes either in f64 (CR_REAL_F64,
 * arithmetic twin of the reference) or in f32 (CR_REAL_F32, inputs rounded to
 * f32 once at upload).
 */
#ifndef CRUCIBLE_HIP_H
#define CRUCIBLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CR_ABI_VERSION 4

#if defined(__GNUC__)
#define CR_API __attribute__((visibility("default")))
#else
#define CR_API
#endif

/* ---- status codes (the reference panics or returns io::Error instead) ---- */
enum {
    CR_OK = 0,
    CR_ERR_INVALID_ARG = 1,   /* reference: assert!/panic! in constructors          */
    CR_ERR_NO_DEVICE = 2,     /* no HIP device / HIP runtime error at create         */
    CR_ERR_HIP = 3,           /* any other HIP runtime failure (see cr_last_error)   */
    CR_ERR_NO_SCENE = 4,      /* render before upload                                 */
    CR_ERR_IO = 5,            /* file open/write failed (reference: io::Error)        */
    CR_ERR_NAN = 6,           /* a pixel mean is NaN / outside [0,1]
                                 (reference: Color::new assert, src/utils.rs:345-350) */
    CR_ERR_UNSUPPORTED = 7,
    CR_ERR_PEER = 8           /* cr_group_*: another member of the group failed its render (every rank returns this or
                                 its own error, none is left waiting in the collective), or an earlier collective of
                                 this group failed and the group must be destroyed                               */
};

/* ---- scalar type the path computes in ---- */
enum { CR_REAL_F32 = 0, CR_REAL_F64 = 1 };

/* ---- scene elements: Hittables::{Sphere,Triangle,HitList} (src/objects/mod.rs:109-115) ---- */
enum { CR_PRIM_SPHERE = 0, CR_PRIM_TRIANGLE = 1, CR_PRIM_LIST = 2, CR_PRIM_BVH = 3 };
enum {
    CR_PRIM_HIDDEN = 1,      /* Sphere.hide / Triangle.hide (sphere.rs:18, triangle.rs:11)                       */
    CR_PRIM_MEMBER = 2,      /* this sphere/triangle is an object of a CR_PRIM_LIST record, not a scene element  */
    CR_LIST_EMPTY_BOX = 4    /* list built by HitList::new(vec): its box stays Aabb::default() (hitlist.rs:13-18);
                                without the flag the box is what HitList::add accumulates (hitlist.rs:24-27)     */
};

/*
 * One element of the flat scene list (Scene.elements, src/scene/mod.rs:77), in
 * list order -- the order matters because the BVH build stable-sorts it
 * (src/objects/bvhwrapper.rs:66-67).
 *   sphere   : v[0..2] = centre, v[3] = radius          (sphere.rs:26)
 *   triangle : v[0..2] = a, v[3..5] = b, v[6..8] = c    (triangle.rs:24)
 *   list     : a HitList handed to Scene::add_element (scene/mod.rs:164-166): v[0] = index of its first object
 *              in prims, v[1] = number of objects (whole numbers).  The objects are consecutive spheres/triangles
 *              flagged CR_PRIM_MEMBER, in the list's order; each belongs to exactly one list.  The BVH build
 *              treats the list as ONE object (bvhwrapper.rs:18-22 keeps it whatever it holds): a leaf wrapper
 *              that holds it walks every object in order with the shrinking interval and no box test
 *              (HitList::hit, hitlist.rs:51-65); hidden objects return no hit (sphere.rs:62, triangle.rs:87)
 *              but still count towards an add()-built box.  A list inside a list behaves exactly like its
 *              objects spliced in place (the inner box is never read), which is how the host mirrors pass it;
 *   bvh      : a BVHWrapper handed to Scene::add_element (scene/mod.rs:161-163), i.e. the result of
 *              BVHWrapper::new_wrapper(list) (bvhwrapper.rs:15-32): v[0], v[1] name its objects like a list's (spheres
 *              and triangles flagged CR_PRIM_MEMBER; hidden ones are dropped, as new_wrapper drops them).  The library
 *              rebuilds the inner tree with the reference's own algorithm (it is a function of the object list), the
 *              outer build sorts the wrapper by its root box, and BVHWrapper::hit walks into it as into any wrapper.
 *              cr_export_bvh answers CR_ERR_UNSUPPORTED for such a scene in CR_BVH_REFERENCE mode (a wrapper holding
 *              one primitive and one sub-tree has no two-children form in the exported layout).  A wrapper without
 *              a visible object is the empty list new_wrapper returns (bvhwrapper.rs:28-30).  Lists or wrappers
 *              inside a wrapper are not representable (CR_ERR_UNSUPPORTED at the mirrors).
 *              Under the opt-in CR_BVH_SAH / _ORDERED / LBVH trees a list's visible objects are ordinary
 *              primitives of the tree (a bvh record's likewise).  material, key_first, key_count are unused for both.
 * key_first/key_count select this primitive's keyframes in CrSceneDesc.keys
 * (0 keys = static; the initial transform is the v[] values themselves).
 */
typedef struct CrPrimitive {
    int32_t kind;
    int32_t material;
    int32_t flags;
    int32_t key_first;
    int32_t key_count;
    int32_t _pad;
    double v[9];
} CrPrimitive;

/* ---- materials: Materials::{Lambertian,Metal,Dielectric} (src/materials/mod.rs:16-21) ---- */
enum { CR_MAT_LAMBERTIAN = 0, CR_MAT_METAL = 1, CR_MAT_DIELECTRIC = 2 };

typedef struct CrMaterial {
    int32_t kind;
    int32_t texture;     /* Lambertian: index into textures (lambertian.rs:18)          */
    double albedo[3];    /* Metal: albedo (metal.rs:12)                                  */
    double param;        /* Lambertian: scatter_prob; Metal: fuzz; Dielectric: refraction_index */
} CrMaterial;

/* ---- textures: Textures::{SolidColor,CheckerTexture,ImageTexture} (src/textures/mod.rs:12-17) ---- */
enum { CR_TEX_SOLID = 0, CR_TEX_CHECKER = 1, CR_TEX_IMAGE = 2 };
/* Checker textures may nest (checker_texture.rs:12-13 hold arbitrary Arc<Textures>); cr_upload_scene returns
 * CR_ERR_UNSUPPORTED for a chain of more than this many checker levels. */
#define CR_MAX_CHECKER_DEPTH 32

typedef struct CrTexture {
    int32_t kind;
    int32_t even;        /* checker: texture index (checker_texture.rs:12)   */
    int32_t odd;         /* checker: texture index (checker_texture.rs:13)   */
    int32_t image;       /* image: index into images (image_texture.rs:11)   */
    double color[3];     /* solid: albedo (solid_color.rs:7)                 */
    double inv_scale;    /* checker: 1.0/scale, computed by the caller exactly as
                            CheckerTexture::new_* does (checker_texture.rs:23,31) */
} CrTexture;

/* RTWImage after image.to_rgb8() (src/asset_loader/img_loader.rs:27-46):
 * row-major, 3 bytes per texel, texel value = byte / 255.0. */
typedef struct CrImage {
    int32_t width;
    int32_t height;
    const uint8_t* rgb8;
} CrImage;

/* ---- Skybox (src/scene/mod.rs:18-25) ---- */
enum { CR_SKY_DEFAULT = 0, CR_SKY_SPHERICAL = 1 };

/*
 * One flattened keyframe of a TransformTimeline (src/timeline/mod.rs:116-120),
 * i.e. one Transform pushed by translate_{x,y,z} / scale_sphere
 * (src/timeline/transform_builder.rs).  The authoring API stays on the host;
 * only its evaluated form crosses the boundary.
 *   channel 0,1,2 : translate x,y,z.  Active when t >= t0
 *                   (valid_time.is_less(t) || contains(t), timeline/mod.rs:239).
 *                   value = a (NERP) | a * s (LERP), s = clamp((t-t0)/(t1-t0),0,1)
 *                   (timeline/mod.rs:90-96, transform_builder.rs `move |t| x * t`).
 *                   Active values are added in array order (timeline/mod.rs:243-246).
 *   channel 3     : sphere radius (scale_sphere, transform_builder.rs:17-96).  Spheres only.
 *   channel 4,5,6 : ScaleX / ScaleY / ScaleZ of a triangle (scale_x/y/z, scale_point, scale_all_uniform:
 *                   scene_animator.rs:38-229, transform_builder.rs:101-346,729).  Triangles only.
 *                   Channels 3..6 are the timeline's `scale` list: the LAST active key in array order wins and
 *                   replaces the initial scale (timeline/mod.rs:249-255); value v = a (NERP) | a + (b - a) * s
 *                   (LERP: `start + (x - start) * t`).  A vertex (x,y,z) -- after the translate keys -- becomes
 *                   ScaleX: (v*x, y, z); ScaleZ: (x, y, v*z); ScaleY: (x, v*x + y, z) -- the reference writes the
 *                   y factor into row 1, column 0 of the matrix (transform_builder.rs:228-246) and this ABI
 *                   reproduces that.  scale_point pushes X, Y, Z keys with one interval, so its Z key wins.
 *                   Keys must arrive in the timeline's list order (translate list, then scale list, each stably
 *                   sorted by start time as the reference sorts them).
 */
enum { CR_KEY_TX = 0, CR_KEY_TY = 1, CR_KEY_TZ = 2, CR_KEY_RADIUS = 3, CR_KEY_SCALE_X = 4, CR_KEY_SCALE_Y = 5,
       CR_KEY_SCALE_Z = 6 };
enum { CR_KEY_NERP = 0, CR_KEY_LERP = 1 };

typedef struct CrKeyframe {
    int32_t channel;
    int32_t interp;
    double t0, t1;
    double a, b;
} CrKeyframe;

/*
 * Which wrapper tree cr_upload_scene builds over the visible primitives.
 *   CR_BVH_REFERENCE  BVHWrapper::help_generate's median split (src/objects/bvhwrapper.rs:46-78):
 *                     the tree the reference walks, hence the parity mode and the default.
 *   CR_BVH_SAH        SURVEY 8(f) row 1: binned surface-area-heuristic topology.  Same wrapper kind
 *                     (box = union of the primitive boxes, leaves of 1-2 primitives), same walk
 *                     (BVHWrapper::hit, bvhwrapper.rs:96-126: left then right, shrinking interval),
 *                     fewer box tests.  The closest hit equals the reference tree's except where a
 *                     ray grazes a box face (Aabb::hit's `max <= min` miss, bvh.rs:96-132), so
 *                     images are not guaranteed bit-identical to CR_BVH_REFERENCE; cr_export_bvh
 *                     hands a checker the exact tree.
 *   CR_BVH_SAH_ORDERED CR_BVH_SAH's tree walked near child first: at an inner wrapper the child on the ray's
 *                     side of the split (the left one when direction[axis] >= 0) is visited before the other,
 *                     which then sees the interval already shrunk.  Not BVHWrapper::hit's order (always left
 *                     then right); the closest hit again differs from the reference tree's only on box-grazing
 *                     rays.  Stackless on the device (one skip link per direction octant).  Megakernel
 *                     pipeline only.
 *   CR_BVH_LBVH       SURVEY 8(f) row 1, "GPU LBVH": the tree is built on the device (Morton keys of the
 *                     primitive-box centroids, radix sort, Karras' topology; one primitive per leaf) in a few
 *                     milliseconds instead of the host builders' 0.3-0.4 s per million primitives.  Walked in
 *                     BVHWrapper::hit's order like CR_BVH_SAH; a lower-quality tree than SAH.
 *
 * CR_BVH_BUILD_DEVICE is a flag OR-ed into bvh_mode (the low byte keeps the mode):
 *   with CR_BVH_SAH / CR_BVH_SAH_ORDERED  the same tree -- children, split_axis, boxes and primitive order, wrapper for
 *                     wrapper -- built on the device instead of on the host: level-synchronous rounds over the large
 *                     ranges, one wave per small subtree.  Meant for large scenes that are edited or
 *                     animated with CR_UPDATE_REBUILD.  Its build time has NOT been measured against the host
 *                     builder's yet: expect it to lose on small scenes, where the host needs 0.2 ms
 *                     for book1 and a round of kernel launches costs more.  A caller's choice, never switched on by the
 *                     library; never a silent fallback either:
 *                     a device failure is CR_ERR_HIP.  CRUCIBLE_SAH_SMALL=<n> (read at every build) sets the span up to
 *                     which one wave finishes a subtree.
 *   with CR_BVH_LBVH  accepted, changes nothing (that tree is device-built already);
 *   with CR_BVH_REFERENCE  CR_ERR_UNSUPPORTED: the median split's stable sort has no device form.
 * Any other bit is CR_ERR_INVALID_ARG.
 */
enum { CR_BVH_REFERENCE = 0, CR_BVH_SAH = 1, CR_BVH_SAH_ORDERED = 2, CR_BVH_LBVH = 3 };
enum { CR_BVH_BUILD_DEVICE = 0x100 };

typedef struct CrSceneDesc {
    int32_t n_prims;
    int32_t n_materials;
    int32_t n_textures;
    int32_t n_images;
    int32_t n_keys;
    int32_t sky_kind;
    int32_t sky_image;
    int32_t bvh_mode;       /* CR_BVH_REFERENCE (0) | CR_BVH_SAH | CR_BVH_SAH_ORDERED | CR_BVH_LBVH, optionally | CR_BVH_BUILD_DEVICE */
    const CrPrimitive* prims;
    const CrMaterial* materials;
    const CrTexture* textures;
    const CrImage* images;
    const CrKeyframe* keys;
} CrSceneDesc;

/*
 * Camera state read by the render path (src/camera/mod.rs:66-100).  Angles are
 * passed in degrees as the reference's setters take them (set_vfov :213,
 * set_defocus_angle :250); image_height is what Viewport::new derives
 * (camera/mod.rs:37-38) and is passed explicitly so the caller's value wins.
 * look_from / look_at keyframes (cam_translate_point, scene_animator.rs) are
 * flattened like primitive keys; channels 0..2 only.
 */
typedef struct CrCameraDesc {
    int32_t image_width;
    int32_t image_height;
    double vfov_degrees;
    double defocus_angle_degrees;
    double focus_dist;
    double look_from[3];
    double look_at[3];
    double vup[3];
    int32_t from_key_count;
    int32_t at_key_count;
    const CrKeyframe* from_keys;
    const CrKeyframe* at_keys;
} CrCameraDesc;

/*
 * Per-render parameters.  samples/max_depth/frame/frame_rate/shutter_angle are
 * Camera fields (camera/mod.rs:83-99).  The reference draws every random number
 * from an unseeded thread-local generator (rand::rng(), ray_casting.rs:74); this
 * ABI replaces it with one seeded stream per (seed, pixel index, sample index)
 * (SplitMix64-derived key, xorshift64* draws) -- see DESIGN.md "RNG".
 * sample_begin/sample_count select a sub-range of the `samples` sample indices
 * (samples-per-pixel sharding across GPUs); the mean is still taken over
 * `samples` when the sums of all shards are added.
 */
/*
 * How a pixel's samples are summed and a path's attenuations multiplied (CrRenderParams.sum_order).  The paths are
 * the same in every mode -- same draws, same walks, same work counters; only the association of the products and
 * sums differs.
 *   CR_SUM_REFERENCE_ORDER  the reference's own order, bit for bit: `attenuation * ray_color(..)` multiplies
 *                           innermost-first (ray_casting.rs:128) and average_samples adds the samples in draw order
 *                           (:161-165).  The parity mode (every bit-exact test runs in it).  Costs a per-sample colour
 *                           buffer of image_width*image_height*3 reals per sample index (up to 40 GiB, see
 *                           cr_render_device) and a per-path attenuation stack.
 *   CR_SUM_RELAXED          the attenuations are multiplied in path order (a_1*a_2*...*a_n*sky: the same n
 *                           multiplies, associated left to right) and a finished sample is added to its pixel as
 *                           round(colour * 2^52) in a 64-bit integer (2^51, 2^50, ... beyond 2047 samples per pixel).
 *                           Integer adds commute, so the frame is deterministic: two runs give the same sums.  Any
 *                           split into shards adds exactly when the shards export their words at the whole frame's
 *                           scale (output_sum = CR_OUTPUT_FIXED_SUM); as reals (output_sum = 1) each shard uses the
 *                           scale of its own sample count, which differs between shards above 2047 samples per
 *                           pixel, and rounds once.  Per channel the mean differs from the reference order by
 *                           at most about (2 * max_depth + samples) * 2^-53: each of the two product orders rounds
 *                           max_depth times, and the reference's own sequential sum rounds once per sample where the
 *                           integer sum does not -- below 1e-13 at depth 50 and 512 samples, 1.0e-14 measured on the
 *                           headline frame (tested: <= 1e-12 against the oracle, equal counters, equal PPM bytes up to
 *                           values that sit on a byte boundary).  No per-sample buffer and no stack: 24 bytes of device
 *                           memory per pixel.
 *   CR_SUM_DEFAULT          the library's choice: CR_SUM_RELAXED (see DESIGN.md section 3.3 for the measurement);
 *                           the environment variable CRUCIBLE_SUM_ORDER=reference|relaxed overrides it.
 */
enum { CR_SUM_DEFAULT = 0, CR_SUM_REFERENCE_ORDER = 1, CR_SUM_RELAXED = 2 };

/*
 * CrRenderParams.output_sum = CR_OUTPUT_FIXED_SUM: the output buffer receives image_width*image_height*3 uint64_t words
 * (row-major, RGB interleaved, for f32 and f64 alike) holding the shard's CR_SUM_RELAXED sums as they are:
 *   bits 0..62  the magnitude, sum over the shard's samples of round(colour * 2^S)
 *   bit 63      the NaN flag (a sample's colour was not a number)
 * S = min(52, 62 - floor(log2(samples))) is taken from `samples`, the WHOLE frame's count, so the words of all shards of
 * one frame are on one scale.  They combine exactly, in any order, with
 *   c = ((a & M) + (b & M)) | ((a | b) & F),   F = 1 << 63, M = ~F
 * -- the magnitudes of one frame's shards total below samples * 2^S < 2^63, so the add never carries into the flag --
 * and cr_fixed_sums_to_rgb turns the combined words into exactly the frame cr_render_device writes in CR_SUM_RELAXED.
 * Needs CR_SUM_RELAXED (after CR_SUM_DEFAULT / CRUCIBLE_SUM_ORDER are resolved) and the megakernel pipeline; otherwise
 * CR_ERR_UNSUPPORTED.  cr_render_host copies the words back without the Color::new check.
 */
enum { CR_OUTPUT_FIXED_SUM = 2 };   /* CrRenderParams.output_sum: 0 mean, 1 sum in reals, 2 fixed-point words */

typedef struct CrRenderParams {
    int32_t samples;
    int32_t sample_begin;
    int32_t sample_count;
    int32_t max_depth;
    uint64_t seed;
    int32_t frame;
    int32_t real_type;      /* CR_REAL_F32 | CR_REAL_F64 */
    double frame_rate;
    double shutter_angle;
    int32_t output_sum;     /* 0: per-pixel mean over `samples` (average_samples,
                               ray_casting.rs:154-173); 1: raw per-pixel sum of this shard;
                               CR_OUTPUT_FIXED_SUM (2): the shard's exact fixed-point sums, see below.  Other values:
                               CR_ERR_INVALID_ARG. */
    int32_t refit_boxes;    /* 0: wrapper boxes stay the construction-time boxes, as in the reference
                               (bvhwrapper.rs:47-50) -- keyframed primitives are clipped where they leave them;
                               1: SURVEY 8(f) rows 1-2: boxes are re-derived on the device for this frame's
                               ray-time interval before the render (crucible_amd/csrc/refit.hpp), so moving
                               primitives are intersected wherever they are.  No effect without primitive keys;
                               CR_REFIT_REBUILD (2): the tree itself is built for this frame, see below.  Any other
                               value acts as 1. */
    int32_t sum_order;      /* CR_SUM_DEFAULT (0) | CR_SUM_REFERENCE_ORDER | CR_SUM_RELAXED */
    int32_t _reserved;
} CrRenderParams;

/*
 * CrRenderParams.refit_boxes.  CR_REFIT_REBUILD: before the render the binned-SAH tree is
 * built over the visible primitives' boxes for this frame's ray times [current_time, current_time + shutter_length] --
 * the box a refit gives a one-primitive leaf --, with the wrapper boxes refit_boxes = 1 derives for that topology; the
 * render walks that tree.  It needs bvh_mode CR_BVH_SAH or CR_BVH_SAH_ORDERED (with CR_BVH_BUILD_DEVICE the device builder
 * builds it, from boxes computed on the device; without, the host builder): CR_ERR_UNSUPPORTED under CR_BVH_REFERENCE and
 * CR_BVH_LBVH, whatever the scene.  Where refit_boxes = 1 would change nothing (no primitive keys) the call is exactly
 * refit_boxes = 0 and nothing is built.  cr_render_frames_* refuse it as they refuse 1.
 * Not sticky: the frame tree is a second tree on the handle, per real type, beside the tree of the upload; renders with
 * refit_boxes 0 or 1 walk that one as before, and cr_export_bvh / cr_build_info keep describing it.  The frame tree is
 * kept until the next cr_upload_scene, cr_update_primitives or cr_destroy, and a render or guide pass with the same ray
 * times reuses it without building (sample batches, a frame and its guide pass).  The build is deterministic, so every
 * member of a group builds the same tree.
 */
enum { CR_REFIT_OFF = 0, CR_REFIT_BOXES = 1, CR_REFIT_REBUILD = 2 };

/*
 * Work counters of the last render (the algorithmic-bytes model of DESIGN.md):
 * segments = closest-hit queries, node_tests = BVH boxes tested,
 * prim_tests = primitive intersection tests, texel_fetches = image texels read.
 */
typedef struct CrStats {
    uint64_t samples;
    uint64_t segments;
    uint64_t node_tests;
    uint64_t prim_tests;
    uint64_t texel_fetches;
    uint64_t nan_pixels;
    double kernel_ms;       /* HIP-event time of the render kernel(s) on the handle's stream */
    double upload_ms;
    int32_t bvh_entries;
    int32_t scene_in_lds;   /* 0: scene read through L2; 1: whole scene staged in LDS; 2: top levels of the BVH in LDS */
} CrStats;

typedef struct CrHandle CrHandle;

/* ---- entry points ---- */

/* Library ABI version (CR_ABI_VERSION). */
CR_API int32_t cr_abi_version(void);

/* Create a renderer bound to one HIP device.  One handle = one caller thread at
 * a time, like the reference's single-caller Camera (camera/mod.rs:354). */
CR_API int32_t cr_create(int32_t device_id, CrHandle** out);
CR_API void cr_destroy(CrHandle* h);

/* Copies the whole description (the caller may free it on return), filters
 * hidden primitives and builds the BVH selected by scene->bvh_mode -- by default the
 * reference topology (BVHWrapper::new_wrapper, src/objects/bvhwrapper.rs:15-93) -- for
 * each scalar type on first use.  Replaces the `world`/`skybox` arguments of Camera::render. */
CR_API int32_t cr_upload_scene(CrHandle* h, const CrSceneDesc* scene);

/* Camera::render minus the file output: renders into a DEVICE buffer of
 * image_width*image_height*3 reals (f32 or f64 per params->real_type), row-major,
 * RGB interleaved.  Asynchronous on the handle's stream unless `stats` is non-NULL
 * (then it synchronises to fill the stats).
 * Device memory: besides the scene the handle keeps a per-path attenuation stack (3*max_depth reals per
 * resident lane, ~150 MB at depth 50) and a per-sample colour buffer of image_width*image_height*3 reals per
 * sample index, up to 40 GiB (CRUCIBLE_SAMPLE_BUF_MB; a render that needs more runs as consecutive sample
 * batches, CRUCIBLE_SAMPLE_GRANULAR=0 avoids the buffer at a large cost in speed).  The buffers are
 * grown on demand, reused by later renders and freed by cr_destroy.
 * Limits: image_width * image_height <= 2^26; 0 <= sample_begin, sample_begin + sample_count <= samples <= INT32_MAX
 * (the sum is formed in 64 bits); any max_depth >= 0 the attenuation stack has memory for; at most 512 camera
 * keyframes (from + at), more: CR_ERR_UNSUPPORTED.  CRUCIBLE_PIPELINE=queue: the LDS-queue kernel takes renders of
 * image_width <= 65535, image_height <= 65535 and max_depth <= 32767 (what its packed slot words hold); larger ones run on
 * the plain megakernel, as scenes do that leave its slots no LDS.  CRUCIBLE_PIPELINE=wavefront has no limit of its own. */
CR_API int32_t cr_render_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                         void* d_out_rgb, CrStats* stats);

/* Same, into a HOST buffer (render + device->host copy, synchronous). */
CR_API int32_t cr_render_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                       void* h_out_rgb, CrStats* stats);

/*
 * A batch of movie frames in one launch: the frames frames[0..n_frames-1] of one camera and one set of params.
 * frames[k] is the frame index params->frame would carry for frame k (params->frame itself is ignored); any list
 * works -- consecutive, strided (m, m+n, ... for one device of several), descending or repeated.  The output holds
 * n_frames consecutive frames, frame k at k * image_width*image_height*3 elements, each laid out as cr_render_device
 * writes one frame: reals for output_sum 0 and 1, uint64_t words at the whole frame's scale for CR_OUTPUT_FIXED_SUM.
 * sample_begin / sample_count mean what they mean for a single render.
 *
 * Frame k is bit for bit what cr_render_device writes for the same camera and params with frame = frames[k], in f32
 * and in f64: the frames differ only in their ray times (computed on the host as for a single render), the RNG streams
 * are keyed by the frame's own pixel index, and CR_SUM_RELAXED sums are integer sums that do not depend on the order
 * of the work.  `stats` covers the whole call: the counters and `samples` summed over the frames, one kernel_ms.
 *
 * Needs CR_SUM_RELAXED (after CR_SUM_DEFAULT / CRUCIBLE_SUM_ORDER are resolved) and the megakernel pipeline, and no
 * box refit (refit_boxes with keyed primitives or HitList elements: the boxes are per frame, a batch shares one set):
 * otherwise CR_ERR_UNSUPPORTED, and the caller renders those frames one at a time.  A null `frames`, n_frames < 1 or
 * anything cr_render_device rejects: CR_ERR_INVALID_ARG.  The handle keeps fixed-point sums for all frames (24 bytes
 * per pixel per frame); a batch too large for device memory fails with CR_ERR_HIP.  A batch that would overflow the
 * 32-bit work counter runs as several launches of whole frames; a frame that alone needs sample batches runs frame by
 * frame.  Asynchronous unless `stats` is non-NULL, like cr_render_device.
 */
CR_API int32_t cr_render_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                       const int32_t* frames, int32_t n_frames, void* d_out, CrStats* stats);

/* Same, into a HOST buffer of n_frames frames (synchronous).  The Color::new check of cr_render_host applies frame by
 * frame; CR_ERR_NAN's message names the first frame that fails it (stats->nan_pixels counts all frames). */
CR_API int32_t cr_render_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                     const int32_t* frames, int32_t n_frames, void* h_out, CrStats* stats);

/*
 * First-hit guide layers (what a denoiser or a compositor reads beside the beauty frame): per pixel the surface albedo,
 * the shading normal, the depth and the coverage of the PRIMARY rays of cr_render_device for the same camera and
 * params -- the stream rng_key(seed, j*W+i, s) and cast_ray's draws (time, two offsets, defocus disk), keyed cameras
 * included -- and Hittables::hit on [0.001, inf) over the tree that render walks (bvh_mode; refit_boxes as in a render).
 *
 * `layers` is a mask of CR_AOV_*.  The output holds the requested layers as planes, one after the other in ascending
 * bit order: albedo W*H*3 reals, normal W*H*3, depth W*H, coverage W*H; row-major, three-channel planes interleaved,
 * reals of params->real_type; layers that were not requested take no space.
 *
 * Per sample s in [sample_begin, sample_begin + sample_count):
 *   coverage  1 on a hit, 0 on a miss;
 *   albedo    on a hit: Lambertian tex.value(u, v, position) (the scatter's attenuation before the divide by
 *             scatter_prob), Metal its albedo, Dielectric (1, 1, 1); on a miss the sky colour ray_color returns;
 *   normal    e = 0.5 * n + 0.5 per component in `real`, n the HitRecord's normal (turned against the ray as
 *             HitRecord::new does), n = (0, 0, 0) on a miss; decode with 2 e - 1;
 *   depth     |position - origin|, position = origin + t * direction: the difference formed as position + (-origin),
 *             the squares added x, y, z, one square root, all in `real`.
 * Per pixel: albedo, normal and coverage are exact fixed-point sums -- a sample adds rint(x * 2^S), evaluated in f64,
 * to a signed 64-bit word, S that of CR_SUM_RELAXED for params->samples -- turned into the mean over `samples`
 * (output_sum 0) or the shard's sum in reals (output_sum 1) as a relaxed render's sums are; a value that is not finite
 * gives NaN.  Depth is the MINIMUM over the shard's samples that hit, +inf where none did, whatever output_sum says.
 * Integer adds and minima commute: the planes do not depend on scheduling, and the words of shards add up.
 *
 * CR_OUTPUT_FIXED_SUM: CR_ERR_UNSUPPORTED.  layers == 0 or an unknown bit: CR_ERR_INVALID_ARG.  Everything
 * cr_render_device rejects is rejected alike; max_depth and sum_order are validated and otherwise not read.  Works
 * under every CRUCIBLE_PIPELINE setting.  A refused call leaves the handle as it was.
 * stats: samples rendered, segments == samples, node_tests / prim_tests of the walk (those of a max_depth = 1 render),
 * texel_fetches, nan_pixels = 0; kernel_ms, bvh_entries, scene_in_lds as for a render.
 * The handle keeps 64 bytes of accumulators per pixel (+ 4 of flags), grown on demand, freed by cr_destroy.
 * Asynchronous unless `stats` is non-NULL.
 */
enum { CR_AOV_ALBEDO = 1, CR_AOV_NORMAL = 2, CR_AOV_DEPTH = 4, CR_AOV_COVERAGE = 8 };
CR_API int32_t cr_render_aov_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                    void* d_out, CrStats* stats);

/* Same, into a HOST buffer (synchronous).  No Color::new check applies: the planes are not colours of a frame. */
CR_API int32_t cr_render_aov_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                  void* h_out, CrStats* stats);

/*
 * The guide layers of a batch of movie frames in one launch: what cr_render_frames_* is to cr_render_device, for
 * cr_render_aov_device.  frames[k] is the frame index params->frame would carry for frame k (params->frame itself is
 * ignored); any list works -- consecutive, strided, descending or repeated.  The output holds n_frames consecutive
 * frames, frame k at k * R reals, R the reals of the requested planes (3*W*H per three-channel layer, W*H per
 * one-channel layer), each laid out as cr_render_aov_device lays out one frame: planes in ascending bit order, layers
 * that were not requested take no space.
 *
 * Frame k is bit for bit what cr_render_aov_device writes for the same camera, params and `layers` with
 * frame = frames[k]: in f32 and f64, for output_sum 0 and 1, every sample_begin / sample_count, every bvh_mode, every
 * residency of the scene and every CRUCIBLE_PIPELINE and CRUCIBLE_SUM_ORDER setting -- the frames differ only in their
 * ray times (computed on the host as for a single call), the RNG streams are keyed by the frame's own pixel index, and
 * the accumulators are integer sums and minima.  Unlike cr_render_frames_* it does not need CR_SUM_RELAXED: sum_order
 * and max_depth are validated and otherwise not read.  The frames' work is handed out as one launch (one ramp-up and
 * one tail for all of them); a batch with more work units than the 32-bit work counter holds runs as several launches
 * of whole frames.
 *
 * `stats` covers the whole call: `samples` and the counters summed over the frames (segments == samples), one
 * kernel_ms, bvh_entries and scene_in_lds as for one frame.
 *
 * A null `frames` or n_frames < 1: CR_ERR_INVALID_ARG.  layers == 0 or an unknown bit: CR_ERR_INVALID_ARG.  Everything
 * cr_render_aov_device rejects is rejected alike (CR_OUTPUT_FIXED_SUM: CR_ERR_UNSUPPORTED).  A call that would refit
 * or rebuild boxes (refit_boxes with keyed primitives or HitList elements, CR_REFIT_REBUILD where it would build) is
 * CR_ERR_UNSUPPORTED as for cr_render_frames_* -- boxes are per frame, a batch shares one set -- and the caller makes
 * one cr_render_aov_* call per frame; refit_boxes on a scene where a refit changes nothing is accepted.  A refused
 * call leaves the handle as it was.
 * The handle keeps 64 bytes of accumulators and 4 of flags per pixel PER FRAME of the batch, grown on demand, freed
 * by cr_destroy; a batch too large for device memory fails with CR_ERR_HIP.  An empty shard (sample_count == 0)
 * launches no first-hit kernel and writes, for every frame, what the single call writes.
 * Asynchronous unless `stats` is non-NULL.
 */
CR_API int32_t cr_render_aov_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                           const int32_t* frames, int32_t n_frames, void* d_out, CrStats* stats);

/* Same, into a HOST buffer of n_frames frames (synchronous). */
CR_API int32_t cr_render_aov_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                         const int32_t* frames, int32_t n_frames, void* h_out, CrStats* stats);

/*
 * Several cameras of one scene in one launch: the views cams[0..n_views-1] under one set of params -- a stereo pair,
 * the faces of a cube map, a turntable, a movie whose camera zooms, pulls focus, rolls or follows a path sampled on the
 * host.  Where a batch of frames (cr_render_frames_*) may differ only in its ray times, the views of a call may differ
 * in everything a CrCameraDesc holds but the image size: vfov_degrees, defocus_angle_degrees, focus_dist, look_from,
 * look_at, vup and the look_from / look_at keys, whose numbers may differ from view to view too.  frames[k] is the frame
 * index params->frame would carry for view k; frames == NULL: params->frame for every view.  The output holds n_views
 * consecutive views, view k at k * image_width*image_height*3 elements, laid out as cr_render_frames_device lays out
 * frames (reals for output_sum 0 and 1, uint64_t words for CR_OUTPUT_FIXED_SUM).
 *
 * View k is bit for bit what cr_render_device writes for cams[k] and params with frame = frames[k], in f32 and f64, for
 * every output_sum, every sample_begin / sample_count, every bvh_mode and every residency of the scene; a repeated view
 * gives the same bytes twice, and a call of one view the single call's bytes and counters.  `stats` covers the whole
 * call: the counters and `samples` summed over the views, one kernel_ms.
 *
 * CR_ERR_INVALID_ARG: a null `cams`, n_views < 1, a view whose image_width / image_height differ from view 0's, and
 * whatever cr_render_device rejects for any one view (the message names the first such view).  CR_ERR_UNSUPPORTED, as
 * for cr_render_frames_*: a sum order other than CR_SUM_RELAXED (after CR_SUM_DEFAULT / CRUCIBLE_SUM_ORDER are
 * resolved), a pipeline other than the megakernel, a call that would refit or rebuild boxes, and more than 512 camera
 * keyframes over all views together (the views' keys share the one table a single camera's keys have).  Everything is
 * checked before anything changes: a refused call leaves the handle as it was.
 * The handle keeps fixed-point sums for all views (24 bytes per pixel per view) and one camera record per view.  A
 * call that would overflow the 32-bit work counter runs as several launches of whole views; a view that alone needs
 * sample batches runs view by view.  Asynchronous unless `stats` is non-NULL, like cr_render_device.
 */
CR_API int32_t cr_render_views_device(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames,
                                      const CrRenderParams* params, void* d_out, CrStats* stats);

/* Same, into a HOST buffer of n_views views (synchronous).  The Color::new check of cr_render_host applies view by
 * view; CR_ERR_NAN's message names the first view that fails it (stats->nan_pixels counts all views). */
CR_API int32_t cr_render_views_host(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames,
                                    const CrRenderParams* params, void* h_out, CrStats* stats);

/*
 * The guide layers of several cameras in one launch: what cr_render_views_* is to cr_render_device, for
 * cr_render_aov_device.  The output holds n_views consecutive views, view k at k * R reals, each laid out as
 * cr_render_aov_frames_device lays out a frame.  View k is bit for bit what cr_render_aov_device writes for cams[k],
 * params and `layers` with frame = frames[k] (frames == NULL: params->frame).  Like cr_render_aov_frames_* it takes every
 * sum order and pipeline; CR_OUTPUT_FIXED_SUM, a call that would refit or rebuild boxes and more than 512 camera
 * keyframes over all views are CR_ERR_UNSUPPORTED, the arguments' refusals those of cr_render_views_* (and layers == 0
 * or an unknown bit: CR_ERR_INVALID_ARG).  `stats` covers the whole call.  Asynchronous unless `stats` is non-NULL.
 */
CR_API int32_t cr_render_aov_views_device(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames,
                                          const CrRenderParams* params, int32_t layers, void* d_out, CrStats* stats);

/* Same, into a HOST buffer of n_views views (synchronous). */
CR_API int32_t cr_render_aov_views_host(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames,
                                        const CrRenderParams* params, int32_t layers, void* h_out, CrStats* stats);

/*
 * A region of a frame: the pixels [x0, x0 + width) x [y0, y0 + height) of the frame that `cam` describes.
 * cam->image_width / image_height stay the WHOLE frame's: they define the viewport, the pixel deltas and the RNG's
 * pixel index (y0 + j) * image_width + (x0 + i).  The output holds the region only: width*height*3 reals, row-major
 * (uint64_t words at the whole frame's scale under CR_OUTPUT_FIXED_SUM, so shards of a region add up exactly and
 * cr_fixed_sums_to_rgb with the region's width and height finalises them).
 *
 * Output pixel (i, j) is bit for bit pixel (x0 + i, y0 + j) of what cr_render_device writes for the same cam and
 * params: in f32 and f64, for every output_sum, every sample_begin / sample_count, every bvh_mode, every residency of
 * the scene and refit_boxes 0, 1 and CR_REFIT_REBUILD (a region call renders one frame, so boxes may be refitted).
 * The RNG streams are keyed by the frame's pixel index, the camera vectors are those of the whole frame and relaxed
 * sums are integer sums.  A region that is the whole frame gives cr_render_device's bytes and counters.
 * stats: samples = width * height * sample_count; segments, node_tests, prim_tests and texel_fetches count the
 * region's samples only, so the counters of regions that partition a frame add up to the frame's.
 *
 * Limits: width * height <= 2^26; the frame itself may have up to 2^31 - 1 pixels here (the RNG key's pixel index has
 * 32 bits) -- a frame beyond cr_render_device's limit is rendered region by region.  Regions split a frame by pixels
 * across handles (devices, processes, nodes) as sample_begin / sample_count split it by samples.
 *
 * CR_ERR_INVALID_ARG: a null `region`, width < 1, height < 1, a negative origin, x0 + width > image_width or
 * y0 + height > image_height (sums formed in 64 bits), more than 2^26 pixels in the region, and whatever
 * cr_render_device rejects.  CR_ERR_UNSUPPORTED: a sum order other than CR_SUM_RELAXED (after CR_SUM_DEFAULT /
 * CRUCIBLE_SUM_ORDER are resolved) or a pipeline other than the megakernel, as for cr_render_frames_*.  Everything is
 * checked before anything changes: a refused call leaves the handle as it was.  An empty shard (sample_count == 0)
 * zero-fills a buffer of the region's size.  Asynchronous unless `stats` is non-NULL, like cr_render_device;
 * cr_export_render_bvh, cr_last_kernel_ms and cr_frame_build_info behave as after a whole-frame call.
 */
typedef struct CrRegion { int32_t x0, y0, width, height; } CrRegion;   /* pixels of the frame cam describes */
CR_API int32_t cr_render_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, const CrRegion* region,
                                       void* d_out, CrStats* stats);

/* Same, into a HOST buffer of the region's size (synchronous); the Color::new check of cr_render_host applies to the
 * region's pixels. */
CR_API int32_t cr_render_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, const CrRegion* region,
                                     void* h_out, CrStats* stats);

/*
 * The guide layers of a region: what cr_render_region_* is to cr_render_device, for cr_render_aov_device.  The output
 * holds the requested planes at the region's size (albedo width*height*3 reals, normal width*height*3, depth
 * width*height, coverage width*height) in cr_render_aov_device's order, and value (i, j) of a plane is bit for bit
 * value (x0 + i, y0 + j) of the whole frame's plane.  Works under every sum order and pipeline, as cr_render_aov_*
 * do.  Refusals: those of cr_render_aov_device (layers; CR_OUTPUT_FIXED_SUM) and the region ones above.  An empty
 * shard writes what the single guide call writes.  stats as for cr_render_aov_device, over the region's samples.
 */
CR_API int32_t cr_render_aov_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                           const CrRegion* region, void* d_out, CrStats* stats);

/* Same, into a HOST buffer (synchronous). */
CR_API int32_t cr_render_aov_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                         const CrRegion* region, void* h_out, CrStats* stats);

/*
 * Guide layers at a count plane: the guide pass in which every pixel takes its own number of primary rays -- fed the
 * `counts` of a cr_render_adaptive_* call, the albedo, normal, depth and coverage of exactly the primary rays that
 * adaptive frame's beauty pixels used.  Each entry point is its cr_render_aov_* sibling with one more argument, `counts`
 * (const int32_t*; device memory for the device forms, host memory for the host forms), in front of the output pointer.
 * The plane is laid out as the adaptive sibling writes it: image_width*image_height values for a frame, width*height
 * for a region, n_frames * image_width*image_height for a batch with frame k at k * image_width*image_height.
 *
 * Definition.  n_p = min(max(counts[p], 0), params->samples).  Pixel p takes the sample indices [0, n_p) of the stream
 * rng_key(seed, frame pixel, s); everything else is cr_render_aov_device's definition.  The words are scaled by 2^S with
 * S that of params->samples (the maximum), as everywhere.  Albedo, normal and coverage are (sum * 2^-S) / n_p with
 * output_sum 0, in the arithmetic that finalizes every guide plane, and sum * 2^-S with output_sum 1.  A pixel with
 * n_p == 0 writes +0.0 in those planes (nothing is divided by zero) and +inf depth.  Depth is the minimum over the
 * samples taken.
 *
 * Consequences.  With params->samples <= 2047 (S = 52) every value of a pixel p with n_p >= 1 is BIT FOR BIT that of
 * the sibling cr_render_aov_* call with params->samples = n_p: in f32 and f64, for every layer mask, bvh_mode, residency
 * and CRUCIBLE_PIPELINE / CRUCIBLE_SUM_ORDER setting, and for refit_boxes as the sibling handles it.  A plane that is
 * params->samples everywhere gives the sibling call's bytes and integer stats.
 * stats: samples == segments == the sum of n_p over the call's pixels, taken from the kernel's own counter (the host
 * does not read a device plane); node_tests, prim_tests and texel_fetches are the walk's own -- over a partition into
 * rectangles on which the plane is constant they add up to those of the sibling region calls at those sample counts;
 * kernel_ms, bvh_entries and scene_in_lds as for the sibling.
 *
 * Refusals, all checked before anything changes (a refused call leaves the handle as it was): the sibling's own, in its
 * order and with its codes (a frames call that would refit or rebuild boxes is CR_ERR_UNSUPPORTED); after those a null
 * `counts` is CR_ERR_INVALID_ARG; after that sample_begin != 0 or sample_count != samples is CR_ERR_UNSUPPORTED -- the
 * plane counts from sample 0, as the adaptive calls do.  The values of the plane are never refused: they are clamped.
 * The launch is sized from params->samples, so an all-zero plane still launches a kernel, which finds nothing to do.
 * The device forms are asynchronous unless `stats` is non-NULL and read `counts` in stream order; the host forms are
 * synchronous and copy the plane into a buffer the handle keeps (4 bytes per pixel per frame, grown on demand, freed by
 * cr_destroy).  No Color::new check applies.  cr_export_render_bvh, cr_last_kernel_ms and cr_frame_build_info behave as
 * after the sibling guide call.
 */
CR_API int32_t cr_render_aov_counts_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                           const int32_t* d_counts, void* d_out, CrStats* stats);
CR_API int32_t cr_render_aov_counts_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                         const int32_t* h_counts, void* h_out, CrStats* stats);
CR_API int32_t cr_render_aov_counts_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                                  const int32_t* frames, int32_t n_frames, const int32_t* d_counts, void* d_out,
                                                  CrStats* stats);
CR_API int32_t cr_render_aov_counts_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                                const int32_t* frames, int32_t n_frames, const int32_t* h_counts, void* h_out,
                                                CrStats* stats);
CR_API int32_t cr_render_aov_counts_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                                  const CrRegion* region, const int32_t* d_counts, void* d_out, CrStats* stats);
CR_API int32_t cr_render_aov_counts_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params, int32_t layers,
                                                const CrRegion* region, const int32_t* h_counts, void* h_out, CrStats* stats);

/*
 * A frame to a noise target: blocks of pixels stop taking samples once their two half-frame means agree.
 * params->samples is the MAXIMUM per pixel.  The output is image_width*image_height*3 reals, each pixel's mean over the
 * samples that pixel took; `counts` (may be NULL) receives image_width*image_height int32_t, the samples each pixel took.
 *
 * The rule, in exact integer arithmetic.  Let P = pass_samples and S = the exponent of the fixed-point scale 2^S of
 * params->samples (as CR_OUTPUT_FIXED_SUM defines it: the largest S <= 52 with samples * 2^S < 2^63; 52 up to 2047 samples).
 *   - Pass p = 0, 1, ... renders the sample indices [pP, (p+1)P) of every pixel of every still-active block.
 *   - Even passes add into accumulator E, odd passes into accumulator O: two sets of relaxed sums, 24 bytes per pixel
 *     each, bit 63 of a word the NaN flag.
 *   - After each pair of passes (q = 1, 2, ...: n = 2qP samples taken) every active block b with n >= min_samples is judged:
 *       d(x, c) = |mag(E[x,c]) - mag(O[x,c])| >> 12, mag = bits 0..62 of the word;
 *       D_b = the sum of d over the block's pixels inside the frame and the three channels, an exact 64-bit integer
 *             (fewer than 2^12 terms, each below 2^51);
 *       T_b = (uint64) min(floor(tolerance * (2^(S-12) * qP * 3 N_b)), 2^63), N_b = the block's pixels inside the frame;
 *             the bracket is exact in f64, then there is one f64 multiply and one floor;
 *       the block stops iff D_b <= T_b, else it stays active.
 *     In words: a block stops when the mean absolute difference between its two half-frame means is at most
 *     `tolerance` (linear colour).
 *   - A block that stops at n is final.  Blocks still active at n = params->samples end there (they are not judged there).
 *   - The blocks are 2^block_log2 pixels square and anchored at pixel (0, 0); edge blocks are partial.
 *   - The output is ((mag(E) + mag(O)) * 2^-S) / n_b in the arithmetic that finalizes every relaxed frame, n_b the
 *     block's sample count; NaN where either word's flag is set.
 * Consequences: the frame and the counts are deterministic and independent of scheduling (integer sums; the order of the
 * active-tile list never reaches the output).  With params->samples <= 2047 (S = 52) every pixel is BIT FOR BIT the pixel
 * of cr_render_device with samples = counts[pixel] under CR_SUM_RELAXED (beyond that a shorter render uses a finer scale).
 * min_samples == params->samples is exactly the plain relaxed render, counters included.
 *
 * CR_ERR_INVALID_ARG: a null `adaptive`; block_log2 outside {0, 3, 4, 5}; _reserved != 0; pass_samples < 1;
 * params->samples or min_samples not a positive multiple of 2 * pass_samples; min_samples > params->samples; a negative
 * or non-finite tolerance; a null output; and whatever cr_render_device rejects.  CR_ERR_UNSUPPORTED: a sum order other
 * than CR_SUM_RELAXED (after CR_SUM_DEFAULT / CRUCIBLE_SUM_ORDER are resolved) or a pipeline other than the megakernel,
 * as for cr_render_region_*; sample_begin != 0 or sample_count != samples (the judgement needs all samples of a pixel);
 * output_sum != 0.  Everything is checked before anything changes: a refused call leaves the handle as it was.
 * refit_boxes 0, 1 and CR_REFIT_REBUILD work: the boxes or the tree are prepared once and the passes reuse them.
 *
 * The call is synchronous: the host reads the number of active tiles back (4 bytes) after every judged pair of passes.
 * The handle keeps 48 bytes per pixel for E and O, apart from the other calls' buffers, freed by cr_destroy.
 * Afterwards cr_export_render_bvh behaves as after a render.  cr_last_kernel_ms reports only the passes since the last
 * judgement (the handle's event pair is recorded anew for every such run); the call's whole render time is
 * stats->render.kernel_ms, the sum over all passes.
 */
typedef struct CrAdaptiveParams {
    int32_t min_samples;    /* no block is judged before it has this many samples per pixel            */
    int32_t pass_samples;   /* P: samples per pixel per launch                                          */
    int32_t block_log2;     /* 3, 4 or 5: blocks of 8, 16 or 32 pixels square; 0 = the default, 4       */
    int32_t _reserved;      /* 0 */
    double  tolerance;      /* >= 0, finite: see the rule above                                         */
} CrAdaptiveParams;

typedef struct CrAdaptiveStats {
    CrStats render;         /* counters and samples summed over all passes, kernel_ms their sum         */
    double  judge_ms;       /* HIP-event time of the judge and finalize kernels                         */
    int32_t passes;         /* launches of the render kernel                                            */
    int32_t blocks;         /* blocks of the frame                                                      */
    int32_t blocks_stopped; /* blocks that stopped before params->samples                               */
    int32_t _pad;
} CrAdaptiveStats;

CR_API int32_t cr_render_adaptive_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                         const CrAdaptiveParams* adaptive, void* d_out_rgb, int32_t* d_counts, CrAdaptiveStats* stats);

/* Same, into HOST buffers; the Color::new check of cr_render_host applies (stats->render.nan_pixels, CR_ERR_NAN). */
CR_API int32_t cr_render_adaptive_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                       const CrAdaptiveParams* adaptive, void* h_out_rgb, int32_t* h_counts, CrAdaptiveStats* stats);

/*
 * A batch of movie frames to a noise target, under one pass loop: what cr_render_frames_device is to cr_render_device,
 * for cr_render_adaptive_device.
 *
 * Frames.  frames[k] is the frame index params->frame would carry; params->frame itself is ignored.  Any list works:
 * consecutive, strided, descending, repeated (a repeated frame has its own accumulators and gives the same bytes twice).
 * Output.  n_frames consecutive frames, frame k at k * image_width*image_height*3 reals.  `counts` may be NULL, else it
 * receives n_frames * image_width*image_height int32_t, frame k at k * image_width*image_height.
 * Bit-exactness.  Frame k and its counts are BIT FOR BIT what cr_render_adaptive_device writes for the same camera,
 * params and adaptive params with frame = frames[k]: in f32 and f64, for every bvh_mode and residency, at any
 * params->samples (the single call uses the same scale 2^S, so this includes S < 52).  The stopping rule is per block
 * and in exact integers, so a frame does not depend on the frames it shares its launches with.
 *
 * The pass loop.  One loop serves the whole batch: pass p renders the samples [pP, (p+1)P) of the active tiles of all
 * frames in one launch (even passes into E, odd into O), a judged pair judges every active block of every frame in one
 * judge launch, and one 4-byte read-back gives the batch's active-tile count.  The loop ends when no tile of any frame is
 * active, or at params->samples; a frame whose blocks have all stopped simply has no tile in the list any more.
 *
 * stats, over the whole call: render's counters and samples are summed over the frames, kernel_ms over all passes;
 * passes is the number of launches of the render kernel; blocks and blocks_stopped are summed over the frames;
 * bvh_entries and scene_in_lds are as for one frame.
 *
 * Memory.  The handle keeps 48 bytes per pixel per frame (E of all frames, then O of all frames), two tile lists of the
 * batch's tile count and one word per block per frame; all of it grows on demand, and a batch too large for device
 * memory is CR_ERR_HIP.
 * Work counter.  One pass over all tiles of the batch must fit the launch's 32-bit work counter.  A batch that does not
 * fit runs as consecutive sub-batches of whole frames, each its own pass loop writing its slice of the output (the
 * memory above is then a sub-batch's): the frames' bytes are unchanged by the split, and passes adds up over the
 * sub-batches.  A frame that alone does not fit is refused exactly as cr_render_adaptive_device refuses it.
 *
 * Refusals, all checked before anything changes (a refused call leaves the handle as it was).  CR_ERR_INVALID_ARG:
 * everything cr_render_adaptive_device refuses, with the same codes, plus a null `frames` or n_frames < 1.
 * CR_ERR_UNSUPPORTED: what cr_render_adaptive_device answers so, and a call that would refit or rebuild boxes --
 * refit_boxes with keyed primitives or HitList elements, or CR_REFIT_REBUILD where it would build: boxes are per
 * frame and a batch shares one set, the rule of cr_render_frames_device (render such frames one at a time).  refit_boxes
 * on a scene where it changes nothing is accepted.  Synchronous, like cr_render_adaptive_device.
 */
CR_API int32_t cr_render_adaptive_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                                const CrAdaptiveParams* adaptive, const int32_t* frames, int32_t n_frames,
                                                void* d_out_rgb, int32_t* d_counts, CrAdaptiveStats* stats);

/* Same, into HOST buffers.  The Color::new check of cr_render_host runs frame by frame: stats->render.nan_pixels counts
 * all frames, and CR_ERR_NAN's message names the first failing frame, as cr_render_frames_host's does. */
CR_API int32_t cr_render_adaptive_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                              const CrAdaptiveParams* adaptive, const int32_t* frames, int32_t n_frames,
                                              void* h_out_rgb, int32_t* h_counts, CrAdaptiveStats* stats);

/*
 * A region of a frame to a noise target: what cr_render_region_device is to cr_render_device, for
 * cr_render_adaptive_device.  An editor re-renders what an edit touched at the frame's own noise level, a frame beyond
 * 2^26 pixels is rendered adaptively region by region, and a farm splits an adaptive frame by pixels across handles.
 *
 * Region and camera.  cam->image_width and image_height stay the whole frame's, and the RNG streams are keyed by the
 * frame's pixel index (y0 + j) * image_width + (x0 + i), as for cr_render_region_*.  The output is width*height*3 reals,
 * row-major; `counts` (may be NULL) receives width*height int32_t.
 * The rule is cr_render_adaptive_device's, unchanged, applied to the region as if it were the frame: the blocks of
 * 2^block_log2 pixels are anchored at the region's origin (x0, y0), blocks at the region's right and bottom edge are
 * partial, N_b counts the block's pixels inside the region, S is that of params->samples.
 *
 * Consequences.
 *   1. With params->samples <= 2047 every pixel is BIT FOR BIT the pixel of cr_render_region_device with
 *      samples = counts[pixel] under CR_SUM_RELAXED, hence the pixel of the whole frame's plain render at that count.
 *   2. Where x0 and y0 are multiples of the block's side and the region's right and bottom edge each fall on such a
 *      multiple or on the frame's edge, the region's blocks are the frame's blocks: image and counts are BIT FOR BIT the
 *      corresponding pixels of cr_render_adaptive_device for the same arguments, and a frame tiled by such regions is
 *      the whole-frame adaptive frame, pixel for pixel and count for count.  Any other region is still deterministic,
 *      but its blocks are not the frame's, so its counts may differ from the frame's.
 *   3. A region that is the whole frame gives cr_render_adaptive_device's bytes, counts and stats.
 *   4. stats->render's four work counters and samples are those of the region's blocks; blocks and blocks_stopped count
 *      the region's blocks.  Over a partition that satisfies (2), samples, the counters, blocks and blocks_stopped add
 *      up to the whole-frame call's; passes does not: the whole-frame call's is the maximum over the partition.
 *   5. min_samples == params->samples is exactly cr_render_region_*, counters included.
 *
 * Refusals, all checked before anything changes (a refused call leaves the handle as it was): everything
 * cr_render_adaptive_device refuses, with the same codes, and everything cr_render_region_device refuses about the
 * region, with the same codes (a null `region`, sizes below 1, a negative origin, overhang with the sums formed in 64
 * bits, more than 2^26 pixels in the region).  The frame itself may have up to 2^31 - 1 pixels, as for regions.
 * CR_ERR_UNSUPPORTED also for a work tile named through CRUCIBLE_SG_TILE that is wider or taller than the block (the
 * whole-frame call renders such a block on the default tile).  A pass over the region's tiles that the 32-bit work
 * counter does not hold runs as consecutive launches of fewer samples, with the same bytes and counters, and counts once
 * in stats->passes.  refit_boxes 0, 1 and CR_REFIT_REBUILD work: the boxes or the tree are prepared once per call.
 *
 * Synchronous.  The handle keeps 48 bytes per pixel of the region.  cr_export_render_bvh, cr_last_kernel_ms and
 * cr_frame_build_info behave as after cr_render_adaptive_device.
 */
CR_API int32_t cr_render_adaptive_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                                const CrAdaptiveParams* adaptive, const CrRegion* region,
                                                void* d_out_rgb, int32_t* d_counts, CrAdaptiveStats* stats);

/* Same, into HOST buffers of the region's size; the Color::new check of cr_render_host applies to the region's pixels
 * (stats->render.nan_pixels, CR_ERR_NAN). */
CR_API int32_t cr_render_adaptive_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* params,
                                              const CrAdaptiveParams* adaptive, const CrRegion* region,
                                              void* h_out_rgb, int32_t* h_counts, CrAdaptiveStats* stats);

/* The wrapper tree the device walks for `real_type`, as BVHWrapper's shape (src/objects/bvhwrapper.rs:7-11):
 * wrapper k has boxes[6k..6k+5] = xmin,xmax,ymin,ymax,zmin,zmax (exact values of `real_type`) and
 * children[2k], children[2k+1] = left, right: >= 0 another wrapper's index, < 0 the bitwise complement of a
 * primitive's index in CrSceneDesc.prims.  Wrappers are numbered in walk order (root 0, left subtree, right
 * subtree); a one-primitive wrapper names that primitive twice (bvhwrapper.rs:58-60).  split_axis (may be NULL)
 * receives, per wrapper, the axis whose direction sign picks the child visited first in CR_BVH_SAH_ORDERED mode
 * (right child first when direction[axis] < 0), or -1 where the order is always left then right.  *n_wrappers
 * receives the count; boxes/children may be NULL to query it.  Builds the tree if the scene was not rendered yet. */
CR_API int32_t cr_export_bvh(CrHandle* h, int32_t real_type, double* boxes, int32_t* children, int32_t* split_axis,
                             int32_t capacity, int32_t* n_wrappers);

/*
 * What the build of the uploaded scene's tree did, for one real type: which builder ran and the phases it went through
 * (the laps CRUCIBLE_BUILD_TIMING prints).  Builds the tree if it is not built yet, as cr_export_bvh does.
 * CR_ERR_INVALID_ARG for a null handle, a null `out` or an unknown real_type; CR_ERR_NO_SCENE before an upload.
 */
typedef struct CrBuildInfo {
    int32_t bvh_mode;          /* base mode (without CR_BVH_BUILD_DEVICE) */
    int32_t built_on_device;   /* 1: CR_BVH_LBVH, or a SAH mode with CR_BVH_BUILD_DEVICE over at least 3 primitives (fewer are one leaf,
                                  which the host writes: 0, with small_threshold 0) */
    int32_t n_wrappers;
    int32_t device_rounds;     /* device SAH build: level-synchronous rounds run */
    int32_t large_nodes;       /* ... nodes split in those rounds */
    int32_t small_subtrees;    /* ... subtrees finished by one wave each */
    int32_t small_threshold;   /* ... the span limit in effect (0 when that builder did not run) */
    int32_t _pad;
    double tree_ms;            /* the tree phase alone: topology and primitive order (the device builders fill the
                                  wrapper boxes after the upload: that is in total_ms) */
    double total_ms;           /* the whole build, uploads included */
} CrBuildInfo;
CR_API int32_t cr_build_info(CrHandle* h, int32_t real_type, CrBuildInfo* out);

/*
 * The tree that the last render or guide pass of `real_type` on this handle walked, with the boxes it walked, in
 * cr_export_bvh's layout: after refit_boxes = CR_REFIT_REBUILD the frame tree, after refit_boxes = 1 the uploaded scene's
 * topology with that frame's boxes, after refit_boxes = 0 what cr_export_bvh returns.  CR_ERR_NO_SCENE before any render
 * of that real type since the last cr_upload_scene or cr_update_primitives.  May synchronise the handle's stream.
 */
CR_API int32_t cr_export_render_bvh(CrHandle* h, int32_t real_type, double* boxes, int32_t* children, int32_t* split_axis,
                                    int32_t capacity, int32_t* n_wrappers);

/*
 * What the last frame-tree build (CR_REFIT_REBUILD) of `real_type` did: builder, rounds, tree_ms (boxes of the frame,
 * topology and order), total_ms (the whole build).  All zero -- n_wrappers = 0 -- while no frame tree exists.  Builds nothing.
 * CR_ERR_INVALID_ARG for a null handle, a null `out` or an unknown real_type; CR_ERR_NO_SCENE before an upload.
 */
CR_API int32_t cr_frame_build_info(CrHandle* h, int32_t real_type, CrBuildInfo* out);

/*
 * Edit primitives of the uploaded scene in place: new coordinates for n spheres / triangles, without another
 * cr_upload_scene.  prim_index[k] is an index into the CrSceneDesc.prims of the last upload (NULL: 0..n-1) and
 * v + 9k its new CrPrimitive.v: a sphere reads v[0..3] (what it stores beyond them is kept), a triangle all nine.
 * Kind, material, flags, key range and list membership cannot be changed; for a keyed primitive the new values are the
 * initial transform its keys apply to.  The caller's arrays are free on return.  The call is ordered on the handle's
 * stream after earlier renders (an asynchronous render launched before it sees the scene as it was) and may synchronise.
 *
 *   CR_UPDATE_REFIT    every precision already built on the handle: the device record of each named visible primitive
 *                      becomes what an upload of the edited description packs, bit for bit (1/radius included), and
 *                      every wrapper box becomes what a fresh build computes for the SAME topology -- a leaf the union
 *                      of its primitives' construction-time boxes, an inner wrapper the tight_enclose of its children
 *                      (src/objects/bvh.rs:67-73) -- on the device, bottom-up; the screening records follow.  Links, LDS
 *                      sizing and kernel selection do not change; cr_export_bvh returns the same children and
 *                      split_axis with the new boxes.  The tree is as good as the edit is small: primitives that
 *                      travel far leave large, overlapping boxes (correct, slower to walk).  A precision not built yet
 *                      builds at first use from the edited description; a hidden primitive changes in the host copy
 *                      only.  refit_boxes and the stale-box default behave as after an upload of the edited description.
 *   CR_UPDATE_REBUILD  the same edit, after which the trees are rebuilt by the scene's bvh_mode builder (on the device under CR_BVH_BUILD_DEVICE) at next use: the
 *                      handle is then what a cr_upload_scene of the edited description leaves, without re-uploading
 *                      images, materials, textures and keys.
 *
 * Everything is checked before anything changes -- after an error the next render is what it would have been:
 * CR_ERR_INVALID_ARG for a null handle, n < 0, null v with n > 0, unknown flags, an index out of range, repeated within
 * the call or naming a CR_PRIM_LIST / CR_PRIM_BVH record, a non-finite coordinate or a negative radius (cr_upload_scene's
 * messages); CR_ERR_NO_SCENE before an upload; CR_ERR_UNSUPPORTED for a scene that holds a CR_PRIM_LIST or CR_PRIM_BVH
 * element (their construction-time boxes are not the union of their objects' boxes, so a refit does not reproduce them).
 * n == 0 is CR_OK and does nothing.
 */
enum { CR_UPDATE_REFIT = 0, CR_UPDATE_REBUILD = 1 };
CR_API int32_t cr_update_primitives(CrHandle* h, const int32_t* prim_index, const double* v,
                                    int32_t n, int32_t flags);

/*
 * Edit what the uploaded scene's surfaces look like, in place and without another cr_upload_scene: the material and
 * texture tables and the primitives' material indices (cr_update_materials), the texels of a rectangle of an image
 * (cr_update_image), the sky (cr_set_sky).  The tree is a function of the geometry alone and is NOT rebuilt: topology,
 * boxes, screening records and leaf order are what they were, and cr_build_info keeps reporting the build that made them.
 *
 * Equivalence: after a successful call the handle behaves as a handle that received cr_upload_scene of the EDITED
 * description does -- the host copy with the new tables, the new CrPrimitive.material indices, the new texels, the new
 * sky -- for every later call: every cr_render_* family and shape, cr_export_bvh, cr_export_render_bvh, cr_build_info,
 * cr_update_primitives; in f32 and f64, under every sum_order, bvh_mode and refit_boxes value.  Output bytes, the integer
 * CrStats counters, bvh_entries and scene_in_lds are equal bit for bit.
 *
 * cr_update_materials
 *   materials / textures   NULL (with a count of 0): the table stays.  Else the WHOLE new table: it may grow or shrink.
 *                      The device tables are repacked as an upload packs them -- live textures re-indexed densely, a
 *                      solid top-level texture folded into its material -- so they are the bytes a fresh upload makes,
 *                      and the LDS sizing of the next launch is what a fresh upload would choose.
 *   prim_index / prim_material   n_assign pairs: CrPrimitive.material of prims[prim_index[k]] becomes prim_material[k].  A
 *                      visible primitive's device record changes in every precision already built; a hidden primitive
 *                      changes in the host copy only; a precision not built yet builds from the edited host copy at
 *                      first use.  In a scene with CR_PRIM_LIST / CR_PRIM_BVH elements the objects of lists may be
 *                      reassigned too: the trees are then rebuilt at next use from the edited host copy, as
 *                      CR_UPDATE_REBUILD does (the side tables stay) -- the same result, at the cost of a build.
 *   Validation is that of the resulting description, before anything changes, with cr_upload_scene's messages and codes:
 *   the texture rules (kind, checker children with smaller indices, image index, solid colours in [0,1], nesting depth:
 *   CR_ERR_UNSUPPORTED beyond CR_MAX_CHECKER_DEPTH), the material rules (kind, a Lambertian's texture index below the new
 *   n_textures, metal fuzz and albedo, a finite param), and after the edit every sphere's and triangle's material below
 *   the new n_materials ("primitive material index out of range": also a table that shrinks under a primitive that is
 *   not reassigned).  A new table is checked against the other table as kept.
 *   The call's own refusals, prefixed "cr_update_materials:": CR_ERR_INVALID_ARG for a null handle, a negative count, a
 *   null table with a count that is not zero, n_assign > 0 with a null prim_index or prim_material, an index out of range,
 *   named twice, or naming a CR_PRIM_LIST / CR_PRIM_BVH record; CR_ERR_NO_SCENE before an upload.  A call that names
 *   nothing (both tables NULL, n_assign == 0) is CR_OK and does nothing.
 *   Frame trees (CR_REFIT_REBUILD): a call that only replaces tables keeps them -- a later render with the same ray times
 *   builds nothing and cr_frame_build_info is unchanged; a call with n_assign > 0 drops them, as cr_update_primitives does.
 *
 * cr_update_image   new texels for the rectangle (x0, y0, width, height) of image `image` of the last upload: rgb8 holds
 *   width*height*3 bytes, row-major, RGB8.  The image's dimensions cannot change.  CR_ERR_INVALID_ARG for a null handle, a
 *   null rgb8, a width or height below 1, an image outside [0, n_images), a rectangle that does not lie inside the image
 *   as uploaded (the sums are formed in 64 bits); CR_ERR_NO_SCENE before an upload.  Keeps the frame trees.
 *
 * cr_set_sky   CrSceneDesc.sky_kind / sky_image of the uploaded scene, under cr_upload_scene's checks and messages
 *   ("unknown sky kind"; "sky image index out of range" for CR_SKY_SPHERICAL).  Keeps the frame trees.
 *
 * Ordering, as for cr_update_primitives: each call is ordered on the handle's stream after earlier launches (an
 * asynchronous render launched before it sees the scene as it was) and may synchronise; the caller's arrays are free on
 * return.  A refused call leaves the handle as it was.
 */
CR_API int32_t cr_update_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials,
                                   const CrTexture* textures, int32_t n_textures,
                                   const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign);
CR_API int32_t cr_update_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height,
                               const uint8_t* rgb8);
CR_API int32_t cr_set_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image);

/* Wait for the last render launched on this handle and return its kernel time in
 * milliseconds, measured with HIP events recorded on the handle's stream around the
 * launch (no counters are copied back). */
CR_API int32_t cr_last_kernel_ms(CrHandle* h, double* out_ms);

/* Block until the handle's stream is idle. */
CR_API int32_t cr_synchronize(CrHandle* h);

/* The hipStream_t the handle launches on (so a caller can order its own work). */
CR_API void* cr_stream(CrHandle* h);

/* PPM P3 writer reproducing Camera::render's output (camera/mod.rs:286,306-311) and
 * `impl Display for Color` (src/utils.rs:422-437): (255*sqrt(c)) as u32.  `rgb` is
 * image_width*image_height*3 host reals of `real_type` holding per-pixel means. */
CR_API int32_t cr_write_ppm(const char* path, const void* rgb, int32_t real_type,
                     int32_t image_width, int32_t image_height);

/* SURVEY 8(f) row 3 -- faster frame output than the reference's ASCII P3, same bytes per channel as
 * `impl Display for Color`: binary PPM (P6) and 8-bit RGB PNG (what BASELINE.json's north_star names). */
CR_API int32_t cr_write_ppm_binary(const char* path, const void* rgb, int32_t real_type,
                                   int32_t image_width, int32_t image_height);
CR_API int32_t cr_write_png(const char* path, const void* rgb, int32_t real_type,
                            int32_t image_width, int32_t image_height);

/* Portable float map, the file a guide layer travels in: the header "Pf" (channels 1) or "PF" (channels 3), a line with
 * width and height, the line "-1.0" (little-endian), then width*height*channels little-endian f32, rows BOTTOM to top.
 * `data` is a host plane of `real_type`, row-major top to bottom; f64 is rounded to f32, +-inf passes through.  Needs
 * no GPU.  Another `channels`: CR_ERR_INVALID_ARG; a file that cannot be written: CR_ERR_IO. */
CR_API int32_t cr_write_pfm(const char* path, const void* data, int32_t real_type,
                            int32_t width, int32_t height, int32_t channels /* 1 | 3 */);

/* Quantise means to the bytes Display would print (3 per pixel); no file. */
CR_API int32_t cr_quantize_rgb8(const void* rgb, int32_t real_type, int64_t n_pixels, uint8_t* out);

/* The per-pixel means of a whole frame of `samples` samples per pixel from its summed CR_OUTPUT_FIXED_SUM words (device
 * buffer of width*height*3 uint64_t): sums * 2^-S / samples, NaN where the flag is set, into d_out_rgb (width*height*3
 * reals of real_type), exactly what cr_render_device writes in CR_SUM_RELAXED.  For callers that move the words with a
 * transport of their own (one process per GPU, a Rust host).  Asynchronous on the handle's stream. */
CR_API int32_t cr_fixed_sums_to_rgb(CrHandle* h, const uint64_t* d_sums, int32_t width, int32_t height, int32_t samples,
                                    int32_t real_type, void* d_out_rgb);

/* Last error text of this handle (NULL handle: last create error). */
CR_API const char* cr_last_error(CrHandle* h);

/*
 * ---- several GPUs of one node: samples-per-pixel sharding + one RCCL reduce ----
 *
 * Every sample is an independent path (src/camera/ray_casting.rs:82-105) and the random stream is keyed by
 * (seed, pixel, sample), so member g of G renders sample indices cr_group_shard(samples, g, G) of EVERY pixel as raw
 * per-pixel sums (the scene is replicated), one reduce over xGMI adds them on member 0, and the root turns them into
 * the mean.  The union is the 1-GPU sample set.
 *   CR_SUM_RELAXED          the members export CR_OUTPUT_FIXED_SUM words; ncclReduce(sum, uint64) adds the magnitudes
 *                           and ncclReduce(max, uint8) the NaN flags (a byte plane), in one ncclGroupStart/End; the root
 *                           finalizes them as cr_fixed_sums_to_rgb does.  The frame is the 1-GPU frame BIT FOR BIT, for
 *                           any member count.
 *   CR_SUM_REFERENCE_ORDER  ncclReduce(sum, f32 | f64 per real_type) of the shards' real sums, then the divide by
 *                           `samples` (average_samples' `/= count`, ray_casting.rs:168-170): the image differs from the
 *                           1-GPU one only by the order of the floating-point adds.
 * A group of one member without a collective is bit-identical to cr_render_device in both orders.  This replaces the reference's worker pool
 * (src/camera/cpu_threading.rs:25-115: `thread_count` OS threads behind one mutex) across devices.
 *
 * Two ways to form a group; both end in the same cr_group_render:
 *   cr_group_create       one process drives n devices (one handle + stream per device, ncclCommInitAll) -- what a
 *                         Rust host calling this library would use;
 *   cr_group_create_rank  one process per GPU (torch.distributed.run style): rank 0 obtains cr_group_unique_id and
 *                         ships its 128 bytes to every rank by any means (ncclCommInitRank).
 * RCCL (librccl.so.1) is loaded on first use; a group of ONE member never needs it.  Movies shard whole frames
 * instead (frame f -> member f % G, src/scene/mod.rs:307-316): no collective, drive cr_group_handle(g) directly.
 */
typedef struct CrGroup CrGroup;
#define CR_GROUP_ID_BYTES 128

/* [begin, begin+count) of member `member` among `n_members`: begin = member*samples/n_members (integer division).
 * The ranges partition [0, samples); with more members than samples some are empty (they contribute zeros).
 * Pure arithmetic: callable without a GPU. */
CR_API int32_t cr_group_shard(int32_t samples, int32_t member, int32_t n_members, int32_t* begin, int32_t* count);

CR_API int32_t cr_group_create(const int32_t* device_ids, int32_t n_devices, CrGroup** out);
CR_API int32_t cr_group_unique_id(uint8_t id[CR_GROUP_ID_BYTES]);
CR_API int32_t cr_group_create_rank(int32_t device_id, int32_t rank, int32_t world_size,
                                    const uint8_t id[CR_GROUP_ID_BYTES], CrGroup** out);
CR_API void cr_group_destroy(CrGroup* g);

/* Members driven by THIS process (n_devices, or 1 in rank mode) / in the whole group / this process's first member. */
CR_API int32_t cr_group_local_size(CrGroup* g);
CR_API int32_t cr_group_size(CrGroup* g);
CR_API int32_t cr_group_rank(CrGroup* g);
CR_API CrHandle* cr_group_handle(CrGroup* g, int32_t local_member);

/* cr_upload_scene on every local member (the scene is replicated). */
CR_API int32_t cr_group_upload_scene(CrGroup* g, const CrSceneDesc* scene);

/* cr_update_primitives on every local member.  Every member is validated before any is changed; the first member's
 * error wins.  In rank mode every rank calls it with the same arguments (no collective is involved). */
CR_API int32_t cr_group_update_primitives(CrGroup* g, const int32_t* prim_index, const double* v,
                                          int32_t n, int32_t flags);

/* cr_update_materials, cr_update_image and cr_set_sky on every local member, under cr_group_update_primitives' rule:
 * every member is validated before any is changed, the first member's error wins, and in rank mode every rank calls with
 * the same arguments (no collective is involved). */
CR_API int32_t cr_group_update_materials(CrGroup* g, const CrMaterial* materials, int32_t n_materials,
                                         const CrTexture* textures, int32_t n_textures,
                                         const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign);
CR_API int32_t cr_group_update_image(CrGroup* g, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height,
                                     const uint8_t* rgb8);
CR_API int32_t cr_group_set_sky(CrGroup* g, int32_t sky_kind, int32_t sky_image);

/* Camera::render across the group.  params->sample_begin/sample_count/output_sum are ignored (output_sum must still be
 * a valid value): the group splits
 * [0, samples) itself and returns the per-pixel MEAN.  d_out_rgb: device buffer of W*H*3 reals on the ROOT member's
 * device (member 0 = device_ids[0], or rank 0); other ranks may pass NULL.  Every rank of a rank-mode group must
 * call this with the same arguments (it is a collective).  Synchronous.  stats (may be NULL): counters summed over
 * the LOCAL members, kernel_ms = the slowest local member's render, reduce_ms in CrGroupStats.
 * Failure: arguments are validated and buffers allocated on every member before anything is launched; with a
 * collective, the members then agree (a 12-byte ncclAllReduce(min) on the render streams) that every render is fine
 * and that every rank reduces the same kind of sums (its resolved sum_order; otherwise CR_ERR_INVALID_ARG) before the
 * ncclReduce is entered -- if one is not, EVERY rank returns an error (its own, or CR_ERR_PEER) and the
 * group stays usable.  If a collective call itself fails, the group's communicators are aborted and every later call
 * on it returns CR_ERR_PEER: destroy the group.  The calling thread's current HIP device is restored on return. */
typedef struct CrGroupStats {
    CrStats render;        /* local members: counters summed, kernel_ms = max */
    double reduce_ms;      /* root-side time of the reduce + the finalize, HIP events on the root's stream */
    int32_t members;       /* whole group */
    int32_t used_rccl;     /* 0: a one-member group rendered directly */
} CrGroupStats;
CR_API int32_t cr_group_render(CrGroup* g, const CrCameraDesc* cam, const CrRenderParams* params, void* d_out_rgb,
                               CrGroupStats* stats);
/* Same, into a HOST buffer on the root (cr_render_host's counterpart: render + reduce + device->host copy, and the
 * Color::new check of every mean -> CR_ERR_NAN).  Ranks other than the root may pass NULL. */
CR_API int32_t cr_group_render_host(CrGroup* g, const CrCameraDesc* cam, const CrRenderParams* params, void* h_out_rgb,
                                    CrGroupStats* stats);
CR_API const char* cr_group_last_error(CrGroup* g);

#ifdef __cplusplus
}
#endif
#endif /* CRUCIBLE_HIP_H */
