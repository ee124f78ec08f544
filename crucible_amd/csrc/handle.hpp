// handle.hpp -- what the translation units of libcrucible_hip.so share: the handle behind the C ABI of
// include/crucible_hip.h, a precision's device copy of the scene, and the internal functions one unit calls in another.
// Those are hidden-visibility functions of cr:: (exports.map keeps the dynamic table to the ABI); each is defined in
// the unit its declaration names.  A kernel instantiation is emitted by exactly one unit:
//   build.hip          build_dev_scene as stages over the host tree code of tree.hpp (a header free of the HIP runtime: the builders,
//                      the splice, the leaf layout, the export walk), the LBVH driver (lbvh.hpp, hipcub), cr_export_bvh, cr_build_info;
//                      the per-frame tree of CR_REFIT_REBUILD (build_frame_scene), cr_export_render_bvh, cr_frame_build_info
//   sah_device.hip     the device-side SAH builder of CR_BVH_BUILD_DEVICE (sah_device.hpp, hipcub)
//   scene.hip          cr_upload_scene (its descriptor checks: scene_checks.hpp, a header free of the HIP runtime), refit.hpp's box kernels,
//                      the screening records, cr_update_primitives, cr_update_materials, cr_update_image, cr_set_sky (update.hpp)
//   render.hip         render_typed: a render's kernel arguments up to the choice of ladder; the stats epilogue
//   render_*.hip       the megakernels of one precision and one sum order (render.hpp: the residency ladder over residency.hpp's rule, and
//                      one launch<real, RELAX> per unit, which takes its kernel as a MegaKernel descriptor)
//   aov.hip            the guide pass cr_render_aov_* (aov.hpp): its host side and the finalize kernel
//   aov_f32.hip, aov_f64.hip   the guide pass's first-hit kernels of one precision (aov_kernel.hpp; one aov_launch<real> per unit)
//   render_views_f32.hip, render_views_f64.hip   the megakernels of several cameras in one launch, cr_render_views_* (render_views.hpp: their ladder
//                      over pathtrace_kernel_views; launched by render.hpp's launch<real, true>)
//   aov_views_f32.hip, aov_views_f64.hip   the first-hit kernels of several cameras in one launch, cr_render_aov_views_* (aov_kernel.hpp's VIEWS axis)
//   aov_counts_f32.hip, aov_counts_f64.hip   the first-hit kernels at a count plane, cr_render_aov_counts_* (aov_kernel.hpp's COUNTS axis; aov_counts.hpp: its integer rules)
//   alt_pipelines.hip  the wavefront and LDS-queue cross-check pipelines (wavefront.hpp, queue.hpp)
//   adaptive.hip       the adaptive family behind its entry points: its argument checks, the pass loop, the judge and finalize kernels (adaptive.hpp)
//   api.hip            cr_create / cr_destroy, all cr_render_* entry points over one RenderCall, errors;  files.hip: PPM / PNG writers;  group.hip: cr_group_*
// What the host side holds on the device is owned by the types of devres.hpp (device memory, events, pinned memory, the stream):
// deleting a handle gives everything back, and no unit frees or destroys by hand.
// The path tracer's code lies in layered headers.  This header reads the bottom layer alone -- records.hpp: the
// records, KernelArgs, MaxBlock and LatencyBlock, over hd.hpp's CR_HD / CR_D -- and launch_plan.hpp, so api, group, scene, build,
// sah_device, adaptive, aov and render parse no kernel code of it.  The units that emit its kernels (render_*, render_views_*,
// aov_*, aov_views_*, aov_counts_*, alt_pipelines) read pathtrace.hpp -- intersect.hpp, shade.hpp, walk.hpp, megakernel.hpp --
// through render.hpp, aov_kernel.hpp, wavefront.hpp and queue.hpp.
#pragma once
#include "../../include/crucible_hip.h"
#include "records.hpp"       // the records and KernelArgs; no kernel code of the path tracer: the units that launch it include pathtrace.hpp
#include "launch_plan.hpp"   // fx_scale_for, and what launch() and aov_launch() ask about their launches
#include "devres.hpp"        // DevBuf, DevEvent, PinnedBuf, DevStream, CamSlot: what owns the device resources (and <hip/hip_runtime.h>)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace cr {

// Sibling wrappers are adjacent in the level-order array and start at ODD indices (1,2), (3,4), ...  Skipping one
// entry at the front of the allocation puts every pair on one 2*sizeof(Entry) boundary: the two children of a
// wrapper then share a cache line (f64: exactly one 128-byte line), so the walk's left-then-right visits touch it once.
template <typename E> constexpr size_t entry_pad() { return (sizeof(E) & (sizeof(E) - 1)) == 0 ? sizeof(E) : 0; }

enum { kWalkNone = 0, kWalkBase = 1, kWalkRefit = 2, kWalkFrame = 3 };

template <typename real> struct DevScene {
    bool built = false;
    DevBuf entries, prims, mats, texs, keys;
    DevBuf leaf_runs;                        // (first, count) of the primitive runs that leaves holding a list name
    int32_t n_entries = 0, n_prims = 0, n_mats = 0, n_texs = 0, n_scene_keys = 0;
    size_t lds_bytes = 0;
    bool animated = false;
    bool has_triangles = false;
    bool has_spheres = false;
    bool has_leaf_runs = false;              // some leaf names its primitives through leaf_runs (a HitList element)
    bool has_bvh_elements = false;           // CR_BVH_REFERENCE over a BVHWrapper element: the records are not the reference's wrappers one to one (no export)
    bool has_lists = false;                  // the tree was built over at least one HitList element: its construction-time box
                                             // (empty, or grown over hidden objects too) is not what refit derives
    DevBuf entries_refit;                    // working copy whose boxes refit_level_kernel rewrites per frame
    DevBuf screen, screen_refit;             // f64, unordered trees: the f32 screening records of entries / entries_refit
    DevBuf screen_overflow;                  // f64: one int, set by the record kernels when a box plane lies beyond the f32 range
    bool screen_usable = true;               // f64: `screen` may be walked on (no box plane beyond the f32 range)
    bool nan_planes = false;                 // a construction-time box has a plane that is not a number (f32: inf - inf): every ray walks with Aabb::hit's own form
    bool ordered = false;                    // CR_BVH_SAH_ORDERED: `entries` holds EntryO records
    size_t entry_bytes = sizeof(Entry<real>);
    std::vector<int8_t> host_axis;           // ordered: split axis per wrapper (-1 leaf), same order as host_entries
    std::vector<int32_t> level_begin;        // entries of tree level l are [level_begin[l], level_begin[l+1])
    std::vector<Entry<real>> host_entries;   // the tree over the scene's objects (for cr_export_bvh); the device copy names primitive runs
    std::vector<int32_t> leaf_desc;          // leaf-order position -> index in the caller's primitive list
    DevBuf desc_pos;                         // the inverse, on the device: index in the caller's primitive list -> position of its record in
                                             // `prims`, -1 where it has none (hidden); scenes without list elements only (cr_update_primitives)
    bool desc_pos_valid = false;
    CrBuildInfo info = {};                   // what the last build of this precision did (cr_build_info)
    bool side_tables = false;                // mats / texs / keys hold the uploaded scene's, as cr_update_materials last repacked mats / texs (a rebuild
                                             // after cr_update_primitives or cr_update_materials keeps them)
    // CR_REFIT_REBUILD (build.hip build_frame_scene).  On the base tree of a SAH mode: what a frame build starts from.
    std::vector<int32_t> in_desc;            // builder input position -> index in the caller's primitive list (the order the SAH builders see)
    std::vector<int32_t> base_order;         // leaf-order position -> builder input position (leaf_desc[i] = in_desc[base_order[i]])
    int32_t last_walk = kWalkNone;           // which tree the last render or guide pass of this precision walked (cr_export_render_bvh)
    // On the frame tree (CrHandle::f32 / f64): the ray-time interval it was built for; mats / texs / keys alias the base tree's
    bool frame_valid = false;
    real frame_ta = real(0), frame_tb = real(0);
    DevBuf frame_map;                        // a frame build's index tables on the device (input positions, then gather sources)
};

}   // namespace cr

using cr::DevBuf;
using cr::DevEvent;
using cr::PinnedBuf;
using cr::DevStream;
using cr::CamSlot;
using cr::DevScene;

// The device-side SAH build's working set (sah_device.hip).  Grow-only and kept on the handle, so that a rebuild of the
// same scene allocates nothing; an upload without CR_BVH_BUILD_DEVICE releases it.
struct SahDeviceWork {
    DevBuf box, order[2], seg[2], pbins, flags, scan, tmp, slots[2], nodes, small, ctr;
    void release() { *this = SahDeviceWork(); }
};

struct CrHandle {
    int device = 0;
    DevStream stream;                 // declared before every other resource: destroyed after all of them
    DevEvent ev0, ev1;
    int n_cus = 0;
    std::string error;
    // host copy of the scene description
    bool has_scene = false;
    std::vector<CrPrimitive> prims;
    std::vector<CrMaterial> materials;
    std::vector<CrTexture> textures;
    std::vector<CrKeyframe> keys;
    int32_t sky_kind = 0, sky_image = -1, bvh_mode = 0;   // bvh_mode: the base mode, CrSceneDesc.bvh_mode's low byte
    bool bvh_device = false;          // CR_BVH_BUILD_DEVICE: the SAH modes build on the device (sah_device.hpp)
    bool has_list_elements = false;   // some CR_PRIM_LIST / CR_PRIM_BVH record: cr_update_primitives does not apply
    DevBuf update_stage;              // cr_update_primitives: the call's rows (9 doubles each), then its indices; cr_update_materials: its
                                      // indices, then its materials; cr_update_image: its RGB8 bytes
    SahDeviceWork sah_work;           // build_sah_device's buffers, kept from build to build: CR_UPDATE_REBUILD sits in an edit loop
    // images are precision independent
    DevBuf images, texels;
    int32_t n_images = 0;
    std::vector<int32_t> image_w, image_h;  // the images' sizes and texel offsets as uploaded (cr_update_image)
    std::vector<uint32_t> image_offset;
    size_t n_texels = 0;                    // words in `texels`
    DevScene<float> s32;
    DevScene<double> s64;
    DevScene<float> f32;              // CR_REFIT_REBUILD: the frame tree of each precision, beside the base tree
    DevScene<double> f64;
    DevBuf work_counter, counters, att_stack, out_buf;
    // Camera keyframes of a render travel in a ring of per-launch slots: a pinned host slot is filled, copied to its
    // device slot on the handle's stream and kept until that copy's event has fired, so back-to-back asynchronous
    // renders (a movie's frames) never see each other's keys.
    static constexpr int kCamSlots = 4;
    static constexpr size_t kMaxCamKeys = 512;
    CamSlot cam[kCamSlots];
    int cam_next = 0, cam_pending_slot = -1;
    DevBuf sample_buf, sg_acc;   // sample-granular megakernel: per-sample colours of a batch, running sums between batches
    DevBuf aov_acc, aov_flags;   // cr_render_aov_*: per pixel 8 x u64 (albedo, normal, coverage sums; depth) and the channels' NaN bits
    DevBuf aov_counts;           // cr_render_aov_counts_*_host: the caller's count plane on the device (4 bytes per pixel per frame), grow-only
    DevBuf fx_acc;               // CR_SUM_RELAXED: per-pixel fixed-point sums (3 x u64 per pixel; per frame of a batch)
    // cr_render_adaptive_* (adaptive.hip): the two half-frame accumulators E and O (relaxed sums, apart from fx_acc), the two
    // tile lists, each block's final sample count, the judge's cursor, the count plane of the host form; the judge's events.
    // cr_render_adaptive_frames_*: of all frames of a pass loop -- E of every frame, then O of every frame
    DevBuf ad_acc, ad_lists, ad_block_n, ad_ctrl, ad_counts;
    DevEvent ad_ev0, ad_ev1;
    // cr_render_frames_*: a batch's per-frame ray times travel through one pinned host buffer, refilled only after the
    // previous batch's copy has run (times_ev); the device table is reused in stream order.  cr_render_views_*: the views'
    // camera records (CamConst, one per view) follow the times in the same table, at the next multiple of 16 bytes
    PinnedBuf times_host;
    DevBuf times_dev;
    DevEvent times_ev;
    int screen_boxes = 1;        // f64, unordered trees: box tests decided on f32 screening records where f32 can (CRUCIBLE_SCREEN=0: never)
    int screen_lds = 1;          // ... also for scenes that sit in LDS whole (CRUCIBLE_SCREEN_LDS=0: only trees read from global memory)
    int default_sum_order = CR_SUM_RELAXED;   // what CR_SUM_DEFAULT means on this handle (CRUCIBLE_SUM_ORDER=reference|relaxed)
    // wavefront pipeline state (wavefront.hpp)
    DevBuf wf_job, wf_rng, wf_ray, wf_depth, wf_hit_t, wf_hit_prim, wf_chunk, wf_ctrl, wf_samples, wf_acc;
    PinnedBuf wf_ring_host;             // host-mapped ring the extend kernel reports its queue length into (16 words)
    uint32_t* wf_ring_dev = nullptr;    // its device address: borrowed, owns nothing
    DevEvent wf_ev[8];
    int pipeline = 0;                   // 0 = megakernel (default), 1 = wavefront kernels, 2 = LDS-queue megakernel (CRUCIBLE_PIPELINE=mega|wavefront|queue)
    int queue_walk_waves = 9, queue_min_batch = 48, queue_patience = 64;
    uint32_t wf_slots = 1u << 21;
    size_t wf_sample_bytes = (size_t)1600 << 20;
    int wf_last_iterations = 0;
    double upload_ms = 0;
    size_t lds_limit = 160 * 1024;
    // Sample-granular scheduling of the megakernel (pathtrace.hpp, KernelArgs::sg_on): on by default; the per-sample
    // colour buffer may take up to sample_buf_limit bytes (more samples than fit are rendered in batches).
    int sample_granular = 1;             // CRUCIBLE_SAMPLE_GRANULAR=0: a lane owns a pixel (no buffer)
    size_t sample_buf_limit = (size_t)40 << 30;   // CRUCIBLE_SAMPLE_BUF_MB (MI355X: 288 GB of HBM)
    int sg_chunk_override = 0;           // CRUCIBLE_SG_CHUNK: items per atomic (default: by launch size)
    uint64_t work_counter_max = 0xF0000000ull;   // work items one launch may hand out (32-bit counter); more samples run as consecutive launches
                                         // (CRUCIBLE_WORK_COUNTER_MAX: tests shrink it to reach that path on small frames)
    int sg_lw = -1, sg_lh = -1;          // CRUCIBLE_SG_TILE=WxH (powers of two, W*H <= 64); default 4x4 pixels x 4 samples
    // f32 trees with more than latency_entries wrappers run on pathtrace_kernel_latency (6 waves/SIMD) with a
    // latency_top_bytes LDS window, three 512-thread groups per CU.  CRUCIBLE_LATENCY_ENTRIES (0 = never).
    int32_t latency_entries = 0;         // (round 3: never by default -- with relaxed sums, the early touch of the leaf's second primitive and the deferred
                                         //  leaf phases the regular kernel is 6.7 % faster on the 1M-sphere tree: 1770 against 1658 Msamples/s)
    size_t latency_top_bytes = 48 * 1024;
    size_t lds_side_limit = 16 * 1024;   // RES_TOP: materials + textures join the LDS window up to this size (CRUCIBLE_LDS_SIDE_KB; 0 = never)
    size_t lds_top_bytes = 128 * 1024;  // LDS spent on the top of a tree that does not fit whole (CRUCIBLE_LDS_TOP_KB; 0 = none): 4096 32-byte records
                                        // (f32 wrappers, or the f64 kernels' screening records) -- one 1024-thread workgroup per CU has the LDS to itself; teapot +2.5 %
    int blocks_per_cu_override = 0;
    int block_override = 0;
    // Wave scheduling of the walk (speed only).  -1 = chosen per scene: sphere scenes 10 / 56, scenes with triangles 8 / 40 --
    // a triangle test is ~1.5x a sphere test, so parked lanes are dearer and the sweeps (gpurun_out/exp7.txt, exp8.txt:
    // teapot +9 % in f64 and f32 at 8 / 40; book1 and the 1M-sphere scene lose 1-2 % there) favour shorter rounds and
    // an earlier exit.  CRUCIBLE_WALK_ROUND / CRUCIBLE_WALK_EXIT override.
    int walk_round_steps = -1;         // wrappers a lane may step through per round; 0 = until every walking lane found a leaf or ran out
    int walk_exit_lanes = -1;          // leave the walk phase once this many lanes are not walking (64 = wait for all)
    int walk_leaf_min = -1;            // CRUCIBLE_WALK_LEAF_MIN: parked lanes a leaf phase waits for while others can still step (0 = every round; default 8:
                                       // book1 +1.5 %, movie frame +1.5 %, 1M spheres +2.9 %, profiles/experiments/r03_leaf_min.txt)
    int last_block = 0, last_grid = 0;
    bool check_abort = false;          // the last launch was a queue kernel whose abort word has not been read yet
    bool keep_counters = false;        // a render without a CrStats still counts: its counters are read later (a group's member, group.hip)
    // The handle's work drains on its device before the members give their resources back (in reverse order of declaration)
    ~CrHandle() { (void)hipSetDevice(device); if (stream) (void)hipStreamSynchronize(stream); }
};

namespace cr {

#define HIP_TRY(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            (h)->error = std::string(#expr) + ": " + hipGetErrorString(_e);                   \
            return CR_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

int32_t fail(CrHandle* h, int32_t code, const std::string& msg);   // api.hip (h == nullptr: cr_create's error)

template <typename real> DevScene<real>& dev_scene(CrHandle* h);
template <> inline DevScene<float>& dev_scene<float>(CrHandle* h) { return h->s32; }
template <> inline DevScene<double>& dev_scene<double>(CrHandle* h) { return h->s64; }

template <typename real> DevScene<real>& frame_scene(CrHandle* h);
template <> inline DevScene<float>& frame_scene<float>(CrHandle* h) { return h->f32; }
template <> inline DevScene<double>& frame_scene<double>(CrHandle* h) { return h->f64; }
// The frame trees go with the scene they were built from: cr_upload_scene, cr_update_primitives (the buffers stay for the next build)
inline void drop_frame_trees(CrHandle* h) {
    h->f32.frame_valid = false; h->f64.frame_valid = false;
    h->f32.info = CrBuildInfo(); h->f64.info = CrBuildInfo();
    h->s32.last_walk = kWalkNone; h->s64.last_walk = kWalkNone;
}

inline size_t real_size(int32_t real_type) { return real_type == CR_REAL_F64 ? sizeof(double) : sizeof(float); }

// what CrRenderParams.sum_order means on this handle: CR_SUM_DEFAULT is the handle's default in the megakernel and the
// reference order in the alternative pipelines
inline int resolve_sum_order(const CrHandle* h, const CrRenderParams* p) {
    return p->sum_order == CR_SUM_DEFAULT ? (h->pipeline == 0 ? h->default_sum_order : CR_SUM_REFERENCE_ORDER) : p->sum_order;
}

// The frames of one render: n frames whose ray times start at times[k] (host) and d_times[k] (the device's copy).  A
// single render is a batch of one without a table (its times start at KernelArgs::current_time).  RELAX kernels only.
struct AdaptiveRun;
template <typename real> struct FrameBatch {
    int32_t n = 1;
    const real* times = nullptr;
    const real* d_times = nullptr;
    const AdaptiveRun* ad = nullptr;   // cr_render_adaptive_*: launch() hands its kernel to adaptive_passes instead of launching it
};

// cr_render_adaptive_* (adaptive.hip).  What the entry point settled ...
struct AdaptiveRun {
    int32_t min_samples, pass_samples, block_log2;
    double tolerance;
    int32_t* d_counts;          // may be null; frame after frame
    CrAdaptiveStats* stats;     // may be null
    bool split_passes;          // cr_render_adaptive_region_*: a pass the work counter does not hold runs as several launches (else it is refused)
};
// ... and what launch() settled: the frame, the render kernel's tile shape and tile counts, the scale of the sums; of a
// batch (cr_render_adaptive_frames_*) the frame count and how many whole frames one launch's work counter holds
struct AdaptiveFrame {
    int32_t W, H, samples;      // W x H: the pixels the passes cover -- the region's (cr_render_adaptive_region_*), else the frame's
    int32_t n_frames, frames_per_launch;
    uint32_t lw, lh, tiles_x, tiles_y;
    double fx_scale;
    void* out;
    bool f64;
    int32_t n_entries, scene_in_lds;
};
// one launch of the render kernel over frames [f0, f0 + fn) of the batch: samples [s0, s1) of the n_tiles tiles `tile_list`
// names (batch-wide numbers, frame f0 first; nullptr: all, in order) into `acc` (frame f0's sums first)
using AdaptivePass = std::function<int32_t(int32_t f0, int32_t fn, const int32_t* tile_list, uint32_t n_tiles, int32_t s0, int32_t s1, unsigned long long* acc)>;
int32_t adaptive_passes(CrHandle* h, const AdaptiveRun& run, const AdaptiveFrame& fr, const AdaptivePass& pass);

// What one cr_render_* call covers, as its entry point settled it (api.hip) and as render_typed, aov_typed and prepare_args
// take it.  A new shape or family is a field here, not a parameter of every function underneath.
enum CallFamily { kCallRender, kCallGuide, kCallAdaptive, kCallGuideCounts };   // kCallGuideCounts: a guide call at a count plane (`counts`)
struct RenderCall {
    // the shape
    const int32_t* frames = nullptr;          // a batch's frame indices; nullptr: the one frame params->frame, and n_frames is 1
    int32_t n_frames = 1;
    const CrRegion* region = nullptr;         // the pixels of the one frame that the call covers; nullptr: the whole frame
    bool batch = false, region_call = false;  // the entry point is a cr_render_*_frames_* / cr_render_*_region_* call: the checks ask, the pointer may be null
    // the family
    CallFamily family = kCallRender;          // the entry point's: the checks ask before `layers` and `adaptive` can tell
    int32_t layers = 0;                       // the guide pass's CR_AOV_* mask; 0: a render
    const AdaptiveRun* adaptive = nullptr;    // a render to a noise target (adaptive.hip); nullptr: all samples of every pixel
    const CrCameraDesc* views = nullptr;      // cr_render_views_* / cr_render_aov_views_*: one camera per frame of the batch (n_frames of them, `frames` their
                                              // frame indices); nullptr: every frame through the call's one camera
    bool views_call = false;                  // the entry point is a views call: the checks ask, `views` may be null
    const int32_t* counts = nullptr;          // kCallGuideCounts: the samples each pixel takes, laid out as the adaptive sibling writes its counts;
                                              // device memory once call_device runs (call_host stages the caller's plane)
    bool guide() const { return family == kCallGuide || family == kCallGuideCounts; }

    size_t frame_pixels(const CrCameraDesc* cd) const {   // of one frame of the output
        return region ? (size_t)region->width * (size_t)region->height : (size_t)cd->image_width * (size_t)cd->image_height;
    }
    size_t layer_channels() const {   // reals per pixel of the planes `layers` names
        return (size_t)((layers & CR_AOV_ALBEDO ? 3 : 0) + (layers & CR_AOV_NORMAL ? 3 : 0) + (layers & CR_AOV_DEPTH ? 1 : 0) + (layers & CR_AOV_COVERAGE ? 1 : 0));
    }
    size_t frame_bytes(const CrCameraDesc* cd, const CrRenderParams* p) const {   // of one frame of the output: reals, or a render's fixed-point words
        return frame_pixels(cd) * (layers ? layer_channels() : 3) * (p->output_sum == CR_OUTPUT_FIXED_SUM ? sizeof(uint64_t) : real_size(p->real_type));
    }
};

// What render_typed settled before the residency ladder (render.hpp)
struct WalkChoice {
    bool anim, cam_keys;            // the kernel kind: keyed primitives, camera keys alone, neither
    bool screen;                    // walk on the f32 screening records (a.screen is set)
    bool screen_lds, plain_lds;     // the whole scene fits in LDS with screening records / with its wrappers
    size_t lds_all_screen;          // LDS bytes of the whole scene with screening records in the wrappers' place
};

// What launch() (render.hpp) needs to know about the kernel it runs, as launch_variant settled it.  A kernel's other
// template parameters (the tree order, the screening records, keyed primitives against camera keys) change its code, not its launch.
template <typename real> struct MegaKernel {
    void (*kern)(const KernelArgs<real>);
    void (*quiet)(const KernelArgs<real>);   // the twin that keeps no work counters; nullptr where none exists
    int res;                                 // RES_LDS / RES_TOP / RES_GLOBAL
    bool keyed;                              // ANIM || CAMK: carries a batch's frame arithmetic and a region's offsets
    bool latency, list;                      // the 6-waves-per-SIMD entry point; pathtrace_kernel_listed
};

// What a ladder asks residency.hpp's choose_residency about this tree on this handle.  The answer depends on the launch as
// well where the 6-waves-per-SIMD entry point may run: walk_ladder fills whole_frame and adaptive in, the guide pass, which
// has no such kernel, leaves them at never.
template <typename real, bool ORD>
ResidencyQuery residency_query(const CrHandle* h, const DevScene<real>& ds, const WalkChoice& w) {
    constexpr bool f32 = std::is_same<real, float>::value;
    ResidencyQuery q = {};
    q.n_entries = ds.n_entries;
    q.entry_rec = sizeof(typename EntryOf<real, ORD>::type); q.screen_rec = sizeof(typename ScreenOf<ORD>::type);
    q.ordered = ORD; q.can_screen = !(ORD && f32);
    q.screen = w.screen; q.screen_lds = w.screen_lds; q.plain_lds = w.plain_lds;
    q.lds_bytes = ds.lds_bytes; q.lds_all_screen = w.lds_all_screen;
    q.side_bytes = side_table_bytes((size_t)ds.n_mats * sizeof(Mat<real>), (size_t)ds.n_texs * sizeof(Tex<real>));
    q.lds_top_bytes = h->lds_top_bytes; q.lds_side_limit = h->lds_side_limit;
    q.f32 = f32; q.latency_entries = h->latency_entries; q.latency_top_bytes = h->latency_top_bytes;
    q.latency_slot_bytes = fx_lds_bytes(LatencyBlock, 4);
    return q;
}

// A scene in LDS whole, as residency.hpp lays it out: records of record_bytes each (its wrappers, or screening records in
// their place), primitive records and, with_side, materials and textures
template <typename real> inline SceneLayout whole_scene_layout(const DevScene<real>& ds, size_t record_bytes, bool with_side = true) {
    return scene_layout((size_t)ds.n_entries * record_bytes, (size_t)ds.n_prims * sizeof(Prim<real>), (size_t)ds.n_mats * sizeof(Mat<real>),
                        (size_t)ds.n_texs * sizeof(Tex<real>), true, with_side);
}
// LDS a scene takes when it sits there whole with its wrappers
template <typename real> inline size_t scene_lds_bytes(const DevScene<real>& ds) { return whole_scene_layout(ds, ds.entry_bytes).end(); }
// A frame tree's side tables are the base tree's (DevBuf::borrow: not owned)
template <typename real> inline void alias_side_tables(DevScene<real>& fs, const DevScene<real>& base) {
    fs.mats.borrow(base.mats); fs.texs.borrow(base.texs); fs.keys.borrow(base.keys);
    fs.n_mats = base.n_mats; fs.n_texs = base.n_texs; fs.n_scene_keys = base.n_scene_keys;
}

// build.hip
template <typename real> int32_t build_dev_scene(CrHandle* h);
// What a render or guide pass walks: builds the base tree, settles CrRenderParams.refit_boxes -- *refit: the
// base tree with this frame's boxes (CR_REFIT_BOXES) -- and under CR_REFIT_REBUILD builds or reuses the frame tree and
// returns that one in *walk.  batch: a cr_render_frames_* call.
template <typename real> int32_t select_tree(CrHandle* h, const CrRenderParams* p, bool batch, DevScene<real>** walk, bool* refit);
// sah_device.hip: the node graph and the primitive order of the SAH tree over n >= 1 boxes (6 doubles each: lo xyz, hi xyz)
struct SahNodeRec;
struct SahDeviceStats;
int32_t build_sah_device(CrHandle* h, const double* boxes, int32_t n, std::vector<SahNodeRec>& nodes, std::vector<int32_t>& order, SahDeviceStats& st);
// ... the same over boxes that are on the device already: h->sah_work.box holds them (n * 6 doubles, written on h->stream)
int32_t build_sah_device_resident(CrHandle* h, int32_t n, std::vector<SahNodeRec>& nodes, std::vector<int32_t>& order, SahDeviceStats& st);
// scene.hip
template <typename real> int32_t run_box_kernels(CrHandle* h, DevScene<real>& ds, void* entries, real ta, real tb, bool use_keys);
// A box plane of these wrappers that is not a number (DevScene::nan_planes; KernelArgs::exact_boxes)
template <typename real> inline bool has_nan_plane(const std::vector<Entry<real>>& entries) {
    for (const Entry<real>& e : entries) for (int k = 0; k < 6; k++) if (e.b[k] != e.b[k]) return true;
    return false;
}
int32_t make_screen(CrHandle* h, DevScene<double>& ds, const void* entries, DevBuf& out, bool* usable);
int32_t make_screen(CrHandle* h, DevScene<float>& ds, const void* entries, DevBuf& out, bool* usable);
int32_t validate_update(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, int32_t flags);
int32_t apply_update(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, int32_t flags);
// cr_update_materials, cr_update_image, cr_set_sky: everything that can refuse the call, then the edit itself
int32_t validate_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                           const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign);
int32_t apply_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                        const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign);
int32_t validate_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8);
int32_t apply_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8);
int32_t validate_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image);
void apply_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image);
// render.hip
int32_t finish_stats(CrHandle* h, CrStats* stats, uint64_t samples, int32_t bvh_entries, int32_t scene_in_lds);
int32_t pick_block(CrHandle* h, const void* kern, int max_block, bool ignore_large_override, size_t lds_base, size_t lds_per_wave,
                   const char* what, int& block, int& per_cu);
int32_t stage_frame_times(CrHandle* h, const void* times, size_t bytes);   // ray times into the handle's device table (times_dev), in stream order
template <typename real>
int32_t render_typed(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, void* d_out, CrStats* stats);
template <typename real>
int32_t prepare_args(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, DevScene<real>& ds, bool refit, bool mega,
                     void* d_out, std::vector<real>& times, KernelArgs<real>& a, WalkChoice& w, FrameBatch<real>& fb);
// render_f32_reference.hip, render_f32_relaxed.hip, render_f64_reference.hip, render_f64_relaxed.hip (render.hpp)
template <typename real, bool ORD, bool RELAX>
int32_t walk_ladder(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, CrStats* stats, const FrameBatch<real>& fb);
// render_views_f32.hip, render_views_f64.hip (render_views.hpp): the same ladder over the VIEWS kernels (a.views is set)
template <typename real, bool ORD>
int32_t views_ladder(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, CrStats* stats, const FrameBatch<real>& fb);
template <typename real>   // the relaxed units: fixed-point sums -> means (or raw sums) of `count` samples
int32_t fx_finalize(CrHandle* h, const unsigned long long* sums, real* out, size_t n, double inv_scale, double count, int32_t output_sum);
// alt_pipelines.hip
template <typename real> int32_t render_wavefront(CrHandle* h, const KernelArgs<real>& a, DevScene<real>& ds, bool anim, CrStats* stats);
template <typename real> int32_t render_queue(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, bool anim, CrStats* stats, bool* launched);
int32_t check_queue_abort(CrHandle* h);
// aov.hip: the guide pass (call.layers) after its argument checks; aov_f32.hip, aov_f64.hip: its kernels (aov.hpp)
template <typename real>
int32_t aov_typed(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, void* d_out, CrStats* stats);
// adaptive.hip: the adaptive family's own argument checks, after validate_render's
int32_t validate_adaptive(CrHandle* h, const CrRenderParams* p, const CrAdaptiveParams* ap, const void* out, const RenderCall& call);
// api.hip
int32_t validate_render(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrRegion* region = nullptr, bool region_call = false);
int32_t fixed_sums_to_rgb(CrHandle* h, const unsigned long long* sums, size_t n, int32_t samples, bool f64, void* out);
uint64_t bad_pixels(const void* rgb, int32_t real_type, size_t n_pix);   // pixels of a host frame with a mean outside [0,1] or NaN

}   // namespace cr
