// api.hip -- the handle's life and the render entry points of include/crucible_hip.h: cr_create reads the CRUCIBLE_*
// knobs; every cr_render_* entry point builds a RenderCall (handle.hpp), which is checked once and handed to render_typed
// (render.hip) or aov_typed (aov.hip) once, into device or host memory; the error strings behind cr_last_error.
//
// Nothing here falls back to a CPU renderer: without a HIP device cr_create fails.
#include "handle.hpp"

namespace cr {

static thread_local std::string g_create_error;

int32_t fail(CrHandle* h, int32_t code, const std::string& msg) {
    if (h) h->error = msg; else g_create_error = msg;
    return code;
}

// fixed-point sums of a whole frame of `samples` samples per pixel -> its per-pixel means, as launch() finalizes them
int32_t fixed_sums_to_rgb(CrHandle* h, const unsigned long long* sums, size_t n, int32_t samples, bool f64, void* out) {
    const double inv_scale = 1.0 / fx_scale_for(samples);
    return f64 ? fx_finalize<double>(h, sums, (double*)out, n, inv_scale, (double)samples, 0) : fx_finalize<float>(h, sums, (float*)out, n, inv_scale, (double)samples, 0);
}

// region_call: a cr_render_region_* / cr_render_aov_region_* call -- `region` is checked too, and the frame may have up to
// 2^31 - 1 pixels (the RNG key's pixel index has 32 bits) where a whole-frame call stops at 2^26
int32_t validate_render(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrRegion* region, bool region_call) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!cam || !p) return fail(h, CR_ERR_INVALID_ARG, "null camera or params");
    if (region_call && !region) return fail(h, CR_ERR_INVALID_ARG, "region is null");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_render before cr_upload_scene");
    if (cam->image_width < 1 || cam->image_height < 1) return fail(h, CR_ERR_INVALID_ARG, "image size must be positive");
    if (!region_call && (int64_t)cam->image_width * cam->image_height > (int64_t)1 << 26) return fail(h, CR_ERR_INVALID_ARG, "image too large");
    if (region_call) {
        if ((int64_t)cam->image_width * cam->image_height > (int64_t)INT32_MAX)
            return fail(h, CR_ERR_INVALID_ARG, "frame too large: a region's frame has at most 2^31 - 1 pixels");
        if (region->width < 1 || region->height < 1) return fail(h, CR_ERR_INVALID_ARG, "region size must be positive");
        if (region->x0 < 0 || region->y0 < 0) return fail(h, CR_ERR_INVALID_ARG, "region origin must not be negative");
        if ((int64_t)region->x0 + region->width > cam->image_width || (int64_t)region->y0 + region->height > cam->image_height)
            return fail(h, CR_ERR_INVALID_ARG, "region reaches outside the frame");
        if ((int64_t)region->width * region->height > (int64_t)1 << 26) return fail(h, CR_ERR_INVALID_ARG, "region too large (more than 2^26 pixels)");
    }
    if (p->samples < 1) return fail(h, CR_ERR_INVALID_ARG, "The camera must have a positive number of samples.");   // camera/mod.rs:235-238
    if (p->sample_begin < 0 || p->sample_count < 0 || (int64_t)p->sample_begin + p->sample_count > p->samples)   // (in 64 bits: the sum of two int32 may pass 2^31)
        return fail(h, CR_ERR_INVALID_ARG, "sample range outside [0, samples)");
    if (p->max_depth < 0) return fail(h, CR_ERR_INVALID_ARG, "max_depth must be >= 0");
    if (p->real_type != CR_REAL_F32 && p->real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    if (p->sum_order != CR_SUM_DEFAULT && p->sum_order != CR_SUM_REFERENCE_ORDER && p->sum_order != CR_SUM_RELAXED) return fail(h, CR_ERR_INVALID_ARG, "unknown sum_order");
    if (p->output_sum < 0 || p->output_sum > CR_OUTPUT_FIXED_SUM) return fail(h, CR_ERR_INVALID_ARG, "unknown output_sum");
    if (!(p->frame_rate > 0)) return fail(h, CR_ERR_INVALID_ARG, "frame_rate must be positive");
    if ((cam->from_key_count > 0 && !cam->from_keys) || (cam->at_key_count > 0 && !cam->at_keys) || cam->from_key_count < 0 || cam->at_key_count < 0)
        return fail(h, CR_ERR_INVALID_ARG, "camera keyframe array missing");
    for (int i = 0; i < cam->from_key_count + cam->at_key_count; i++) {   // cam_translate_* only (scene_animator.rs)
        const CrKeyframe& k = i < cam->from_key_count ? cam->from_keys[i] : cam->at_keys[i - cam->from_key_count];
        if (k.channel < CR_KEY_TX || k.channel > CR_KEY_TZ || (k.interp != CR_KEY_NERP && k.interp != CR_KEY_LERP))
            return fail(h, CR_ERR_INVALID_ARG, "camera keyframes are translations (channels 0..2)");
    }
    return CR_OK;
}

// The checks of every cr_render_* entry point: a render's, then the family's own in the order each family has had them --
// a call with two faults reports the first.  render: frames, n_frames, out, the region's sum order.  guide layers: frames,
// n_frames, the layer mask, out, the fixed-point refusal; at a count plane after those the plane, then the shard.
// adaptive: validate_adaptive's (out among them), then frames, n_frames.
// views (cr_render_views_*, cr_render_aov_views_*): the views' own checks come first -- the table, then each view as a single
// call of it is checked, then the frame sizes --, and behind the family's checks what a batch of views cannot do.
static int32_t validate_call(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const RenderCall& call, const void* out,
                             const CrAdaptiveParams* ap) {
    if (call.views_call) {
        if (!h) return CR_ERR_INVALID_ARG;
        if (!call.views) return fail(h, CR_ERR_INVALID_ARG, "cams is null");
        if (call.n_frames < 1) return fail(h, CR_ERR_INVALID_ARG, "n_views must be at least 1");
        for (int32_t k = 0; k < call.n_frames; k++) {
            const int32_t rv = validate_render(h, &call.views[k], p);
            if (rv != CR_OK) return fail(h, rv, "view " + std::to_string(k) + ": " + h->error);
            if (call.views[k].image_width != call.views[0].image_width || call.views[k].image_height != call.views[0].image_height)
                return fail(h, CR_ERR_INVALID_ARG, "view " + std::to_string(k) + ": the views of a call have one image size (view 0's)");
        }
    }
    int32_t rc = validate_render(h, cam, p, call.region, call.region_call);
    if (rc != CR_OK) return rc;
    if (call.family == kCallAdaptive && (rc = validate_adaptive(h, p, ap, out, call)) != CR_OK) return rc;
    if (call.batch && !call.frames) return fail(h, CR_ERR_INVALID_ARG, "frames is null");
    if (call.batch && call.n_frames < 1) return fail(h, CR_ERR_INVALID_ARG, "n_frames must be at least 1");
    if (call.family == kCallAdaptive) return CR_OK;
    const int32_t all = CR_AOV_ALBEDO | CR_AOV_NORMAL | CR_AOV_DEPTH | CR_AOV_COVERAGE;
    if (call.guide() && (call.layers == 0 || (call.layers & ~all))) return fail(h, CR_ERR_INVALID_ARG, "layers must be a non-empty mask of CR_AOV_*");
    if (!out) return fail(h, CR_ERR_INVALID_ARG, "output buffer is null");
    if (call.guide() && p->output_sum == CR_OUTPUT_FIXED_SUM)
        return fail(h, CR_ERR_UNSUPPORTED, "guide layers come as reals (output_sum 0 or 1), not as fixed-point words");
    if (call.family == kCallGuideCounts && !call.counts) return fail(h, CR_ERR_INVALID_ARG, "counts is null");
    if (call.family == kCallGuideCounts && (p->sample_begin != 0 || p->sample_count != p->samples))
        return fail(h, CR_ERR_UNSUPPORTED, "guide layers at a count plane take a pixel's samples from sample 0 (sample_begin 0, sample_count == samples), "
                                           "as the adaptive calls do");
    if (call.views_call) {
        if (call.family == kCallRender && (resolve_sum_order(h, p) != CR_SUM_RELAXED || h->pipeline != 0))
            return fail(h, CR_ERR_UNSUPPORTED, "cr_render_views needs CR_SUM_RELAXED and the megakernel pipeline, as cr_render_frames does");
        int64_t keys = 0;
        for (int32_t k = 0; k < call.n_frames; k++) keys += (int64_t)call.views[k].from_key_count + call.views[k].at_key_count;
        if (keys > (int64_t)CrHandle::kMaxCamKeys) return fail(h, CR_ERR_UNSUPPORTED, "more than 512 camera keyframes over all views");
    }
    if (call.family == kCallRender && call.region_call && (resolve_sum_order(h, p) != CR_SUM_RELAXED || h->pipeline != 0))
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_region needs CR_SUM_RELAXED and the megakernel pipeline (a reference-order sum is "
                                           "sequential over samples; the region's offsets live in the relaxed kernels)");
    return CR_OK;
}

// A checked call into device memory: the family's typed function of the params' precision, then the camera-key slot's release
static int32_t call_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const RenderCall& call, void* d_out, CrStats* stats) {
    HIP_TRY(h, hipSetDevice(h->device));
    h->cam_pending_slot = -1;
    const bool f64 = p->real_type == CR_REAL_F64;
    int32_t rc = call.layers ? (f64 ? aov_typed<double>(h, cam, p, call, d_out, stats) : aov_typed<float>(h, cam, p, call, d_out, stats))
                             : (f64 ? render_typed<double>(h, cam, p, call, d_out, stats) : render_typed<float>(h, cam, p, call, d_out, stats));
    if (h->cam_pending_slot >= 0) {   // the camera-key slot is free again once everything queued so far has run
        hipError_t e = hipEventRecord(h->cam[h->cam_pending_slot].ev, h->stream);
        h->cam_pending_slot = -1;
        if (e != hipSuccess && rc == CR_OK) { h->error = std::string("hipEventRecord: ") + hipGetErrorString(e); rc = CR_ERR_HIP; }
    }
    return rc;
}

// Color::new asserts 0 <= c <= 1 on every mean (ray_casting.rs:172): the pixels of a host frame that would panic there
uint64_t bad_pixels(const void* rgb, int32_t real_type, size_t n_pix) {
    uint64_t bad = 0;
    for (size_t i = 0; i < n_pix; i++) {
        bool ok = true;
        for (int k = 0; k < 3; k++) {
            double v = real_type == CR_REAL_F64 ? ((const double*)rgb)[3 * i + k] : (double)((const float*)rgb)[3 * i + k];
            ok = ok && (v >= 0.0 && v <= 1.0);
        }
        bad += ok ? 0 : 1;
    }
    return bad;
}

// A checked call into host memory: into the handle's buffers (the output's; the counts' when an adaptive call asks for
// them; a guide call's count plane, copied in on the stream before the launch), copy back, and where the family's output is a frame of colour means, check them frame by frame
static int32_t call_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, RenderCall call, void* h_out, CrStats* stats) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_pix = call.frame_pixels(cam), frame_bytes = call.frame_bytes(cam, p);
    const size_t bytes = frame_bytes * (size_t)call.n_frames, count_bytes = n_pix * (size_t)call.n_frames * sizeof(int32_t);
    AdaptiveRun run = {};            // the caller's run with the counts in the handle's buffer
    int32_t* h_counts = nullptr;
    hipError_t e = h->out_buf.ensure(bytes);
    if (call.adaptive) {
        run = *call.adaptive;
        h_counts = run.d_counts;
        if (e == hipSuccess && h_counts) e = h->ad_counts.ensure(count_bytes);
        run.d_counts = h_counts ? (int32_t*)h->ad_counts.p : nullptr;
        call.adaptive = &run;
    }
    if (e == hipSuccess && call.counts) e = h->aov_counts.ensure(count_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("output buffer: ") + hipGetErrorString(e)); }
    if (call.counts) {
        HIP_TRY(h, hipMemcpyAsync(h->aov_counts.p, call.counts, count_bytes, hipMemcpyHostToDevice, h->stream));
        call.counts = (const int32_t*)h->aov_counts.p;
    }
    // a caller's null stats is passed on: such a render keeps no work counters where a kernel without them exists (render.hpp launch())
    int32_t rc = call_device(h, cam, p, call, h->out_buf.p, stats);
    if (rc != CR_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h_out, h->out_buf.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h_counts) HIP_TRY(h, hipMemcpyAsync(h_counts, h->ad_counts.p, count_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the pixel check is for colour means: guide layers have none, and a render's sums (output_sum != 0; an adaptive
    // call's is 0) are not means
    if (call.layers || p->output_sum) return CR_OK;
    uint64_t bad = 0;
    int32_t first_bad = -1;
    for (int32_t k = 0; k < call.n_frames; k++) {
        const uint64_t b = bad_pixels((const char*)h_out + (size_t)k * frame_bytes, p->real_type, n_pix);
        if (b && first_bad < 0) first_bad = k;
        bad += b;
    }
    // nan_pixels lands in the render's CrStats, or in the CrStats inside the adaptive call's
    CrStats* const into = !call.adaptive ? stats : (run.stats ? &run.stats->render : nullptr);
    if (into) into->nan_pixels = bad;
    if (bad && !call.frames) return fail(h, CR_ERR_NAN, "a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)");
    if (bad && call.views)
        return fail(h, CR_ERR_NAN, "view " + std::to_string(first_bad) + " (frame " + std::to_string(call.frames[first_bad]) +
                                       "): a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)");
    if (bad)
        return fail(h, CR_ERR_NAN, "frame " + std::to_string(call.frames[first_bad]) + " (entry " + std::to_string(first_bad) +
                                       " of the batch): a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)");
    return CR_OK;
}

// What an adaptive entry point was given beside a render's arguments
struct AdaptiveAsk {
    const CrAdaptiveParams* ap = nullptr;
    int32_t* counts = nullptr;          // may be null; device or host memory as the output is
    CrAdaptiveStats* stats = nullptr;   // may be null
};

constexpr bool kDevice = false, kHost = true;   // run_call's `host`

// Every cr_render_* entry point: the checks, then the call into device or host memory (an adaptive call's stats are `ask`'s)
static int32_t run_call(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, RenderCall call, bool host, void* out, CrStats* stats,
                        const AdaptiveAsk& ask = {}) {
    const int32_t rc = validate_call(h, cam, p, call, out, ask.ap);
    if (rc != CR_OK) return rc;
    std::vector<int32_t> same_frame;   // a views call without frame indices: params->frame for every view
    if (call.views_call && !call.frames) { same_frame.assign((size_t)call.n_frames, p->frame); call.frames = same_frame.data(); }
    AdaptiveRun run = {};
    if (call.family == kCallAdaptive) {
        run = {ask.ap->min_samples, ask.ap->pass_samples, ask.ap->block_log2 ? ask.ap->block_log2 : 4, ask.ap->tolerance, ask.counts, ask.stats, call.region != nullptr};
        call.adaptive = &run;
    }
    return host ? call_host(h, cam, p, call, out, stats) : call_device(h, cam, p, call, out, stats);
}

// The descriptors the entry points start from: the shape, then the family
static RenderCall one_frame() { return RenderCall(); }
static RenderCall batch_of(const int32_t* frames, int32_t n_frames) { RenderCall c; c.frames = frames; c.n_frames = n_frames; c.batch = true; return c; }
static RenderCall views_of(const CrCameraDesc* cams, int32_t n_views, const int32_t* frames) {   // a batch whose frame k has the camera cams[k]
    RenderCall c; c.views = cams; c.views_call = true; c.frames = frames; c.n_frames = n_views; return c;
}
static const CrCameraDesc* first_view(const CrCameraDesc* cams, int32_t n_views) { return n_views >= 1 ? cams : nullptr; }   // the call's camera: view 0
static RenderCall region_of(const CrRegion* region) { RenderCall c; c.region = region; c.region_call = true; return c; }
static RenderCall guide(RenderCall c, int32_t layers) { c.family = kCallGuide; c.layers = layers; return c; }
static RenderCall guide_at(RenderCall c, int32_t layers, const int32_t* counts) { c.family = kCallGuideCounts; c.layers = layers; c.counts = counts; return c; }
static RenderCall adaptive(RenderCall c) { c.family = kCallAdaptive; return c; }

}   // namespace cr

using namespace cr;

extern "C" {

int32_t cr_abi_version(void) { return CR_ABI_VERSION; }

int32_t cr_create(int32_t device_id, CrHandle** out) {
    if (!out) return fail(nullptr, CR_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev < 1) return fail(nullptr, CR_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, CR_ERR_INVALID_ARG, "device_id out of range");
    CrHandle* h = new CrHandle();
    h->device = device_id;
    auto bail = [&](const char* what, hipError_t err) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        delete h;
        return CR_ERR_HIP;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    h->n_cus = prop.multiProcessorCount;
    if ((e = h->stream.create(hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = h->ev0.create()) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = h->ev1.create()) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = h->work_counter.ensure(16)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = h->counters.ensure(64 * sizeof(uint64_t))) != hipSuccess) return bail("hipMalloc", e);
    if (const char* s = getenv("CRUCIBLE_LDS_LIMIT")) h->lds_limit = (size_t)atol(s);
    if (const char* s = getenv("CRUCIBLE_SAMPLE_GRANULAR")) h->sample_granular = atoi(s) != 0;
    if (const char* s = getenv("CRUCIBLE_SCREEN")) h->screen_boxes = atoi(s) != 0;
    if (const char* s = getenv("CRUCIBLE_SCREEN_LDS")) h->screen_lds = atoi(s) != 0;
    if (const char* s = getenv("CRUCIBLE_SUM_ORDER")) h->default_sum_order = strcmp(s, "reference") == 0 ? CR_SUM_REFERENCE_ORDER : CR_SUM_RELAXED;
    if (const char* s = getenv("CRUCIBLE_SAMPLE_BUF_MB")) h->sample_buf_limit = (size_t)std::max(0L, atol(s)) << 20;
    if (const char* s = getenv("CRUCIBLE_SG_CHUNK")) h->sg_chunk_override = std::max(0, atoi(s));
    if (const char* s = getenv("CRUCIBLE_WORK_COUNTER_MAX")) h->work_counter_max = std::min<uint64_t>(0xF0000000ull, (uint64_t)std::max(64LL, atoll(s)));
    if (const char* s = getenv("CRUCIBLE_SG_TILE")) {
        int tw = 0, th = 0;
        if (sscanf(s, "%dx%d", &tw, &th) == 2 && tw > 0 && th > 0 && (tw & (tw - 1)) == 0 && (th & (th - 1)) == 0 && tw * th <= 64) {
            h->sg_lw = __builtin_ctz((unsigned)tw); h->sg_lh = __builtin_ctz((unsigned)th);
        }
    }
    if (const char* s = getenv("CRUCIBLE_LATENCY_ENTRIES")) h->latency_entries = (int32_t)std::max(0L, atol(s));
    if (const char* s = getenv("CRUCIBLE_LATENCY_TOP_KB")) h->latency_top_bytes = (size_t)std::max(0L, atol(s)) * 1024;
    if (const char* s = getenv("CRUCIBLE_LDS_SIDE_KB")) h->lds_side_limit = (size_t)std::max(0L, atol(s)) * 1024;
    if (const char* s = getenv("CRUCIBLE_LDS_TOP_KB")) h->lds_top_bytes = (size_t)std::max(0L, atol(s)) * 1024;
    if (const char* s = getenv("CRUCIBLE_BLOCKS_PER_CU")) h->blocks_per_cu_override = atoi(s);
    if (const char* s = getenv("CRUCIBLE_BLOCK")) h->block_override = atoi(s);
    if (const char* s = getenv("CRUCIBLE_WALK_ROUND")) h->walk_round_steps = std::max(0, atoi(s));
    if (const char* s = getenv("CRUCIBLE_WALK_EXIT")) h->walk_exit_lanes = std::min(64, std::max(1, atoi(s)));
    if (const char* s = getenv("CRUCIBLE_WALK_LEAF_MIN")) h->walk_leaf_min = std::min(64, std::max(0, atoi(s)));
    if (const char* s = getenv("CRUCIBLE_PIPELINE")) h->pipeline = strcmp(s, "mega") == 0 ? 0 : (strcmp(s, "queue") == 0 ? 2 : 1);
    if (const char* s = getenv("CRUCIBLE_QUEUE_BATCH")) h->queue_min_batch = std::min(64, std::max(1, atoi(s)));
    if (const char* s = getenv("CRUCIBLE_QUEUE_PATIENCE")) h->queue_patience = std::max(0, atoi(s));
    if (const char* s = getenv("CRUCIBLE_QUEUE_WALKERS")) h->queue_walk_waves = std::min(15, std::max(1, atoi(s)));
    if (const char* s = getenv("CRUCIBLE_WF_SLOTS")) h->wf_slots = (uint32_t)std::max(64L, atol(s));
    if (const char* s = getenv("CRUCIBLE_WF_SAMPLE_MB")) h->wf_sample_bytes = (size_t)std::max(1L, atol(s)) << 20;
    *out = h;
    return CR_OK;
}

void cr_destroy(CrHandle* h) { if (h) delete h; }   // ~CrHandle drains the stream; the members give their resources back

// The twenty-eight render entry points: four families (render, guide layers, adaptive, guide layers at a count plane) in
// three shapes (one frame, a batch of frames, a region of a frame) into device or host memory, and the batches of views of
// the first two families (cr_render_views_*, cr_render_aov_views_*) -- each a RenderCall and where its results go.

int32_t cr_render_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, void* d_out, CrStats* stats) {
    return run_call(h, cam, p, one_frame(), kDevice, d_out, stats);
}

int32_t cr_render_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, void* h_out, CrStats* stats) {
    return run_call(h, cam, p, one_frame(), kHost, h_out, stats);
}

int32_t cr_render_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const int32_t* frames, int32_t n_frames,
                                void* d_out, CrStats* stats) {
    return run_call(h, cam, p, batch_of(frames, n_frames), kDevice, d_out, stats);
}

int32_t cr_render_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const int32_t* frames, int32_t n_frames,
                              void* h_out, CrStats* stats) {
    return run_call(h, cam, p, batch_of(frames, n_frames), kHost, h_out, stats);
}

int32_t cr_render_views_device(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, const CrRenderParams* p,
                               void* d_out, CrStats* stats) {
    return run_call(h, first_view(cams, n_views), p, views_of(cams, n_views, frames), kDevice, d_out, stats);
}

int32_t cr_render_views_host(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, const CrRenderParams* p,
                             void* h_out, CrStats* stats) {
    return run_call(h, first_view(cams, n_views), p, views_of(cams, n_views, frames), kHost, h_out, stats);
}

int32_t cr_render_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrRegion* region, void* d_out, CrStats* stats) {
    return run_call(h, cam, p, region_of(region), kDevice, d_out, stats);
}

int32_t cr_render_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrRegion* region, void* h_out, CrStats* stats) {
    return run_call(h, cam, p, region_of(region), kHost, h_out, stats);
}

int32_t cr_render_aov_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide(one_frame(), layers), kDevice, d_out, stats);
}

int32_t cr_render_aov_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide(one_frame(), layers), kHost, h_out, stats);
}

int32_t cr_render_aov_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* frames, int32_t n_frames,
                                    void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide(batch_of(frames, n_frames), layers), kDevice, d_out, stats);
}

int32_t cr_render_aov_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* frames, int32_t n_frames,
                                  void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide(batch_of(frames, n_frames), layers), kHost, h_out, stats);
}

int32_t cr_render_aov_views_device(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, const CrRenderParams* p,
                                   int32_t layers, void* d_out, CrStats* stats) {
    return run_call(h, first_view(cams, n_views), p, guide(views_of(cams, n_views, frames), layers), kDevice, d_out, stats);
}

int32_t cr_render_aov_views_host(CrHandle* h, const CrCameraDesc* cams, int32_t n_views, const int32_t* frames, const CrRenderParams* p,
                                 int32_t layers, void* h_out, CrStats* stats) {
    return run_call(h, first_view(cams, n_views), p, guide(views_of(cams, n_views, frames), layers), kHost, h_out, stats);
}

int32_t cr_render_aov_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const CrRegion* region,
                                    void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide(region_of(region), layers), kDevice, d_out, stats);
}

int32_t cr_render_aov_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const CrRegion* region,
                                  void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide(region_of(region), layers), kHost, h_out, stats);
}

int32_t cr_render_aov_counts_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* d_counts,
                                    void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(one_frame(), layers, d_counts), kDevice, d_out, stats);
}

int32_t cr_render_aov_counts_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* h_counts,
                                  void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(one_frame(), layers, h_counts), kHost, h_out, stats);
}

int32_t cr_render_aov_counts_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* frames,
                                           int32_t n_frames, const int32_t* d_counts, void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(batch_of(frames, n_frames), layers, d_counts), kDevice, d_out, stats);
}

int32_t cr_render_aov_counts_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const int32_t* frames,
                                         int32_t n_frames, const int32_t* h_counts, void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(batch_of(frames, n_frames), layers, h_counts), kHost, h_out, stats);
}

int32_t cr_render_aov_counts_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const CrRegion* region,
                                           const int32_t* d_counts, void* d_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(region_of(region), layers, d_counts), kDevice, d_out, stats);
}

int32_t cr_render_aov_counts_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, int32_t layers, const CrRegion* region,
                                         const int32_t* h_counts, void* h_out, CrStats* stats) {
    return run_call(h, cam, p, guide_at(region_of(region), layers, h_counts), kHost, h_out, stats);
}

int32_t cr_render_adaptive_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, void* d_out,
                                  int32_t* d_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(one_frame()), kDevice, d_out, nullptr, {ap, d_counts, stats});
}

int32_t cr_render_adaptive_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, void* h_out,
                                int32_t* h_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(one_frame()), kHost, h_out, nullptr, {ap, h_counts, stats});
}

int32_t cr_render_adaptive_frames_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap,
                                         const int32_t* frames, int32_t n_frames, void* d_out, int32_t* d_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(batch_of(frames, n_frames)), kDevice, d_out, nullptr, {ap, d_counts, stats});
}

int32_t cr_render_adaptive_frames_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap,
                                       const int32_t* frames, int32_t n_frames, void* h_out, int32_t* h_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(batch_of(frames, n_frames)), kHost, h_out, nullptr, {ap, h_counts, stats});
}

int32_t cr_render_adaptive_region_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap,
                                         const CrRegion* region, void* d_out, int32_t* d_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(region_of(region)), kDevice, d_out, nullptr, {ap, d_counts, stats});
}

int32_t cr_render_adaptive_region_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap,
                                       const CrRegion* region, void* h_out, int32_t* h_counts, CrAdaptiveStats* stats) {
    return run_call(h, cam, p, adaptive(region_of(region)), kHost, h_out, nullptr, {ap, h_counts, stats});
}

int32_t cr_fixed_sums_to_rgb(CrHandle* h, const uint64_t* d_sums, int32_t width, int32_t height, int32_t samples, int32_t real_type,
                             void* d_out_rgb) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!d_sums || !d_out_rgb) return fail(h, CR_ERR_INVALID_ARG, "cr_fixed_sums_to_rgb: null buffer");
    if (width < 1 || height < 1) return fail(h, CR_ERR_INVALID_ARG, "image size must be positive");
    if ((int64_t)width * height > (int64_t)1 << 26) return fail(h, CR_ERR_INVALID_ARG, "image too large");
    if (samples < 1) return fail(h, CR_ERR_INVALID_ARG, "The camera must have a positive number of samples.");
    if (real_type != CR_REAL_F32 && real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    HIP_TRY(h, hipSetDevice(h->device));
    return fixed_sums_to_rgb(h, (const unsigned long long*)d_sums, (size_t)width * (size_t)height * 3, samples, real_type == CR_REAL_F64, d_out_rgb);
}

int32_t cr_last_kernel_ms(CrHandle* h, double* out_ms) {
    if (!h || !out_ms) return CR_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *out_ms = ms;
    return check_queue_abort(h);
}

int32_t cr_synchronize(CrHandle* h) {
    if (!h) return CR_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue_abort(h);
}

void* cr_stream(CrHandle* h) { return h ? (void*)h->stream : nullptr; }

const char* cr_last_error(CrHandle* h) { return h ? h->error.c_str() : g_create_error.c_str(); }

}   // extern "C"
