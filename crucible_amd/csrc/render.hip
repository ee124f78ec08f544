// render.hip -- a render up to its kernel: render_typed has prepare_args fill the kernel arguments (camera, frame times,
// refitted boxes, screening records) and hands them to the residency ladder of the precision and sum order (render.hpp, render_*.hip)
// or to a cross-check pipeline (alt_pipelines.hip).  Also what every launch path shares: the workgroup-size choice and
// the stats epilogue.  No kernel is emitted here.
#include "handle.hpp"
#include "pack.hpp"

namespace cr {

// After ev1 was recorded behind a render of `samples` samples: its time and work counters into *stats.  No samples (an
// empty shard): no kernel ran, the counters are an earlier render's and stay unread.
int32_t finish_stats(CrHandle* h, CrStats* stats, uint64_t samples, int32_t bvh_entries, int32_t scene_in_lds) {
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    uint64_t c[4] = {0, 0, 0, 0};
    if (samples > 0) HIP_TRY(h, hipMemcpy(c, h->counters.p, sizeof c, hipMemcpyDeviceToHost));
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = ms;
    stats->segments = c[0]; stats->node_tests = c[1]; stats->prim_tests = c[2]; stats->texel_fetches = c[3];
    stats->samples = samples;
    stats->upload_ms = h->upload_ms;
    stats->bvh_entries = bvh_entries;
    stats->scene_in_lds = scene_in_lds;
    return CR_OK;
}

// Workgroup size and workgroups per CU of `kern`: the candidate that keeps the most waves resident per CU (a larger
// workgroup shares one LDS copy of the scene among more waves); ties go to the larger.  A workgroup of w waves asks for
// lds_base + w * lds_per_wave bytes of LDS.  CRUCIBLE_BLOCK narrows the candidates to one; the two callers differ in an
// override above max_block: the megakernel ignores it (ignore_large_override), the wavefront driver is left without a
// candidate and reports that the kernel does not fit.
int32_t pick_block(CrHandle* h, const void* kern, int max_block, bool ignore_large_override, size_t lds_base, size_t lds_per_wave,
                   const char* what, int& block, int& per_cu) {
    int best_waves = 0;
    block = 256; per_cu = 1;
    for (int cand : {1024, 512, 256}) {
        if (cand > max_block) continue;
        if (h->block_override > 0 && cand != h->block_override && !(ignore_large_override && h->block_override > max_block)) continue;
        int n = 0;
        HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, cand, lds_base + (size_t)(cand / 64) * lds_per_wave));
        if (n * cand / 64 > best_waves) { best_waves = n * cand / 64; block = cand; per_cu = n; }
    }
    if (best_waves == 0) return fail(h, CR_ERR_HIP, what);
    if (h->blocks_per_cu_override > 0) per_cu = h->blocks_per_cu_override;
    return CR_OK;
}

// cr_render_frames_*: the batch's ray times through the handle's pinned staging buffer into its device table
// (cr_render_views_*: the views' camera records behind the times, one table)
int32_t stage_frame_times(CrHandle* h, const void* times, size_t bytes) {
    if (h->times_ev) HIP_TRY(h, hipEventSynchronize(h->times_ev));   // the previous batch's copy has read the staging buffer
    else HIP_TRY(h, h->times_ev.create(hipEventDisableTiming));
    {
        const hipError_t e = h->times_host.ensure(bytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("frame times: ") + hipGetErrorString(e)); }
    }
    const hipError_t e = h->times_dev.ensure(bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("frame times: ") + hipGetErrorString(e)); }
    memcpy(h->times_host.p, times, bytes);
    HIP_TRY(h, hipMemcpyAsync(h->times_dev.p, h->times_host.p, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->times_ev, h->stream));
    return CR_OK;
}

// What a render settles before its kernels are chosen, shared with the guide pass (aov.hip): the kernel arguments (scene
// tables, camera and its key slot, sample range, ray times -- of a batch's frames too --, this frame's refitted boxes and
// screening records, the walk's scheduling knobs) and the kernel kind.  mega: the walk runs in a megakernel-style kernel
// (screening records, parked leaves); the cross-check pipelines walk without either.  call: its frames and the pixels of
// the frame that the launch covers (call.region; nullptr: all of them).
template <typename real>
int32_t prepare_args(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, DevScene<real>& ds, bool refit, bool mega,
                     void* d_out, std::vector<real>& times, KernelArgs<real>& a, WalkChoice& w, FrameBatch<real>& fb) {
    const int32_t* const frames = call.frames;
    const CrRegion* const region = call.region;
    memset(&a, 0, sizeof a);
    a.entries = (const Entry<real>*)ds.entries.p; a.prims = (const Prim<real>*)ds.prims.p; a.leaf_runs = ds.has_leaf_runs ? (const int32_t*)ds.leaf_runs.p : nullptr;
    a.mats = (const Mat<real>*)ds.mats.p; a.texs = (const Tex<real>*)ds.texs.p;
    a.images = (const ImageRef*)h->images.p; a.texels = (const uint32_t*)h->texels.p;
    a.keys = (const Key<real>*)ds.keys.p;
    a.n_entries = ds.n_entries; a.n_prims = ds.n_prims; a.n_mats = ds.n_mats; a.n_texs = ds.n_texs;
    a.sky_kind = h->sky_kind; a.sky_image = h->sky_image;

    // camera set-up (pack.hpp)
    // (cr_render_views_*: cd is view 0, whose record a.cam holds for the frame's size; the views' records go into a table of
    // their own and their keys one view after the other into the one slot -- pack.hpp pack_views)
    CamConst<real>& c = a.cam;
    pack_camera(cd, c);
    int64_t nk = (int64_t)cd->from_key_count + cd->at_key_count;
    std::vector<CamConst<real>> views;
    if (call.views) { views.resize((size_t)call.n_frames); nk = pack_views(call.views, call.n_frames, views.data()); }
    if (nk > (int64_t)CrHandle::kMaxCamKeys)
        return fail(h, CR_ERR_UNSUPPORTED, call.views ? "more than 512 camera keyframes over all views" : "more than 512 camera keyframes");
    a.cam_keys = nullptr;
    if (nk > 0) {   // per-launch slot: never overwritten while an earlier render may still read it
        const int slot = h->cam_next;
        h->cam_next = (slot + 1) % CrHandle::kCamSlots;
        const size_t slot_bytes = CrHandle::kMaxCamKeys * sizeof(Key<double>);
        CamSlot& cs = h->cam[slot];
        if (!cs) {   // the slot's three resources together, or none of them (a later render tries again)
            const hipError_t e = cs.acquire(slot_bytes);
            if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("camera keyframe slot: ") + hipGetErrorString(e)); }
        } else HIP_TRY(h, hipEventSynchronize(cs.ev));   // the slot's previous user has finished with it
        Key<real>* ck = (Key<real>*)cs.host.p;
        if (call.views) pack_view_keys(call.views, call.n_frames, ck);
        else pack_view_keys(cd, 1, ck);
        HIP_TRY(h, hipMemcpyAsync(cs.dev.p, ck, nk * sizeof(Key<real>), hipMemcpyHostToDevice, h->stream));
        a.cam_keys = (const Key<real>*)cs.dev.p;
        h->cam_pending_slot = slot;
    }
    pack_camera_frame(c);   // static camera: the per-sample vectors
    a.reg_x0 = region ? (uint32_t)region->x0 : 0u; a.reg_y0 = region ? (uint32_t)region->y0 : 0u;
    a.reg_w = (uint32_t)(region ? region->width : c.W); a.reg_h = (uint32_t)(region ? region->height : c.H);

    a.sample_begin = p->sample_begin; a.sample_end = p->sample_begin + p->sample_count;
    a.samples_total = p->samples; a.max_depth = p->max_depth;
    a.seed_mixed = mix64(p->seed + RNG_GAMMA);
    frame_times(p, a.current_time, a.shutter_length);   // ray_casting.rs:77-79
    a.output_sum = p->output_sum;
    a.exact_boxes = (!refit && ds.nan_planes) ? 1 : 0;   // the boxes of a refit hold no NaN (refit.hpp box_is_number)
    if (frames) {   // each frame's times as a single render of it computes them (the shutter is the same for all)
        times.resize((size_t)call.n_frames);
        CrRenderParams q = *p;
        for (int32_t k = 0; k < call.n_frames; k++) { q.frame = frames[k]; frame_times(&q, times[(size_t)k], a.shutter_length); }
        // (cr_render_views_*: one table, the views' camera records behind the times at the next multiple of 16 bytes)
        const size_t time_bytes = times.size() * sizeof(real), views_at = (time_bytes + 15) & ~(size_t)15;
        std::vector<char> table(call.views ? views_at + views.size() * sizeof(CamConst<real>) : 0);
        if (call.views) {
            memcpy(table.data(), times.data(), time_bytes);
            memcpy(table.data() + views_at, views.data(), views.size() * sizeof(CamConst<real>));
        }
        int32_t rc = call.views ? stage_frame_times(h, table.data(), table.size()) : stage_frame_times(h, times.data(), time_bytes);
        if (rc != CR_OK) return rc;
        a.current_time = times[0];
        fb.n = call.n_frames; fb.times = times.data(); fb.d_times = (const real*)h->times_dev.p;
        if (call.views) a.views = (const CamConst<real>*)((const char*)h->times_dev.p + views_at);
    }
    if (refit) {   // refit.hpp: wrapper boxes for this frame's ray times [current_time, current_time + shutter_length]
        const size_t bytes = (size_t)ds.n_entries * ds.entry_bytes;
        HIP_TRY(h, ds.entries_refit.ensure(bytes, ds.entries.pad));
        HIP_TRY(h, hipMemcpyAsync(ds.entries_refit.p, ds.entries.p, bytes, hipMemcpyDeviceToDevice, h->stream));
        { int32_t rc = run_box_kernels<real>(h, ds, ds.entries_refit.p, a.current_time, a.current_time + a.shutter_length, true); if (rc != CR_OK) return rc; }
        a.entries = (const Entry<real>*)ds.entries_refit.p;
    }
    // f64 megakernel on an unordered tree: the walk decides its box tests on the f32 screening records (half the bytes
    // per step), see walk_round (A/B in profiles/experiments/r03_screen_ab.txt).
    // (not on a tree with a box plane beyond the f32 range: make_screen)
    bool screen = mega && ds.screen.p != nullptr && ds.n_entries > 0 && h->screen_boxes && ds.n_entries < (ds.ordered ? kScreenMaxEntriesO : kScreenMaxEntries);
    if (screen) {
        a.screen = ds.screen.p;
        bool usable = ds.screen_usable;
        if (refit) {
            int32_t rc = make_screen(h, ds, ds.entries_refit.p, ds.screen_refit, &usable);
            if (rc != CR_OK) return rc;
            a.screen = ds.screen_refit.p;
        }
        if (!usable) { screen = false; a.screen = nullptr; }
    }
    // a SCREEN kernel stages screening records where the others stage wrappers
    const size_t screen_rec = ds.ordered ? sizeof(ScreenEntryO) : sizeof(ScreenEntry);
    w.screen = screen;
    w.lds_all_screen = whole_scene_layout(ds, screen_rec).end();
    set_tiles(a, (uint32_t)(c.W + 7) / 8u, (uint32_t)(c.H + 7) / 8u);
    a.work_counter = (uint32_t*)h->work_counter.p;
    a.counters = (uint64_t*)h->counters.p;
    a.out = (real*)d_out;
    a.uniform_kind = (ds.has_spheres && !ds.has_triangles) ? 0 : ((ds.has_triangles && !ds.has_spheres) ? 1 : -1);
    a.walk_exit_lanes = (uint32_t)(h->walk_exit_lanes >= 0 ? h->walk_exit_lanes : (ds.has_triangles ? 40 : 56));
    a.walk_round_steps = (uint32_t)(h->walk_round_steps >= 0 ? h->walk_round_steps : (ds.has_triangles ? 8 : 10));
    a.walk_leaf_min = mega ? (uint32_t)(h->walk_leaf_min >= 0 ? h->walk_leaf_min : 8) : 0u;   // the other pipelines test a leaf in the round that found it
    a.sg_on = 0; a.sg_lw = a.sg_lh = 3; set_groups(a, 0); a.sg_total = 0; a.sample_buf = nullptr;   // set by launch()

    // the ANIM kernels also carry the decode of leaves that hold a HitList element (pathtrace.hpp walk_round)
    w.anim = ds.animated || ds.has_leaf_runs;   // keyed primitives (the ANIM kernels also follow a keyed camera)
    // camera keys alone: the static kernels' CAMK variant, which also renders the batches of scenes without keys (the
    // static kernels do not carry a batch's frame arithmetic; with an unkeyed camera CAMK computes what they compute),
    // and for the same reason the regions of such scenes
    w.cam_keys = c.animated || frames != nullptr || region != nullptr;
    return CR_OK;
}

// One frame (call.frames == nullptr: params->frame), or the frames call.frames in one batch (cr_render_frames_*), or the
// pixels call.region of one frame (cr_render_region_*, whose entry has checked the sum order and the pipeline), or one frame
// to a noise target (cr_render_adaptive_*, whose entry has checked the same: call.adaptive, adaptive.hip), or a batch of
// frames to one (cr_render_adaptive_frames_*: call.adaptive with call.frames; a batch's rules hold, refit boxes among them).
template <typename real>
int32_t render_typed(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, void* d_out, CrStats* stats) {
    DevScene<real>* walk = nullptr;
    bool refit = false;
    int32_t rc = select_tree<real>(h, p, call.frames != nullptr, &walk, &refit);   // the base tree, or the frame's own (CR_REFIT_REBUILD)
    if (rc != CR_OK) return rc;
    DevScene<real>& ds = *walk;
    const int sum_order = resolve_sum_order(h, p);
    const bool fixed = p->output_sum == CR_OUTPUT_FIXED_SUM;
    if (fixed && (sum_order != CR_SUM_RELAXED || h->pipeline != 0))
        return fail(h, CR_ERR_UNSUPPORTED, "CR_OUTPUT_FIXED_SUM needs CR_SUM_RELAXED and the megakernel pipeline (a reference-order sum is sequential over samples)");
    if (call.frames) {
        if (call.views && refit)
            return fail(h, CR_ERR_UNSUPPORTED, "cr_render_views cannot refit boxes: refit boxes are per frame, a launch shares one set "
                                               "(render such views one at a time)");
        if (sum_order != CR_SUM_RELAXED || h->pipeline != 0)
            return fail(h, CR_ERR_UNSUPPORTED, "cr_render_frames needs CR_SUM_RELAXED and the megakernel pipeline (a reference-order sum is "
                                               "sequential over samples and would need a per-sample buffer per frame)");
        if (refit)
            return fail(h, CR_ERR_UNSUPPORTED, "cr_render_frames cannot refit boxes: refit boxes are per frame, a batch shares one set "
                                               "(render such frames one at a time)");
    }
    if (p->sample_count == 0) {
        // An empty shard (more ranks than samples): the sum of no samples, and 0 / samples for the mean, are both
        // zero -- cast_ray's loop body never runs (ray_casting.rs:82).  No kernel is launched.
        const size_t bytes = (size_t)call.n_frames * call.frame_bytes(cd, p);
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        HIP_TRY(h, hipMemsetAsync(d_out, 0, bytes, h->stream));
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        return stats ? finish_stats(h, stats, 0, ds.n_entries, 0) : CR_OK;
    }
    KernelArgs<real> a;
    WalkChoice w;
    FrameBatch<real> fb;
    std::vector<real> times;
    rc = prepare_args<real>(h, cd, p, call, ds, refit, h->pipeline == 0, d_out, times, a, w, fb);
    if (rc != CR_OK) return rc;
    if (call.adaptive) { fb.ad = call.adaptive; w.cam_keys = true; }   // the active-tile list lives where the region's offsets do: a scene without keys runs on CAMK
    dev_scene<real>(h).last_walk = walk != &dev_scene<real>(h) ? kWalkFrame : (refit ? kWalkRefit : kWalkBase);
    // relaxed sums exist in the megakernel; the alternative pipelines are reference-order cross-checks
    if (sum_order == CR_SUM_RELAXED && h->pipeline != 0) return fail(h, CR_ERR_UNSUPPORTED, "CR_SUM_RELAXED is implemented by the megakernel pipeline only");
    const bool relax = sum_order == CR_SUM_RELAXED;
    const size_t fx_need = relax ? fx_lds_bytes(MaxBlock<real>::value, 4) : 0;   // the relaxed sums' slots share the LDS
    w.screen_lds = w.screen && h->screen_lds && w.lds_all_screen + fx_need <= h->lds_limit;
    w.plain_lds = ds.lds_bytes + fx_need <= h->lds_limit;
    // cr_render_views_*: the kernels that read a camera record per view (render_views.hpp; relaxed sums, the megakernel)
    if (call.views) return ds.ordered ? views_ladder<real, true>(h, a, ds, w, stats, fb) : views_ladder<real, false>(h, a, ds, w, stats, fb);
    if (ds.ordered) {   // near-child-first walk: megakernel only
        if (h->pipeline != 0) return fail(h, CR_ERR_UNSUPPORTED, "CR_BVH_SAH_ORDERED is implemented by the megakernel pipeline only");
        return relax ? walk_ladder<real, true, true>(h, a, ds, w, stats, fb) : walk_ladder<real, true, false>(h, a, ds, w, stats, fb);
    }
    if (h->pipeline == 1) return render_wavefront<real>(h, a, ds, w.anim || w.cam_keys, stats);
    if (h->pipeline == 2) {   // the LDS-queue megakernel where it fits, else the plain megakernel below
        bool launched = false;
        rc = render_queue<real>(h, a, ds, w.anim || w.cam_keys, stats, &launched);
        if (launched || rc != CR_OK) return rc;
    }
    return relax ? walk_ladder<real, false, true>(h, a, ds, w, stats, fb) : walk_ladder<real, false, false>(h, a, ds, w, stats, fb);
}

template int32_t prepare_args<float>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, DevScene<float>&, bool, bool, void*, std::vector<float>&, KernelArgs<float>&, WalkChoice&, FrameBatch<float>&);
template int32_t prepare_args<double>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, DevScene<double>&, bool, bool, void*, std::vector<double>&, KernelArgs<double>&, WalkChoice&, FrameBatch<double>&);
template int32_t render_typed<float>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, void*, CrStats*);
template int32_t render_typed<double>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, void*, CrStats*);

}   // namespace cr
