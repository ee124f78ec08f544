// render.hpp -- the megakernel's host side for one precision and one sum order: launch() sets a pathtrace.hpp kernel up
// and runs it, launch_variant() picks the kernel kind and describes it to launch() (MegaKernel, handle.hpp), walk_ladder()
// turns the scene's residency (residency.hpp's rule, which the guide pass shares) into the kernel that stages it.  Included
// by the render_*.hip units only, each of which instantiates walk_ladder (both tree orders) for its <real, RELAX>, so the
// kernels of the four combinations compile side by side and no kernel is emitted twice.  launch() is a template over
// <real, RELAX> alone: a unit compiles it once, whatever the number of its kernels.  How a render is cut
// into launches -- tile, LDS, sample batches, frames per launch, grid, chunk -- is launch_plan.hpp's arithmetic (DESIGN.md
// 6.19), which a plain compiler checks; launch() keeps the HIP calls and the refusals' texts, in their order.
#pragma once
#include "handle.hpp"
#include "pathtrace.hpp"

#include <type_traits>

namespace cr {

template <typename real>
int32_t fx_finalize(CrHandle* h, const unsigned long long* sums, real* out, size_t n, double inv_scale, double count, int32_t output_sum) {
    hipLaunchKernelGGL((fx_finalize_kernel<real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sums, out, n, inv_scale, count, output_sum);
    HIP_TRY(h, hipGetLastError());
    return CR_OK;
}

#ifdef CR_DIAG
// a build with -DCR_DIAG: the launch's clocks and DG_ counters, one line on stderr per render that asks for stats
inline int32_t diag_dump(CrHandle* h, int block, uint32_t grid) {
    uint64_t d[64];
    HIP_TRY(h, hipMemcpy(d, h->counters.p, sizeof d, hipMemcpyDeviceToHost));
    const char* names[] = {"box_wave", "box_lane", "prim_wave", "prim_lane", "round_wave", "round_lane", "leafph_wave", "leafph_lane",
                           "shade_wave", "shade_lane", "lamb_lane", "metal_lane", "diel_lane", "sky_lane", "ruv_wave", "ruv_lane",
                           "regen_wave", "regen_lane", "outer_wave", "unwind_wave", "unwind_lane", "hitsh_wave", "hitsh_lane", "band_wave", "band_lane",
                           "root2_wave", "root2_lane", "quot_wave", "quot_lane", "quotdiv_wave", "quotdiv_lane"};
    static_assert(sizeof names / sizeof names[0] == DG_N, "one name per DG_ counter");
    fprintf(stderr, "[diag] block=%d grid=%u clk_regen=%llu clk_trace=%llu clk_shade=%llu clk_total=%llu", block, grid,
            (unsigned long long)d[9], (unsigned long long)d[10], (unsigned long long)d[11], (unsigned long long)d[12]);
    for (int i = 0; i < DG_N; i++) fprintf(stderr, " %s=%llu", names[i], (unsigned long long)d[16 + i]);
    fprintf(stderr, "\n");
    return CR_OK;
}
#endif

// the frames [f0, f0 + fn) of a batch as one launch's: their count and where their ray times start (a single render: its own)
template <typename real>
void set_frame_slice(KernelArgs<real>& args, const KernelArgs<real>& args_in, const FrameBatch<real>& fb, int32_t f0, int32_t fn) {
    args.n_frames = (uint32_t)fn;
    args.current_time = fb.times ? fb.times[f0] : args_in.current_time;
    args.frame_times = fb.d_times ? fb.d_times + f0 : nullptr;
}

// One launch routine per unit.  What it depends on in the kernel it runs is MegaKernel's fields (handle.hpp), filled by
// launch_variant below; the sum order alone stays a template parameter, because the two orders run different finalize
// kernels and a unit may name only its own.  k.list: the passes of cr_render_adaptive_* -- pathtrace_kernel_listed, handed
// to adaptive_passes (adaptive.hip).
// The sequence: plan the tile; attribute and pick_block; what the kernel kind renders; plan the samples and frames; the buffers
// and memsets; per frame slice and batch, the arguments from the plan and the launch; finalize; stats.
template <typename real, bool RELAX>
int32_t launch(CrHandle* h, const MegaKernel<real>& k, const KernelArgs<real>& args_in, size_t scene_lds_bytes, CrStats* stats, const FrameBatch<real>& fb) {
    KernelArgs<real> args = args_in;
    // A render whose caller asked for no stats runs the kernel that keeps no work counters, where one exists (k.quiet: the
    // headline's kernel, never in a CR_DIAG build, which counts every launch); adaptive calls and batches of frames run on
    // kernels with keys, which all count; keep_counters: a group's member.
    const bool quiet = k.quiet && !stats && !h->keep_counters && !fb.ad && fb.n == 1;
    void (*const kern)(const KernelArgs<real>) = quiet ? k.quiet : k.kern;
    const int max_block = k.latency ? LatencyBlock : MaxBlock<real>::value;
    // the samples of one launch (cr_render_adaptive_*: one pass of pass_samples samples) and of the launch's pixels: the region's
    // (prepare_args: the whole frame unless cr_render_region_* named one; RELAX kernels with keys only)
    const int32_t s_begin = args.sample_begin, s_end = fb.ad ? s_begin + fb.ad->pass_samples : args.sample_end;
    const bool fixed = args.output_sum == CR_OUTPUT_FIXED_SUM;
    const TilePlan tile = plan_tile(h->sg_lw, h->sg_lh, s_end - s_begin, fb.ad ? fb.ad->block_log2 : -1, RELAX, k.res, scene_lds_bytes, max_block);
    const bool use_lds = tile.use_lds;
    args.fx_lds_off = (uint32_t)tile.fx_off;
    if (use_lds) HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile.lds_bytes(max_block)));
    int block = 256, per_cu = 1;   // an override above max_block is ignored here (the latency entry point's 512 under CRUCIBLE_BLOCK=1024)
    { int32_t rc = pick_block(h, (const void*)kern, max_block, true, tile.lds_base, tile.lds_per_wave, "kernel does not fit on a CU", block, per_cu); if (rc != CR_OK) return rc; }
    const size_t lds_bytes = tile.lds_bytes(block);
    args.n_frames = 1; args.frame_times = nullptr;
    switch (check_call_shape(RELAX, k.keyed, k.latency, k.list, fb.n, whole_frame(args.reg_x0, args.reg_y0, args.reg_w, args.reg_h, args.cam.W, args.cam.H), fb.ad != nullptr)) {
    case kShapeOneFrame: return fail(h, CR_ERR_UNSUPPORTED, "this kernel variant renders one frame per launch");
    case kShapeWholeFrames: return fail(h, CR_ERR_UNSUPPORTED, "this kernel variant renders whole frames");
    case kShapeNoList: return fail(h, CR_ERR_UNSUPPORTED, "this kernel variant does not carry the active-tile list");
    case kShapeOk: break;
    }
    // Sample-granular mode: batches of samples; each batch is one launch of the path tracer, in the reference order followed
    // by the ordered sum (sg_finalize_kernel) over the colours it left in the buffer
    const SampleQuery sq = {RELAX, h->sample_granular != 0, s_begin, s_end, args.reg_w, args.reg_h, sizeof(real), h->sample_buf_limit, h->work_counter_max, tile.lw, tile.lh,
                            h->sg_lw >= 0, fb.n, fb.ad != nullptr, fb.ad && fb.ad->split_passes, fixed, args_in.tiles_x, args_in.tiles_y};
    SamplePlan sp = plan_samples(sq);
    if constexpr (RELAX) {   // (the reference order's plan refuses nothing: it falls back)
        if (sp.refusal == kPlanCounter) return fail(h, CR_ERR_UNSUPPORTED, "image too large for the 32-bit work counter");
        if (sp.refusal == kPlanCounterPass) return fail(h, CR_ERR_UNSUPPORTED, "image too large for the 32-bit work counter at this pass_samples");
        if (sp.fx_acc_bytes) {
            const hipError_t e = h->fx_acc.ensure(sp.fx_acc_bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, CR_ERR_HIP, "fixed-point sums of " + std::to_string(fb.n) + " frame(s): " + hipGetErrorString(e));
            }
        }
    } else {   // a buffer that cannot be had: a lane owns a pixel
        if (sp.sample_buf_bytes && h->sample_buf.ensure(sp.sample_buf_bytes) != hipSuccess) { (void)hipGetLastError(); lane_owns_pixel(sp); }
        if (sp.sg_acc_bytes && h->sg_acc.ensure(sp.sg_acc_bytes) != hipSuccess) { (void)hipGetLastError(); lane_owns_pixel(sp); }
    }
    if (sp.tiled) { args.sg_lw = (uint32_t)sp.lw; args.sg_lh = (uint32_t)sp.lh; }
    set_tiles(args, sp.tiles_x, sp.tiles_y);
    args.sg_on = sp.batch > 0 ? 1u : 0u;
    const int32_t batch = sp.batch, fpl = sp.fpl;   // (the plan as numbers: the closures below keep these, not the plan)
    const uint32_t ns = sp.ns;
    const uint64_t frame_tiles = sp.tiles();
    const size_t frame_words = sp.frame_words;
    const GridPlan gp = plan_grid(h->n_cus, per_cu, sp.grid_work(s_end - s_begin), block, 1);
    const uint32_t grid = gp.blocks;
    args.n_threads = gp.n_threads;
    if constexpr (!RELAX) {
        HIP_TRY(h, h->att_stack.ensure(att_stack_bytes(args.max_depth, args.n_threads, sizeof(real))));
        args.att_stack = (real*)h->att_stack.p;
    } else {
        // the scale of the n samples a pixel receives in this render; CR_OUTPUT_FIXED_SUM: the sums go straight into the caller's buffer
        args.fx_scale = fx_scale_for(fx_scale_samples(fixed, fb.ad != nullptr, args.samples_total, s_begin, s_end));
        args.fx_acc = fixed ? (unsigned long long*)args.out : (unsigned long long*)h->fx_acc.p;
        if (!fb.ad) HIP_TRY(h, hipMemsetAsync(args.fx_acc, 0, sp.fx_words * sizeof(unsigned long long), h->stream));
    }
    if (!quiet) HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, 64 * sizeof(uint64_t), h->stream));
    // one launch of the kernel on `args` as they stand: the work counter starts at zero
    auto run = [&](uint32_t blocks) -> int32_t {
        HIP_TRY(h, hipMemsetAsync(h->work_counter.p, 0, 4, h->stream));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(block), use_lds ? lds_bytes : 0, h->stream, args);
        HIP_TRY(h, hipGetLastError());
        return CR_OK;
    };
    // one batch of samples [b0, b1) of fn frames of `tiles` tiles, as plan_batch sizes it
    auto run_batch = [&](int32_t b0, int32_t b1, uint64_t tiles, int32_t fn, bool fit) -> int32_t {
        const BatchLaunch bl = plan_batch(ns, b1 - b0, tiles, fn, fit, grid, block, h->sg_chunk_override);
        args.sample_begin = b0; args.sample_end = b1;
        set_groups(args, bl.groups);
        args.sg_total = bl.sg_total;
        args.sg_chunk = bl.chunk;
        return run(bl.blocks);
    };
    if (k.list) {
        // cr_render_adaptive_*: the passes are adaptive_passes' (adaptive.hip), each one a launch of this kernel over the tiles
        // it names, into the accumulator it names; the counters add up over the passes
        if (!args.sg_on) return fail(h, CR_ERR_UNSUPPORTED, "image too large for the 32-bit work counter");
        h->last_block = block; h->last_grid = (int)grid;
        // (cr_render_adaptive_frames_*: a pass loop's frames [f0, f0 + fn) of the batch, at most fpl, as the loop below sets them)
        const AdaptivePass pass = [&](int32_t f0, int32_t fn, const int32_t* tile_list, uint32_t n_tiles, int32_t s0, int32_t s1, unsigned long long* acc) -> int32_t {
            args.tile_list = tile_list; args.fx_acc = acc;
            set_frame_slice(args, args_in, fb, f0, fn);
            // one launch, unless the work counter holds fewer samples of the tiles than the pass has (split_passes; batch >= 1)
            for (int64_t b0 = s0; b0 < s1; b0 += batch) {
                const int32_t rc = run_batch((int32_t)b0, batch_end(b0, batch, s1), n_tiles, 1, true);   // (the list's tiles are the batch's, of all its frames)
                if (rc != CR_OK) return rc;
            }
            return CR_OK;
        };
        // (the pass loop judges the launch's pixels: a region's blocks and tiles share its origin)
        const AdaptiveFrame fr = {(int32_t)args.reg_w, (int32_t)args.reg_h, args.samples_total, fb.n, fpl, args.sg_lw, args.sg_lh, args.tiles_x, args.tiles_y, args.fx_scale,
                                  (void*)args.out, std::is_same<real, double>::value, args.n_entries, k.res};
        return adaptive_passes(h, *fb.ad, fr, pass);
    }
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (!args.sg_on) {
        int32_t rc = run(grid);
        if (rc != CR_OK) return rc;
    } else {
        args.sample_buf = (real*)h->sample_buf.p;
        unsigned long long* const fx_frame0 = args.fx_acc;
        const CamConst<real>* const views0 = args.views;   // cr_render_views_*: a frame is a view, its camera record travels with it
        for (int32_t f0 = 0; f0 < fb.n; f0 += fpl) {   // one pass for a single render
            const int32_t fn = std::min(fpl, fb.n - f0);
            if constexpr (RELAX) {   // frames [f0, f0 + fn) of a batch
                set_frame_slice(args, args_in, fb, f0, fn);
                args.fx_acc = fx_frame0 + (size_t)f0 * frame_words;
                if (views0) args.views = views0 + f0;
            }
            for (int64_t b0 = s_begin; b0 < s_end; b0 += batch) {   // (64 bits: b0 + batch may pass INT32_MAX)
                const int32_t b1 = batch_end(b0, batch, s_end);
                { int32_t rc = run_batch((int32_t)b0, b1, frame_tiles, fn, false); if (rc != CR_OK) return rc; }
                if constexpr (!RELAX) {   // (relaxed: the sums stay in fx_acc until the last batch)
                    hipLaunchKernelGGL((sg_finalize_kernel<real>), dim3((unsigned)((sp.tile_pixels() + 255) / 256)), dim3(256), 0, h->stream, args,
                                       (real*)h->sg_acc.p, b1 - (int32_t)b0, b0 == s_begin ? 1 : 0, b1 == s_end ? 1 : 0);
                    HIP_TRY(h, hipGetLastError());
                }
            }
        }
        if constexpr (RELAX) if (!fixed) {   // a batch's frames follow each other in fx_acc and in the output
            int32_t rc = fx_finalize<real>(h, (const unsigned long long*)h->fx_acc.p, args.out, sp.fx_words, 1.0 / args.fx_scale, (double)args.samples_total, args.output_sum);
            if (rc != CR_OK) return rc;
        }
        args.sample_begin = s_begin; args.sample_end = s_end;
    }
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->last_block = block; h->last_grid = (int)grid;
    if (stats) {
        int32_t rc = finish_stats(h, stats, (uint64_t)sp.npix * (uint64_t)(args.sample_end - args.sample_begin) * (uint64_t)fb.n, args.n_entries, k.res);
        if (rc != CR_OK) return rc;
#ifdef CR_DIAG
        rc = diag_dump(h, block, grid);
        if (rc != CR_OK) return rc;
#endif
    }
    return CR_OK;
}

// Picks the kernel kind: keyed primitives (ANIM), camera keys alone (CAMK) or neither.  The ANIM kernels follow a keyed
// camera themselves, so ANIM with CAMK is never instantiated.
// The one place that names the kernels: `on` describes the kernel of <ANIM, CAMK, LIST> to launch() and runs it.
template <typename real, int RES, bool ORD, bool LATENCY, bool RELAX, bool SCREEN = false>
int32_t launch_variant(CrHandle* h, const KernelArgs<real>& a, size_t lds_bytes, CrStats* stats, const WalkChoice& w, const FrameBatch<real>& fb) {
    static_assert(!LATENCY || RES == RES_TOP, "the 6-waves-per-SIMD entry point exists for RES_TOP only");
    using yes = std::true_type;
    using no = std::false_type;
    auto on = [&](auto anim, auto camk, auto list) {
        constexpr bool ANIM = decltype(anim)::value, CAMK = decltype(camk)::value, LIST = decltype(list)::value;
        static_assert(!LIST || (RELAX && ANIM != CAMK && !LATENCY), "the listed kernels are relaxed kernels with keys");
        // (pathtrace_kernel is named whatever the kind, and first: a unit emits its kernels in the order it first names them,
        // and the code the compiler makes of a kernel depends on that order -- scripts/isa_diff.py shows it)
        MegaKernel<real> k = {pathtrace_kernel<real, RES, ANIM, ORD, CAMK, RELAX, SCREEN>, nullptr, RES, ANIM || CAMK, LATENCY, LIST};
        if constexpr (LATENCY) k.kern = pathtrace_kernel_latency<real, ANIM, ORD, CAMK, RELAX>;
        if constexpr (LIST) k.kern = pathtrace_kernel_listed<real, RES, ANIM, ORD, CAMK, SCREEN>;
#ifndef CR_DIAG
        // the twin that keeps no work counters: of the static f64 relaxed SCREEN kernel on an unordered tree with the scene in LDS
        // (two conditions: what this function's parameters decide is settled before the lambda's own, so no f32 unit meets the f64 twin)
        if constexpr (std::is_same<real, double>::value && RES == RES_LDS && !ORD && !LATENCY && RELAX && SCREEN)
            if constexpr (!ANIM && !CAMK && !LIST) k.quiet = pathtrace_kernel_quiet<RES>;
#endif
        return launch<real, RELAX>(h, k, a, lds_bytes, stats, fb);
    };
    if (fb.ad) {   // cr_render_adaptive_*: the listed kernels (a scene without keys on the camera-key one)
        if constexpr (RELAX && !LATENCY) return w.anim ? on(yes{}, no{}, yes{}) : on(no{}, yes{}, yes{});
        else return fail(h, CR_ERR_UNSUPPORTED, "this kernel variant does not carry the active-tile list");
    }
    if (w.anim) return on(yes{}, no{}, no{});
    if (w.cam_keys) return on(no{}, yes{}, no{});
    return on(no{}, no{}, no{});
}

// The residency ladder: residency.hpp's rule settles the residency, the window and whether the walk runs on screening
// records (the whole scene in LDS, else a window of the tree's top there, else everything through L2); this is its answer
// as a kernel.  ORD: the near-child-first walk over EntryO / ScreenEntryO records.
template <typename real, bool ORD, bool RELAX>
int32_t walk_ladder(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, CrStats* stats, const FrameBatch<real>& fb) {
    constexpr bool f32 = std::is_same<real, float>::value;   // the double kernel needs far more than 80 VGPRs: it halves there
    ResidencyQuery q = residency_query<real, ORD>(h, ds, w);
    // (the 6-waves-per-SIMD kernels render whole frames: a region of such a tree runs on the regular kernel, the same bytes)
    q.whole_frame = whole_frame(a.reg_x0, a.reg_y0, a.reg_w, a.reg_h, a.cam.W, a.cam.H);
    q.adaptive = fb.ad != nullptr;
    const Residency r = choose_residency(q);
    a.lds_entries = r.lds_entries;
    if (r.lds_side) a.lds_side = 1;
    if (r.clear_screen) a.screen = nullptr;
    return residency_dispatch<!(ORD && f32), f32>(r, [&](auto res, auto screen, auto latency) {
        return launch_variant<real, decltype(res)::value, ORD, decltype(latency)::value, RELAX, decltype(screen)::value>(h, a, r.lds_bytes, stats, w, fb);
    });
}

// a unit's instantiations: the ladders of both tree orders, and with them every kernel of <real, RELAX>
#define CR_RENDER_UNIT(real, RELAX)                                                                                                                            \
    template int32_t cr::walk_ladder<real, false, RELAX>(CrHandle*, KernelArgs<real>&, const DevScene<real>&, const WalkChoice&, CrStats*, const FrameBatch<real>&); \
    template int32_t cr::walk_ladder<real, true, RELAX>(CrHandle*, KernelArgs<real>&, const DevScene<real>&, const WalkChoice&, CrStats*, const FrameBatch<real>&);

}   // namespace cr
