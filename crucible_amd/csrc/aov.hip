// aov.hip -- the guide pass behind cr_render_aov_* and cr_render_aov_frames_*: first-hit albedo, normal, depth and coverage per pixel (aov.hpp has the
// accumulator layout, include/crucible_hip.h the definition of every layer).  aov_typed sets a launch up through the
// render's own prepare_args (camera-key slot, ray times, refitted boxes, screening records: render.hip), runs the first-hit
// kernel of the scene's residency (aov_f32.hip / aov_f64.hip) and turns the accumulators into the requested planes.
#include "aov.hpp"

namespace cr {

// The accumulators of pixel i into the planes that were asked for, in ascending bit order.  A sum becomes a real as
// fx_finalize_kernel turns a relaxed sum into one -- the word's magnitude in two exact halves, one rounding in their add,
// times 2^-S, divided by the frame's sample count unless the shard's sum is asked for -- with the word's sign put back;
// a flagged channel is NaN.  Depth: the complement of the largest word, +inf where no sample hit.
// blockIdx.y: the frame of a batch, whose planes begin frame_reals reals after the previous frame's.
// COUNTS (aov_counts_finalize_kernel): the divisor is the pixel's own clamped count, `count` the clamp's maximum; a pixel
// without samples is not divided (aov_counts.hpp) -- its sums are zero and stay +0.0, its depth +inf.
template <typename real, bool COUNTS>
CR_D void aov_finalize_pixel(const unsigned long long* acc, const uint32_t* flags, real* out, size_t npix, int32_t layers,
                             double inv_scale, double count, int32_t output_sum, size_t frame_reals, const int32_t* counts) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    acc += (size_t)blockIdx.y * npix * kAovWords;
    flags += (size_t)blockIdx.y * npix;
    out += (size_t)blockIdx.y * frame_reals;
    bool divide = !output_sum;
    if constexpr (COUNTS) {
        const uint32_t n_p = aov_count_clamp(counts[(size_t)blockIdx.y * npix + i], (int32_t)count);
        divide = aov_count_divides(n_p, output_sum);
        count = (double)n_p;
    }
    const unsigned long long* w = acc + i * kAovWords;
    const uint32_t bad = flags[i];
    auto value = [&](uint32_t c) -> real {
        const long long v = (long long)w[c];
        const unsigned long long m = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        double s = ((double)(uint32_t)(m >> 32) * 4294967296.0 + (double)(uint32_t)m) * inv_scale;
        if (divide) s = s / count;
        if (v < 0) s = -s;
        if ((bad >> c) & 1u) s = __builtin_nan("");
        return (real)s;
    };
    real* o = out;
    if (layers & CR_AOV_ALBEDO) { for (uint32_t c = 0; c < 3; c++) o[i * 3 + c] = value(c); o += npix * 3; }
    if (layers & CR_AOV_NORMAL) { for (uint32_t c = 0; c < 3; c++) o[i * 3 + c] = value(3 + c); o += npix * 3; }
    if (layers & CR_AOV_DEPTH) {
        const unsigned long long d = w[kAovDepth];
        real r = r_inf(real(0));
        if (d) {
            if constexpr (sizeof(real) == 8) r = __builtin_bit_cast(double, ~d);
            else r = __builtin_bit_cast(float, (uint32_t)~d);
        }
        o[i] = r;
        o += npix;
    }
    if (layers & CR_AOV_COVERAGE) o[i] = value(kAovCoverage);
}

template <typename real>
__global__ void __launch_bounds__(256) aov_finalize_kernel(const unsigned long long* acc, const uint32_t* flags, real* out, size_t npix, int32_t layers,
                                                           double inv_scale, double count, int32_t output_sum, size_t frame_reals) {
    aov_finalize_pixel<real, false>(acc, flags, out, npix, layers, inv_scale, count, output_sum, frame_reals, nullptr);
}

template <typename real>
__global__ void __launch_bounds__(256) aov_counts_finalize_kernel(const unsigned long long* acc, const uint32_t* flags, real* out, size_t npix, int32_t layers,
                                                                  double inv_scale, double count, int32_t output_sum, size_t frame_reals,
                                                                  const int32_t* counts) {
    aov_finalize_pixel<real, true>(acc, flags, out, npix, layers, inv_scale, count, output_sum, frame_reals, counts);
}

// One frame (call.frames == nullptr: params->frame), or the frames call.frames in one batch (cr_render_aov_frames_*):
// the batch's frames lie one behind the other in the accumulators, in the flags and in the output.  call.region: the pixels
// of the one frame that the pass covers (cr_render_aov_region_*) -- accumulators, flags and planes are then the region's
// size, and the pass runs as a batch of one frame on the BATCH kernels, which carry the region's offsets.
// call.counts (cr_render_aov_counts_*; device memory): the samples each pixel takes -- the COUNTS kernels, which are BATCH
// kernels, so one frame runs as a batch of one; the finalize divides by the pixel's count, and stats->samples is the
// kernel's own count of the primary rays it cast, since the host does not see the plane.
// call.views (cr_render_aov_views_*): a batch whose frame k is seen through call.views[k] -- the VIEWS kernels, which are
// BATCH kernels; prepare_args has packed the views' records and keys.
template <typename real>
int32_t aov_typed(CrHandle* h, const CrCameraDesc* cd, const CrRenderParams* p, const RenderCall& call, void* d_out, CrStats* stats) {
    const int32_t* const frames = call.frames;
    const CrRegion* const region = call.region;
    const int32_t n_frames = call.n_frames, layers = call.layers;
    DevScene<real>* walk = nullptr;
    bool refit = false;
    int32_t rc = select_tree<real>(h, p, frames != nullptr, &walk, &refit);   // as a render decides it
    if (rc != CR_OK) return rc;
    if (call.views && refit)
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_aov_views cannot refit boxes: refit boxes are per frame, a launch shares one set "
                                           "(render such views one at a time)");
    if (frames && refit)
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_frames cannot refit boxes: refit boxes are per frame, a batch shares one set "
                                           "(render such frames one at a time)");
    DevScene<real>& ds = *walk;
    const size_t frame_pix = call.frame_pixels(cd);
    const size_t npix = frame_pix * (size_t)n_frames;   // (at most 2^26 * 2^31: the byte counts below fit in 64 bits)
    hipError_t e = h->aov_acc.ensure(npix * kAovWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = h->aov_flags.ensure(npix * sizeof(uint32_t));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("guide accumulators: ") + hipGetErrorString(e)); }
    AovArgs<real> a;
    memset(&a, 0, sizeof a);
    WalkChoice w;
    int res = 0;
    if (p->sample_count > 0) {   // (an empty shard: no kernel, sums of nothing and no hit)
        FrameBatch<real> fb;
        std::vector<real> times;
        // the walk is the megakernel's under every pipeline setting: the cross-check pipelines have no guide pass of their own
        rc = prepare_args<real>(h, cd, p, call, ds, refit, true, d_out, times, a.k, w, fb);
        if (rc != CR_OK) return rc;
        if (region || (call.counts && !frames)) {   // the BATCH kernels read a frame's first ray time from the device's table
            rc = stage_frame_times(h, &a.k.current_time, sizeof(real));
            if (rc != CR_OK) return rc;
        }
        dev_scene<real>(h).last_walk = walk != &dev_scene<real>(h) ? kWalkFrame : (refit ? kWalkRefit : kWalkBase);
        set_tiles(a.k, (a.k.reg_w + 3u) >> 2, (a.k.reg_h + 3u) >> 2);
        a.k.fx_scale = fx_scale_for(p->samples);   // of the whole frame, so that the words of shards add up
        a.acc = (unsigned long long*)h->aov_acc.p; a.flags = (uint32_t*)h->aov_flags.p;
        a.layers = layers;
        a.groups = ((uint32_t)p->sample_count + 3u) >> 2;
        if (frames) { a.n_frames = (uint32_t)n_frames; a.frame_times = fb.d_times; }
        else if (region || call.counts) { a.n_frames = 1u; a.frame_times = (const real*)h->times_dev.p; }
        a.counts = call.counts;
        const size_t need = aov_lds_bytes(MaxBlock<real>::value);   // the waves' slots share the LDS
        w.screen_lds = w.screen && h->screen_lds && w.lds_all_screen + need <= h->lds_limit;
        w.plain_lds = ds.lds_bytes + need <= h->lds_limit;
    }
    HIP_TRY(h, hipMemsetAsync(h->aov_acc.p, 0, npix * kAovWords * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->aov_flags.p, 0, npix * sizeof(uint32_t), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, 64 * sizeof(uint64_t), h->stream));
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (p->sample_count > 0) {
        rc = call.views ? aov_views_ladder<real>(h, a, ds, w, &res) : (call.counts ? aov_counts_ladder<real>(h, a, ds, w, &res) : aov_ladder<real>(h, a, ds, w, &res));
        if (rc != CR_OK) return rc;
    }
    const size_t frame_reals = frame_pix * call.layer_channels();
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += 65535) {   // (a grid has at most 65535 rows)
        const size_t fn = std::min<size_t>(65535, (size_t)n_frames - f0);
        const dim3 grid((unsigned)((frame_pix + 255) / 256), (unsigned)fn);
        const unsigned long long* const acc = (const unsigned long long*)h->aov_acc.p + f0 * frame_pix * kAovWords;
        const uint32_t* const flags = (const uint32_t*)h->aov_flags.p + f0 * frame_pix;
        if (call.counts)
            hipLaunchKernelGGL((aov_counts_finalize_kernel<real>), grid, dim3(256), 0, h->stream, acc, flags, (real*)d_out + f0 * frame_reals, frame_pix, layers,
                               1.0 / fx_scale_for(p->samples), (double)p->samples, p->output_sum, frame_reals, call.counts + f0 * frame_pix);
        else
            hipLaunchKernelGGL((aov_finalize_kernel<real>), grid, dim3(256), 0, h->stream, acc, flags, (real*)d_out + f0 * frame_reals, frame_pix, layers,
                               1.0 / fx_scale_for(p->samples), (double)p->samples, p->output_sum, frame_reals);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    if (!stats) return CR_OK;
    rc = finish_stats(h, stats, (uint64_t)npix * (uint64_t)p->sample_count, ds.n_entries, res);
    if (rc == CR_OK && call.counts) stats->samples = stats->segments;   // the sum of the clamped counts, as the kernel counted it
    return rc;
}

template int32_t aov_typed<float>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, void*, CrStats*);
template int32_t aov_typed<double>(CrHandle*, const CrCameraDesc*, const CrRenderParams*, const RenderCall&, void*, CrStats*);

}   // namespace cr
