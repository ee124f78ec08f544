// adaptive.hip -- the adaptive family behind cr_render_adaptive_*, cr_render_adaptive_frames_* and cr_render_adaptive_region_*
// (include/crucible_hip.h; the entry points are in api.hip): a frame, a batch of frames under one pass
// loop, or a region of a frame judged as if it were the frame, whose blocks of pixels stop taking samples once their two
// half-frame sums agree.  The family's argument checks, the pass loop around the render kernel that launch() (render.hpp)
// hands over, the judge kernel (one wave per block: the difference sum, the verdict, the next list of active tiles) and the
// finalize kernel (per-pixel means by each block's own sample count, the count plane).
#include "handle.hpp"
#include "adaptive.hpp"

namespace cr {

struct JudgeArgs {
    const unsigned long long* E;         // frame f's sums at f * frame_words, in both
    const unsigned long long* O;
    size_t frame_words;                  // W * H * 3
    int32_t W, H;                        // the pixels the passes cover: a region's own (its blocks and tiles start at its origin), else the frame's
    uint32_t block_log2, n_blocks;       // n_blocks: of one frame
    uint32_t n_frames;                   // the pass loop's frames: n_frames * n_blocks blocks, frame after frame (adaptive_batch_block)
    uint32_t lw, lh, tiles_x, tiles_y;   // the render kernel's tiles: their sides divide the block's
    double tolerance, scale12;           // scale12 = 2^(S - 12)
    uint32_t qp;                         // q * P: the samples in each half
    int32_t n;                           // samples per pixel taken so far (2 q P)
    int32_t* block_n;                    // per block of every frame: 0 while active, else the sample count it stopped at
    int32_t* next_list;                  // tiles of the blocks that stay active (batch-wide numbers), n_frames * tiles_x * tiles_y slots
    uint32_t* cursor;                    // slots of next_list in use: the active tiles the host reads back
};

// One wave per block.  An active block's D_b is an integer sum, so the order of the wave's reduction does not matter; a
// block that stays active appends its tiles to the next list at a range it takes from the one cursor (the order of the
// list varies from run to run; nothing observable depends on it).  A block sees its own frame's sums and nothing else, so
// its verdict does not depend on the frames it shares the launch with.
__global__ void __launch_bounds__(256) adaptive_judge_kernel(const JudgeArgs a) {
    const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (g >= a.n_frames * a.n_blocks) return;
    if (a.block_n[g] != 0) return;   // stopped earlier: final
    uint32_t f, b;
    adaptive_batch_block(g, a.n_blocks, f, b);
    const unsigned long long* const E = a.E + (size_t)f * a.frame_words;
    const unsigned long long* const O = a.O + (size_t)f * a.frame_words;
    uint32_t x0, y0, bw, bh;
    adaptive_block_rect(a.W, a.H, a.block_log2, b, x0, y0, bw, bh);
    const uint32_t row_words = bw * 3u, words = row_words * bh;
    unsigned long long d = 0;
    for (uint32_t k = lane; k < words; k += 64u) {
        const uint32_t row = k / row_words, col = k - row * row_words;
        const size_t i = ((size_t)(y0 + row) * (size_t)a.W + x0) * 3 + col;   // y0 + row < H, x0 * 3 + col < W * 3
        d += adaptive_term(E[i], O[i]);
    }
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (adaptive_stops(d, adaptive_threshold(a.tolerance, a.scale12, a.qp, bw * bh))) {
        if (lane == 0) a.block_n[g] = a.n;
        return;
    }
    // the block's tiles inside its frame's rows of the batch's tile grid
    uint32_t tx0, ty0, tw, th;
    adaptive_block_tiles(x0, y0, a.block_log2, a.lw, a.lh, a.tiles_x, a.tiles_y, tx0, ty0, tw, th);
    const uint32_t cnt = tw * th;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.cursor, cnt);
    base = (uint32_t)__shfl((int)base, 0);
    // the blocks partition each frame's tile grid, so base + cnt <= n_frames * tiles_x * tiles_y, the list's size
    for (uint32_t k = lane; k < cnt; k += 64u) a.next_list[base + k] = (int32_t)adaptive_block_tile(f, a.tiles_x, a.tiles_y, tx0, ty0, tw, k);
}

// ((mag(E) + mag(O)) * 2^-S) / n_b in fx_finalize_kernel's arithmetic, NaN where either flag is set; the count plane.
// n_frames frames, one after the other in E, O, out and counts; block_n holds n_blocks words per frame.
template <typename real>
__global__ void __launch_bounds__(256) adaptive_finalize_kernel(const unsigned long long* E, const unsigned long long* O, const int32_t* block_n,
                                                                real* out, int32_t* counts, int32_t W, int32_t H, uint32_t n_frames, uint32_t n_blocks,
                                                                uint32_t block_log2, int32_t samples, double inv_scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t frame_pix = (size_t)W * (size_t)H;
    if (i >= (size_t)n_frames * frame_pix * 3) return;
    const size_t gp = i / 3, f = gp / frame_pix;
    const uint32_t px = (uint32_t)(gp - f * frame_pix), y = px / (uint32_t)W, x = px - y * (uint32_t)W;
    const int32_t stopped = block_n[f * n_blocks + (y >> block_log2) * adaptive_blocks_x(W, block_log2) + (x >> block_log2)];
    const int32_t n = stopped ? stopped : samples;   // still active at the end: all of them
    const unsigned long long e = E[i], o = O[i];
    const unsigned long long m = (e & ~kFxNaN) + (o & ~kFxNaN);   // below 2^63: the sums of at most `samples` samples
    double s = ((double)(uint32_t)(m >> 32) * 4294967296.0 + (double)(uint32_t)m) * inv_scale;
    s = s / (double)n;
    if ((e | o) & kFxNaN) s = __builtin_nan("");
    out[i] = (real)s;
    if (counts && i == gp * 3) counts[gp] = n;
}

static int32_t elapsed_into(CrHandle* h, hipEvent_t a, hipEvent_t b, double& sum) {
    float ms = 0;
    HIP_TRY(h, hipEventSynchronize(b));
    HIP_TRY(h, hipEventElapsedTime(&ms, a, b));
    sum += ms;
    return CR_OK;
}

// what the pass loops of one call add up to (CrAdaptiveStats)
struct AdaptiveTotals {
    uint64_t samples = 0;
    int32_t passes = 0, blocks = 0, stopped = 0;
    double render_ms = 0, judge_ms = 0;
};

// One pass loop: frames [f0, f0 + fn) of the call, whose tiles fit one launch's work counter together.  The frames' sums
// live in the handle's accumulators (E of the fn frames, then O), their means go to the frames' slice of the output.
static int32_t adaptive_pass_loop(CrHandle* h, const AdaptiveRun& run, const AdaptiveFrame& fr, const AdaptivePass& pass, int32_t f0, int32_t fn,
                                  AdaptiveTotals& tot) {
    const uint32_t L = (uint32_t)run.block_log2;
    const int32_t P = run.pass_samples, S = fr.samples;
    const size_t frame_pix = (size_t)fr.W * (size_t)fr.H, frame_words = frame_pix * 3, words = (size_t)fn * frame_words;
    const uint32_t n_tiles = (uint32_t)fn * fr.tiles_x * fr.tiles_y;   // (fits: launch() sized the loop by the 32-bit work counter)
    const uint32_t frame_blocks = adaptive_blocks_x(fr.W, L) * adaptive_blocks_y(fr.H, L), n_blocks = (uint32_t)fn * frame_blocks;
    int32_t rc;
    unsigned long long* const E = (unsigned long long*)h->ad_acc.p;
    unsigned long long* const O = E + words;
    int32_t* const lists = (int32_t*)h->ad_lists.p;
    HIP_TRY(h, hipMemsetAsync(E, 0, 2 * words * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ad_block_n.p, 0, (size_t)n_blocks * sizeof(int32_t), h->stream));

    int exp2 = 0;
    (void)std::frexp(fr.fx_scale, &exp2);   // fx_scale = 2^(exp2 - 1)
    JudgeArgs ja;
    ja.E = E; ja.O = O; ja.frame_words = frame_words; ja.W = fr.W; ja.H = fr.H; ja.block_log2 = L; ja.n_blocks = frame_blocks; ja.n_frames = (uint32_t)fn;
    ja.lw = fr.lw; ja.lh = fr.lh; ja.tiles_x = fr.tiles_x; ja.tiles_y = fr.tiles_y;
    ja.tolerance = run.tolerance; ja.scale12 = std::ldexp(1.0, exp2 - 1 - 12);
    ja.block_n = (int32_t*)h->ad_block_n.p; ja.cursor = (uint32_t*)h->ad_ctrl.p;

    const int32_t* list = nullptr;   // the first passes render every tile, in order
    uint32_t active = n_tiles;
    int cur = 0;
    bool span_open = false;          // ev0 .. ev1 spans the render launches since the last judgement
    for (int32_t n = 0, q = 1; n < S && active > 0; q++) {
        if (!span_open) { HIP_TRY(h, hipEventRecord(h->ev0, h->stream)); span_open = true; }
        if ((rc = pass(f0, fn, list, active, n, n + P, E)) != CR_OK) return rc;
        if ((rc = pass(f0, fn, list, active, n + P, n + 2 * P, O)) != CR_OK) return rc;
        n += 2 * P; tot.passes += 2;
        if (n < run.min_samples || n >= S) continue;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        span_open = false;
        int32_t* const next = lists + (size_t)(cur ^ 1) * n_tiles;
        ja.qp = (uint32_t)q * (uint32_t)P; ja.n = n; ja.next_list = next;
        HIP_TRY(h, hipMemsetAsync(h->ad_ctrl.p, 0, 4, h->stream));
        HIP_TRY(h, hipEventRecord(h->ad_ev0, h->stream));
        hipLaunchKernelGGL(adaptive_judge_kernel, dim3((n_blocks + 3) / 4), dim3(256), 0, h->stream, ja);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(h->ad_ev1, h->stream));
        uint32_t left = 0;
        HIP_TRY(h, hipMemcpyAsync(&left, h->ad_ctrl.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (left > n_tiles) return fail(h, CR_ERR_HIP, "adaptive judge: more active tiles than the frames have");
        if ((rc = elapsed_into(h, h->ev0, h->ev1, tot.render_ms)) != CR_OK) return rc;
        if ((rc = elapsed_into(h, h->ad_ev0, h->ad_ev1, tot.judge_ms)) != CR_OK) return rc;
        list = next; cur ^= 1; active = left;
    }
    if (span_open) HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventRecord(h->ad_ev0, h->stream));
    const unsigned fin_grid = (unsigned)((words + 255) / 256);   // (E and O exist: 16 bytes per word, so far fewer than 2^39 words)
    const double inv_scale = 1.0 / fr.fx_scale;
    int32_t* const counts = run.d_counts ? run.d_counts + (size_t)f0 * frame_pix : nullptr;
    if (fr.f64) hipLaunchKernelGGL((adaptive_finalize_kernel<double>), dim3(fin_grid), dim3(256), 0, h->stream, E, O, ja.block_n,
                                   (double*)fr.out + (size_t)f0 * frame_words, counts, fr.W, fr.H, (uint32_t)fn, frame_blocks, L, S, inv_scale);
    else hipLaunchKernelGGL((adaptive_finalize_kernel<float>), dim3(fin_grid), dim3(256), 0, h->stream, E, O, ja.block_n,
                            (float*)fr.out + (size_t)f0 * frame_words, counts, fr.W, fr.H, (uint32_t)fn, frame_blocks, L, S, inv_scale);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ad_ev1, h->stream));
    std::vector<int32_t> block_n(n_blocks);
    HIP_TRY(h, hipMemcpyAsync(block_n.data(), h->ad_block_n.p, (size_t)n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (span_open && (rc = elapsed_into(h, h->ev0, h->ev1, tot.render_ms)) != CR_OK) return rc;
    if ((rc = elapsed_into(h, h->ad_ev0, h->ad_ev1, tot.judge_ms)) != CR_OK) return rc;
    for (uint32_t g = 0; g < n_blocks; g++) {
        uint32_t f, b, x0, y0, bw, bh;
        adaptive_batch_block(g, frame_blocks, f, b);
        adaptive_block_rect(fr.W, fr.H, L, b, x0, y0, bw, bh);
        tot.samples += (uint64_t)bw * bh * (uint64_t)(block_n[g] ? block_n[g] : S);
        tot.stopped += block_n[g] != 0;
    }
    tot.blocks += (int32_t)n_blocks;
    return CR_OK;
}

// The pass loops of one call: one over all frames where a pass over all their tiles fits the work counter
// (fr.frames_per_launch, launch()'s arithmetic), else consecutive ones over as many whole frames as do.
int32_t adaptive_passes(CrHandle* h, const AdaptiveRun& run, const AdaptiveFrame& fr, const AdaptivePass& pass) {
    const uint32_t L = (uint32_t)run.block_log2;
    if (fr.lw > L || fr.lh > L) return fail(h, CR_ERR_UNSUPPORTED, "the work tile does not divide the adaptive block");
    const int32_t cap = std::max(1, std::min(fr.frames_per_launch, fr.n_frames));   // frames per pass loop
    const size_t words = (size_t)cap * (size_t)fr.W * (size_t)fr.H * 3;
    const size_t n_tiles = (size_t)cap * fr.tiles_x * fr.tiles_y;
    const size_t n_blocks = (size_t)cap * adaptive_blocks_x(fr.W, L) * adaptive_blocks_y(fr.H, L);
    auto need = [&](DevBuf& buf, size_t bytes, const char* what) -> int32_t {
        const hipError_t e = buf.ensure(bytes);
        if (e == hipSuccess) return CR_OK;
        (void)hipGetLastError();
        return fail(h, CR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    int32_t rc;
    if ((rc = need(h->ad_acc, 2 * words * sizeof(unsigned long long), "adaptive accumulators")) != CR_OK) return rc;
    if ((rc = need(h->ad_lists, 2 * n_tiles * sizeof(int32_t), "adaptive tile lists")) != CR_OK) return rc;
    if ((rc = need(h->ad_block_n, n_blocks * sizeof(int32_t), "adaptive block counts")) != CR_OK) return rc;
    if ((rc = need(h->ad_ctrl, 16, "adaptive cursor")) != CR_OK) return rc;
    HIP_TRY(h, h->ad_ev0.create());
    HIP_TRY(h, h->ad_ev1.create());
    AdaptiveTotals tot;
    for (int32_t f0 = 0; f0 < fr.n_frames; f0 += cap)
        if ((rc = adaptive_pass_loop(h, run, fr, pass, f0, std::min(cap, fr.n_frames - f0), tot)) != CR_OK) return rc;
    if (!run.stats) return CR_OK;
    CrAdaptiveStats* st = run.stats;
    memset(st, 0, sizeof *st);
    // (the work counters add up over every launch of the call; finish_stats' time is the last run of passes only)
    if ((rc = finish_stats(h, &st->render, tot.samples, fr.n_entries, fr.scene_in_lds)) != CR_OK) return rc;
    st->render.kernel_ms = tot.render_ms;
    st->judge_ms = tot.judge_ms;
    st->passes = tot.passes; st->blocks = tot.blocks; st->blocks_stopped = tot.stopped;
    return CR_OK;
}

// The adaptive family's own checks, in the header's order, after validate_render's and before a batch's (api.hip
// validate_call); nothing has changed when one of them refuses
int32_t validate_adaptive(CrHandle* h, const CrRenderParams* p, const CrAdaptiveParams* ap, const void* out, const RenderCall& call) {
    if (!ap) return fail(h, CR_ERR_INVALID_ARG, "adaptive params are null");
    if (!out) return fail(h, CR_ERR_INVALID_ARG, "output buffer is null");
    if (ap->block_log2 != 0 && (ap->block_log2 < 3 || ap->block_log2 > 5)) return fail(h, CR_ERR_INVALID_ARG, "block_log2 must be 0, 3, 4 or 5");
    if (ap->_reserved != 0) return fail(h, CR_ERR_INVALID_ARG, "CrAdaptiveParams._reserved must be 0");
    if (ap->pass_samples < 1) return fail(h, CR_ERR_INVALID_ARG, "pass_samples must be at least 1");
    const int64_t pair = 2 * (int64_t)ap->pass_samples;
    if (p->samples % pair != 0) return fail(h, CR_ERR_INVALID_ARG, "samples must be a positive multiple of 2 * pass_samples");
    if (ap->min_samples < 1 || ap->min_samples % pair != 0) return fail(h, CR_ERR_INVALID_ARG, "min_samples must be a positive multiple of 2 * pass_samples");
    if (ap->min_samples > p->samples) return fail(h, CR_ERR_INVALID_ARG, "min_samples exceeds samples");
    if (!(ap->tolerance >= 0) || !std::isfinite(ap->tolerance)) return fail(h, CR_ERR_INVALID_ARG, "tolerance must be finite and not negative");
    if (resolve_sum_order(h, p) != CR_SUM_RELAXED || h->pipeline != 0)
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_adaptive needs CR_SUM_RELAXED and the megakernel pipeline (the two half-frame sums are relaxed "
                                           "sums; the active-tile list lives in the relaxed kernels)");
    if (p->sample_begin != 0 || p->sample_count != p->samples)
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_adaptive judges all samples of a pixel: sample_begin must be 0 and sample_count == samples");
    if (p->output_sum != 0) return fail(h, CR_ERR_UNSUPPORTED, "cr_render_adaptive writes means (output_sum 0)");
    // tiles must partition blocks: a work tile that CRUCIBLE_SG_TILE names and that is wider or taller than the block is
    // refused here, where the whole-frame calls give way to the default shape
    const int32_t L = ap->block_log2 ? ap->block_log2 : 4;
    if (call.region_call && (h->sg_lw > L || h->sg_lh > L))
        return fail(h, CR_ERR_UNSUPPORTED, "cr_render_adaptive_region: the work tile CRUCIBLE_SG_TILE names does not fit the adaptive block");
    return CR_OK;
}

}   // namespace cr
