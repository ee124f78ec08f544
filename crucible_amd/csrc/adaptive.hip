// adaptive.hip -- cr_render_adaptive_* (include/crucible_hip.h): a frame whose blocks of pixels stop taking
// samples once their two half-frame sums agree.  The entry points' checks, the pass loop around the render kernel that
// launch() (render.hpp) hands over, the judge kernel (one wave per block: the difference sum, the verdict, the next list
// of active tiles) and the finalize kernel (per-pixel means by each block's own sample count, the count plane).
#include "handle.hpp"
#include "adaptive.hpp"

namespace cr {

struct JudgeArgs {
    const unsigned long long* E;
    const unsigned long long* O;
    int32_t W, H;
    uint32_t block_log2, n_blocks;
    uint32_t lw, lh, tiles_x, tiles_y;   // the render kernel's tiles: their sides divide the block's
    double tolerance, scale12;           // scale12 = 2^(S - 12)
    uint32_t qp;                         // q * P: the samples in each half
    int32_t n;                           // samples per pixel taken so far (2 q P)
    int32_t* block_n;                    // per block: 0 while active, else the sample count it stopped at
    int32_t* next_list;                  // tiles of the blocks that stay active, tiles_x * tiles_y slots
    uint32_t* cursor;                    // slots of next_list in use: the active tiles the host reads back
};

// One wave per block.  An active block's D_b is an integer sum, so the order of the wave's reduction does not matter; a
// block that stays active appends its tiles to the next list at a range it takes from the one cursor (the order of the
// list varies from run to run; nothing observable depends on it).
__global__ void __launch_bounds__(256) adaptive_judge_kernel(const JudgeArgs a) {
    const uint32_t b = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (b >= a.n_blocks) return;
    if (a.block_n[b] != 0) return;   // stopped earlier: final
    uint32_t x0, y0, bw, bh;
    adaptive_block_rect(a.W, a.H, a.block_log2, b, x0, y0, bw, bh);
    const uint32_t row_words = bw * 3u, words = row_words * bh;
    unsigned long long d = 0;
    for (uint32_t k = lane; k < words; k += 64u) {
        const uint32_t row = k / row_words, col = k - row * row_words;
        const size_t i = ((size_t)(y0 + row) * (size_t)a.W + x0) * 3 + col;   // y0 + row < H, x0 * 3 + col < W * 3
        d += adaptive_term(a.E[i], a.O[i]);
    }
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (adaptive_stops(d, adaptive_threshold(a.tolerance, a.scale12, a.qp, bw * bh))) {
        if (lane == 0) a.block_n[b] = a.n;
        return;
    }
    // the block's tiles inside the frame's tile grid (blocks and tiles are both anchored at pixel (0, 0))
    const uint32_t tx0 = x0 >> a.lw, ty0 = y0 >> a.lh, B = 1u << a.block_log2;
    const uint32_t tw = min(B >> a.lw, a.tiles_x - tx0), th = min(B >> a.lh, a.tiles_y - ty0), cnt = tw * th;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.cursor, cnt);
    base = (uint32_t)__shfl((int)base, 0);
    // the blocks partition the tile grid, so base + cnt <= tiles_x * tiles_y, the list's size
    for (uint32_t k = lane; k < cnt; k += 64u) {
        const uint32_t r = k / tw;
        a.next_list[base + k] = (int32_t)((ty0 + r) * a.tiles_x + tx0 + (k - r * tw));
    }
}

// ((mag(E) + mag(O)) * 2^-S) / n_b in fx_finalize_kernel's arithmetic, NaN where either flag is set; the count plane.
template <typename real>
__global__ void __launch_bounds__(256) adaptive_finalize_kernel(const unsigned long long* E, const unsigned long long* O, const int32_t* block_n,
                                                                real* out, int32_t* counts, int32_t W, int32_t H, uint32_t block_log2,
                                                                int32_t samples, double inv_scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)W * (size_t)H * 3) return;
    const uint32_t px = (uint32_t)(i / 3), y = px / (uint32_t)W, x = px - y * (uint32_t)W;
    const int32_t stopped = block_n[(y >> block_log2) * adaptive_blocks_x(W, block_log2) + (x >> block_log2)];
    const int32_t n = stopped ? stopped : samples;   // still active at the end: all of them
    const unsigned long long e = E[i], o = O[i];
    const unsigned long long m = (e & ~kFxNaN) + (o & ~kFxNaN);   // below 2^63: the sums of at most `samples` samples
    double s = ((double)(uint32_t)(m >> 32) * 4294967296.0 + (double)(uint32_t)m) * inv_scale;
    s = s / (double)n;
    if ((e | o) & kFxNaN) s = __builtin_nan("");
    out[i] = (real)s;
    if (counts && i == (size_t)px * 3) counts[px] = n;
}

static int32_t elapsed_into(CrHandle* h, hipEvent_t a, hipEvent_t b, double& sum) {
    float ms = 0;
    HIP_TRY(h, hipEventSynchronize(b));
    HIP_TRY(h, hipEventElapsedTime(&ms, a, b));
    sum += ms;
    return CR_OK;
}

int32_t adaptive_passes(CrHandle* h, const AdaptiveRun& run, const AdaptiveFrame& fr, const AdaptivePass& pass) {
    const uint32_t L = (uint32_t)run.block_log2;
    if (fr.lw > L || fr.lh > L) return fail(h, CR_ERR_UNSUPPORTED, "the work tile does not divide the adaptive block");
    const int32_t P = run.pass_samples, S = fr.samples;
    const size_t words = (size_t)fr.W * (size_t)fr.H * 3;
    const uint32_t n_tiles = fr.tiles_x * fr.tiles_y;
    const uint32_t bx_n = adaptive_blocks_x(fr.W, L), n_blocks = bx_n * adaptive_blocks_y(fr.H, L);
    auto need = [&](DevBuf& buf, size_t bytes, const char* what) -> int32_t {
        const hipError_t e = buf.ensure(bytes);
        if (e == hipSuccess) return CR_OK;
        (void)hipGetLastError();
        return fail(h, CR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    int32_t rc;
    if ((rc = need(h->ad_acc, 2 * words * sizeof(unsigned long long), "adaptive accumulators")) != CR_OK) return rc;
    if ((rc = need(h->ad_lists, 2 * (size_t)n_tiles * sizeof(int32_t), "adaptive tile lists")) != CR_OK) return rc;
    if ((rc = need(h->ad_block_n, (size_t)n_blocks * sizeof(int32_t), "adaptive block counts")) != CR_OK) return rc;
    if ((rc = need(h->ad_ctrl, 16, "adaptive cursor")) != CR_OK) return rc;
    if (!h->ad_ev0) HIP_TRY(h, hipEventCreate(&h->ad_ev0));
    if (!h->ad_ev1) HIP_TRY(h, hipEventCreate(&h->ad_ev1));
    unsigned long long* const E = (unsigned long long*)h->ad_acc.p;
    unsigned long long* const O = E + words;
    int32_t* const lists = (int32_t*)h->ad_lists.p;
    HIP_TRY(h, hipMemsetAsync(E, 0, 2 * words * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ad_block_n.p, 0, (size_t)n_blocks * sizeof(int32_t), h->stream));

    int exp2 = 0;
    (void)std::frexp(fr.fx_scale, &exp2);   // fx_scale = 2^(exp2 - 1)
    JudgeArgs ja;
    ja.E = E; ja.O = O; ja.W = fr.W; ja.H = fr.H; ja.block_log2 = L; ja.n_blocks = n_blocks;
    ja.lw = fr.lw; ja.lh = fr.lh; ja.tiles_x = fr.tiles_x; ja.tiles_y = fr.tiles_y;
    ja.tolerance = run.tolerance; ja.scale12 = std::ldexp(1.0, exp2 - 1 - 12);
    ja.block_n = (int32_t*)h->ad_block_n.p; ja.cursor = (uint32_t*)h->ad_ctrl.p;

    const int32_t* list = nullptr;   // the first passes render every tile, in order
    uint32_t active = n_tiles;
    int cur = 0, passes = 0;
    double render_ms = 0, judge_ms = 0;
    bool span_open = false;          // ev0 .. ev1 spans the render launches since the last judgement
    for (int32_t n = 0, q = 1; n < S && active > 0; q++) {
        if (!span_open) { HIP_TRY(h, hipEventRecord(h->ev0, h->stream)); span_open = true; }
        if ((rc = pass(list, active, n, n + P, E)) != CR_OK) return rc;
        if ((rc = pass(list, active, n + P, n + 2 * P, O)) != CR_OK) return rc;
        n += 2 * P; passes += 2;
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
        if (left > n_tiles) return fail(h, CR_ERR_HIP, "adaptive judge: more active tiles than the frame has");
        if ((rc = elapsed_into(h, h->ev0, h->ev1, render_ms)) != CR_OK) return rc;
        if ((rc = elapsed_into(h, h->ad_ev0, h->ad_ev1, judge_ms)) != CR_OK) return rc;
        list = next; cur ^= 1; active = left;
    }
    if (span_open) HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventRecord(h->ad_ev0, h->stream));
    const unsigned fin_grid = (unsigned)((words + 255) / 256);
    const double inv_scale = 1.0 / fr.fx_scale;
    if (fr.f64) hipLaunchKernelGGL((adaptive_finalize_kernel<double>), dim3(fin_grid), dim3(256), 0, h->stream, E, O, ja.block_n, (double*)fr.out, run.d_counts,
                                   fr.W, fr.H, L, S, inv_scale);
    else hipLaunchKernelGGL((adaptive_finalize_kernel<float>), dim3(fin_grid), dim3(256), 0, h->stream, E, O, ja.block_n, (float*)fr.out, run.d_counts,
                            fr.W, fr.H, L, S, inv_scale);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ad_ev1, h->stream));
    std::vector<int32_t> block_n(n_blocks);
    HIP_TRY(h, hipMemcpyAsync(block_n.data(), h->ad_block_n.p, (size_t)n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (span_open && (rc = elapsed_into(h, h->ev0, h->ev1, render_ms)) != CR_OK) return rc;
    if ((rc = elapsed_into(h, h->ad_ev0, h->ad_ev1, judge_ms)) != CR_OK) return rc;
    if (!run.stats) return CR_OK;
    uint64_t samples = 0;
    int32_t stopped = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint32_t x0, y0, bw, bh;
        adaptive_block_rect(fr.W, fr.H, L, b, x0, y0, bw, bh);
        samples += (uint64_t)bw * bh * (uint64_t)(block_n[b] ? block_n[b] : S);
        stopped += block_n[b] != 0;
    }
    CrAdaptiveStats* st = run.stats;
    memset(st, 0, sizeof *st);
    if ((rc = finish_stats(h, &st->render, samples, fr.n_entries, fr.scene_in_lds)) != CR_OK) return rc;
    st->render.kernel_ms = render_ms;   // (finish_stats saw the last run of passes only: the sum over all of them)
    st->judge_ms = judge_ms;
    st->passes = passes; st->blocks = (int32_t)n_blocks; st->blocks_stopped = stopped;
    return CR_OK;
}

// the checks of cr_render_adaptive_*, in the header's order; nothing has changed when one of them refuses
static int32_t validate_adaptive(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, const void* out) {
    int32_t rc = validate_render(h, cam, p);
    if (rc != CR_OK) return rc;
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
    return CR_OK;
}

static int32_t adaptive_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, void* d_out, int32_t* d_counts,
                               CrAdaptiveStats* stats) {
    HIP_TRY(h, hipSetDevice(h->device));
    const AdaptiveRun run = {ap->min_samples, ap->pass_samples, ap->block_log2 ? ap->block_log2 : 4, ap->tolerance, d_counts, stats};
    h->cam_pending_slot = -1;
    int32_t rc = p->real_type == CR_REAL_F64 ? render_typed<double>(h, cam, p, d_out, nullptr, nullptr, 1, nullptr, &run)
                                             : render_typed<float>(h, cam, p, d_out, nullptr, nullptr, 1, nullptr, &run);
    if (h->cam_pending_slot >= 0) {   // the camera-key slot is free again once everything queued so far has run
        const hipError_t e = hipEventRecord(h->cam_ev[h->cam_pending_slot], h->stream);
        h->cam_pending_slot = -1;
        if (e != hipSuccess && rc == CR_OK) { h->error = std::string("hipEventRecord: ") + hipGetErrorString(e); rc = CR_ERR_HIP; }
    }
    return rc;
}

}   // namespace cr

using namespace cr;

extern "C" {

int32_t cr_render_adaptive_device(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, void* d_out,
                                  int32_t* d_counts, CrAdaptiveStats* stats) {
    const int32_t rc = validate_adaptive(h, cam, p, ap, d_out);
    return rc != CR_OK ? rc : adaptive_device(h, cam, p, ap, d_out, d_counts, stats);
}

int32_t cr_render_adaptive_host(CrHandle* h, const CrCameraDesc* cam, const CrRenderParams* p, const CrAdaptiveParams* ap, void* h_out,
                                int32_t* h_counts, CrAdaptiveStats* stats) {
    int32_t rc = validate_adaptive(h, cam, p, ap, h_out);
    if (rc != CR_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_pix = (size_t)cam->image_width * (size_t)cam->image_height, bytes = n_pix * 3 * real_size(p->real_type);
    hipError_t e = h->out_buf.ensure(bytes);
    if (e == hipSuccess && h_counts) e = h->ad_counts.ensure(n_pix * sizeof(int32_t));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, CR_ERR_HIP, std::string("output buffer: ") + hipGetErrorString(e)); }
    rc = adaptive_device(h, cam, p, ap, h->out_buf.p, h_counts ? (int32_t*)h->ad_counts.p : nullptr, stats);
    if (rc != CR_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h_out, h->out_buf.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h_counts) HIP_TRY(h, hipMemcpyAsync(h_counts, h->ad_counts.p, n_pix * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint64_t bad = bad_pixels(h_out, p->real_type, n_pix);
    if (stats) stats->render.nan_pixels = bad;
    if (bad) return fail(h, CR_ERR_NAN, "a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)");
    return CR_OK;
}

}   // extern "C"
