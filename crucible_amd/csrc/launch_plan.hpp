// launch_plan.hpp -- how a render or a guide pass is cut into kernel launches: the work tile and the LDS
// bytes of the sums' slots, the sample batch that the 32-bit work counter and the colour buffer allow, the whole frames
// one launch holds, a batch's groups, work items and chunk, the grid, and the guide pass's units.  launch() (render.hpp)
// and aov_launch() (aov_kernel.hpp) ask these functions and keep the HIP calls; nothing here touches a device.  Free of
// the HIP runtime and of the record types -- sizes arrive as numbers --, so that a plain C++ compiler can check it
// (tests/launch_plan_check.cpp), as it checks residency.hpp, whose layout and RES_* this header builds on.
#pragma once
#include "hd.hpp"
#include "residency.hpp"

#include <cmath>

namespace cr {

CR_HD uint64_t plan_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
CR_HD uint64_t plan_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ------------------------------------------------------------------ the small rules

// Work items per atomic on the work counter.  1024 keeps the counter quiet on long launches; a short launch (a
// small frame, or one GPU's shard of the samples) would end with whole chunks of imbalance, so a wave's chunk is at most
// 1/128 of its share, and at least one wave's round.  chunk_override: CRUCIBLE_SG_CHUNK.
CR_HD uint32_t work_chunk(uint64_t sg_total, uint64_t grid, uint64_t block, int chunk_override) {
    const uint64_t waves = grid * block / 64, per_wave = sg_total / (waves > 1 ? waves : 1);
    const uint64_t share = per_wave / 128;
    const uint64_t c = chunk_override > 0 ? (uint64_t)chunk_override : (share < 64 ? 64 : (share > 1024 ? 1024 : share));
    return (uint32_t)((c + 63) / 64 * 64);
}

// The default work tile of 2^lw x 2^lh pixels times 64 >> (lw + lh) samples, by the samples n a launch renders:
// 4 x 4 x 4, wider tiles of fewer samples when there are fewer than 4
CR_HD void default_tile(int64_t n, int& lw, int& lh) {
    lw = n >= 4 ? 2 : 3;
    lh = n >= 2 ? 2 : 3;
}

// LDS bytes of a block's relaxed sums: two slots per wave of 3 words per pixel of a 2^tile_log2-pixel tile
constexpr size_t fx_lds_bytes(int block, uint32_t tile_log2) { return (size_t)(block / 64) * 2 * ((size_t)3 << tile_log2) * sizeof(unsigned long long); }

// LDS bytes of a block's guide slots: per wave 16 pixels x 8 words (aov.hpp, which holds the layout, asserts the number)
constexpr size_t kAovSlotBytes = 1024;
constexpr size_t aov_lds_bytes(int block) { return (size_t)(block / 64) * kAovSlotBytes; }

// CR_SUM_RELAXED's fixed-point scale 2^S for n samples per pixel: n * 2^S < 2^63, S = 52 up to 2047 samples
inline double fx_scale_for(int64_t n) {
    int lg = 0;
    while ((n >> (lg + 1)) > 0) lg++;
    return std::ldexp(1.0, 52 < 62 - lg ? 52 : 62 - lg);
}

// the launch covers every pixel of its W x H frame: no region
CR_HD bool whole_frame(uint32_t reg_x0, uint32_t reg_y0, uint32_t reg_w, uint32_t reg_h, int32_t W, int32_t H) {
    return !reg_x0 && !reg_y0 && reg_w == (uint32_t)W && reg_h == (uint32_t)H;
}

// ------------------------------------------------------------------ the tile and the LDS of a render launch

// The work tile (sample-granular hand-out): 2^lw x 2^lh pixels times 64 >> (lw + lh) consecutive samples; and what a
// block takes of LDS.  relax: the waves' accumulator slots follow the scene there (2 x 384 B per wave for a 16-pixel tile).
struct TilePlan {
    int lw, lh;
    bool relax, use_lds;             // use_lds: the launch asks for dynamic LDS at all (a staged scene, or the sums' slots)
    size_t scene_lds_bytes;
    size_t fx_off;                   // where the slots begin (KernelArgs::fx_lds_off): behind the scene, 0 without one
    size_t lds_base, lds_per_wave;   // what pick_block budgets: a block's bytes whatever its size, and per wave
    CR_HD size_t lds_bytes(int block) const { return relax ? fx_off + fx_lds_bytes(block, (uint32_t)(lw + lh)) : scene_lds_bytes; }
};

// tile_lw, tile_lh: the handle's override (CRUCIBLE_SG_TILE), -1 without one; n_samples: what one launch renders (an
// adaptive run: one pass); block_log2: an adaptive run's block, whose sides the tile's must divide, -1 outside one.
// A tile too large for what the scene leaves free of 160 KB falls back to 16 pixels (the surplus sample slots of its
// groups stay empty); the fallback itself is not measured again.
CR_HD TilePlan plan_tile(int tile_lw, int tile_lh, int64_t n_samples, int block_log2, bool relax, int res, size_t scene_lds_bytes, int max_block) {
    TilePlan t = {};
    t.relax = relax; t.use_lds = res != RES_GLOBAL || relax; t.scene_lds_bytes = scene_lds_bytes;
    if (block_log2 >= 0 && (tile_lw > block_log2 || tile_lh > block_log2)) tile_lw = tile_lh = -1;
    if (tile_lw < 0) default_tile(n_samples, tile_lw, tile_lh);
    t.fx_off = res != RES_GLOBAL ? r16(scene_lds_bytes) : 0;
    if (relax && t.fx_off + fx_lds_bytes(max_block, (uint32_t)(tile_lw + tile_lh)) > (size_t)160 * 1024) { tile_lw = 2; tile_lh = 2; }
    t.lw = tile_lw; t.lh = tile_lh;
    t.lds_base = relax ? t.fx_off : (t.use_lds ? scene_lds_bytes : 0);
    t.lds_per_wave = relax ? fx_lds_bytes(64, (uint32_t)(tile_lw + tile_lh)) : 0;
    return t;
}

// ------------------------------------------------------------------ what a kernel kind renders

enum CallShape { kShapeOk, kShapeOneFrame, kShapeWholeFrames, kShapeNoList };

// keyed: the kernel carries a batch's frame arithmetic and a region's offsets (relaxed kernels only); latency: the
// 6-waves-per-SIMD entry point; list: the kernel carries the active-tile list, which adaptive runs and no others use
CR_HD CallShape check_call_shape(bool relax, bool keyed, bool latency, bool list, int32_t n_frames, bool whole, bool adaptive) {
    if (n_frames > 1 && !(relax && keyed)) return kShapeOneFrame;
    if (!whole && (latency || !(relax && keyed))) return kShapeWholeFrames;
    if (list != adaptive) return kShapeNoList;
    return kShapeOk;
}

// ------------------------------------------------------------------ samples per launch, frames per launch

struct SampleQuery {
    bool relax, sample_granular;         // the sum order; CRUCIBLE_SAMPLE_GRANULAR (reference order: 0 = a lane owns a pixel)
    int32_t s_begin, s_end;              // the samples of the call (an adaptive run: of one pass)
    uint32_t reg_w, reg_h;               // the launch's pixels: the region's, else the frame's
    size_t real_bytes;
    size_t sample_buf_limit;             // CRUCIBLE_SAMPLE_BUF_MB
    uint64_t work_counter_max;           // CRUCIBLE_WORK_COUNTER_MAX
    int lw, lh;                          // plan_tile's
    bool tile_fixed;                     // ... which the handle named: the batch does not choose another
    int32_t n_frames;
    bool adaptive, split_passes, fixed_sums;   // fixed_sums: CR_OUTPUT_FIXED_SUM, the sums go straight into the caller's buffer
    uint32_t px_tiles_x, px_tiles_y;     // the 8 x 8 tiles of the plan in which a lane owns a pixel, as the arguments arrive
};

// the groups of ns samples that n samples fill; the end of the batch that begins at sample b0 (64 bits: b0 + batch may pass INT32_MAX)
CR_HD uint32_t sample_groups(int32_t n, uint32_t ns) { return (uint32_t)(((int64_t)n + ns - 1) / ns); }
CR_HD int32_t batch_end(int64_t b0, int32_t batch, int32_t s_end) { return (int32_t)(b0 + batch < (int64_t)s_end ? b0 + batch : (int64_t)s_end); }

enum PlanRefusal { kPlanOk, kPlanCounter, kPlanCounterPass };   // "image too large for the 32-bit work counter", "... at this pass_samples"

struct SamplePlan {
    PlanRefusal refusal;
    bool tiled;                  // lw, lh are the launch's (also where batch fell to 0 afterwards); else the arguments keep theirs
    int32_t batch;               // samples per launch; 0: a lane owns a pixel and sums its samples itself (KernelArgs::sg_on = 0)
    int lw, lh;
    uint32_t tiles_x, tiles_y;
    uint32_t ns;                 // samples per group, 64 >> (lw + lh); 1 where batch is 0
    int32_t fpl;                 // whole frames per launch (a frame that needs sample batches on its own renders frame by frame)
    size_t npix;                 // of one frame of the launch
    size_t frame_words, fx_words;   // relaxed: 64-bit sums of one frame, of all frames
    size_t fx_acc_bytes, sample_buf_bytes, sg_acc_bytes;   // what the launch wants of the handle's buffers; 0: nothing
    uint32_t px_tiles_x, px_tiles_y;

    CR_HD uint64_t tiles() const { return (uint64_t)tiles_x * tiles_y; }
    CR_HD uint64_t tile_pixels() const { return tiles() << (lw + lh); }   // edge padding included
    // the work items of the largest launch, which sizes the grid
    CR_HD uint64_t grid_work(int32_t n_samples) const {
        return batch > 0 ? tiles() * (uint64_t)fpl * sample_groups(batch < n_samples ? batch : n_samples, ns) * 64u : tiles() * 64u;
    }
};

// The fallback of the reference order: a lane owns a pixel.  Also what launch() applies when a buffer the plan wanted
// cannot be had.
CR_HD void lane_owns_pixel(SamplePlan& p) {
    p.batch = 0; p.ns = 1;
    p.tiles_x = p.px_tiles_x; p.tiles_y = p.px_tiles_y;
    p.sample_buf_bytes = p.sg_acc_bytes = 0;
}

// Sample-granular mode: batches of samples whose work items the 32-bit counter holds -- tiles * groups * 64 plus one chunk
// per wave -- and, in the reference order, whose colours fit the buffer: one colour per work item of a batch, whole tiles
// and whole sample groups (edge padding included).
CR_HD SamplePlan plan_samples(const SampleQuery& q) {
    SamplePlan p = {};
    p.refusal = kPlanOk; p.tiled = false; p.batch = 0; p.fpl = 1; p.ns = 1;
    p.lw = q.lw; p.lh = q.lh;
    p.px_tiles_x = p.tiles_x = q.px_tiles_x; p.px_tiles_y = p.tiles_y = q.px_tiles_y;
    const size_t npix = p.npix = (size_t)q.reg_w * (size_t)q.reg_h;
    p.frame_words = npix * 3; p.fx_words = (size_t)q.n_frames * npix * 3;
    if (!((q.sample_granular || q.relax) && q.s_end > q.s_begin)) return p;
    const int32_t n = q.s_end - q.s_begin;
    const size_t per_sample = npix * 3 * q.real_bytes;
    p.batch = (int32_t)plan_min((uint64_t)n, q.relax ? (uint64_t)INT32_MAX : plan_max(1, q.sample_buf_limit / per_sample));
    if (!q.relax && !q.tile_fixed) default_tile(p.batch, p.lw, p.lh);   // by the batch, which the buffer may have cut
    p.tiled = true;
    p.ns = 64u >> (p.lw + p.lh);
    p.tiles_x = (q.reg_w + (1u << p.lw) - 1) >> p.lw; p.tiles_y = (q.reg_h + (1u << p.lh) - 1) >> p.lh;
    const uint64_t max_groups = q.work_counter_max / (p.tiles() * 64);
    if (max_groups < 1) p.batch = 0;
    else p.batch = (int32_t)plan_min((uint64_t)p.batch, max_groups * p.ns);
    if (q.relax) {
        if (p.batch <= 0) { p.refusal = kPlanCounter; return p; }
        if (p.batch == n) p.fpl = (int32_t)plan_min((uint64_t)q.n_frames, max_groups / (((uint64_t)p.batch + p.ns - 1) / p.ns));
        // (cr_render_adaptive_region_*: such a pass runs as consecutive launches of `batch` samples, as a region render's samples do)
        if (q.adaptive && !q.split_passes && p.batch < n) { p.refusal = kPlanCounterPass; return p; }
        if (!q.fixed_sums && !q.adaptive) p.fx_acc_bytes = p.fx_words * sizeof(unsigned long long);   // (adaptive_passes keeps its own two accumulators)
        return p;
    }
    const uint32_t ns = p.ns;
    const uint64_t tiles = p.tiles();
    auto batch_bytes = [&](int32_t b) { return (size_t)tiles * (((size_t)b + ns - 1) / ns) * 64u * 3u * q.real_bytes; };
    while (p.batch > (int32_t)ns && batch_bytes(p.batch) > (size_t)plan_max(q.sample_buf_limit, batch_bytes((int32_t)ns))) p.batch -= (int32_t)ns;
    if (p.batch == 0) { lane_owns_pixel(p); return p; }
    p.sample_buf_bytes = batch_bytes(p.batch);
    if (p.batch < n) p.sg_acc_bytes = per_sample;   // the running sums between batches
    return p;
}

// The attenuation stack of the reference order: three reals per bounce and thread
CR_HD size_t att_stack_bytes(int32_t max_depth, uint32_t n_threads, size_t real_bytes) {
    return (size_t)3 * (size_t)(max_depth > 0 ? max_depth : 1) * n_threads * real_bytes;
}

// the samples whose scale the relaxed sums of this launch carry: CR_OUTPUT_FIXED_SUM and adaptive runs the whole frame's, so
// that the words of any shards of it add up to the frame's
CR_HD int64_t fx_scale_samples(bool fixed_sums, bool adaptive, int32_t samples_total, int32_t s_begin, int32_t s_end) {
    return fixed_sums || adaptive ? samples_total : s_end - s_begin;
}

// ------------------------------------------------------------------ the grid

// Persistent blocks: as many as fit the device (n_cus * per_cu), no more than the work fills, at least one.
// lanes_per_item: 1 for the render, whose work item is a thread's; 64 for the guide pass, whose unit is a wave's.
struct GridPlan { uint32_t blocks, n_threads; };
CR_HD GridPlan plan_grid(int n_cus, int per_cu, uint64_t work, int block, int lanes_per_item) {
    uint32_t grid = (uint32_t)(n_cus * per_cu);
    const int per_block = block / lanes_per_item;
    const uint64_t need_blocks = (work + per_block - 1) / per_block;
    if ((uint64_t)grid > need_blocks) grid = (uint32_t)need_blocks;
    if (grid < 1) grid = 1;
    return {grid, grid * (uint32_t)block};
}

// ------------------------------------------------------------------ one batch of samples

// One batch of n_samples samples, ns to a group, of frames * tiles tiles (those of all the launch's frames): its groups, work
// items and chunk.
// fit: on no more blocks than the items fill (a pass may name few tiles); else on the whole grid
struct BatchLaunch { uint32_t groups, sg_total, blocks, chunk; };
CR_HD BatchLaunch plan_batch(uint32_t ns, int32_t n_samples, uint64_t tiles, int32_t frames, bool fit, uint32_t grid, int block, int chunk_override) {
    BatchLaunch b;
    b.groups = sample_groups(n_samples, ns);
    b.sg_total = (uint32_t)(tiles * (uint64_t)frames * b.groups * 64u);
    b.blocks = fit ? (uint32_t)plan_max(1, plan_min(grid, ((uint64_t)b.sg_total + block - 1) / block)) : grid;
    b.chunk = work_chunk(b.sg_total, b.blocks, (uint64_t)block, chunk_override);
    return b;
}

// ------------------------------------------------------------------ the guide pass's units

// A unit is unit_groups consecutive sample groups of one tile: about eight units per resident wave, so that the tail is
// short and a unit still flushes rarely.  A batch (the BATCH kernels) is sized as one piece of work: the eight units per
// wave count the units of all its frames.  Its units are capped by work_counter_max -- a limit below one frame's tiles,
// which only a test sets, is raised to them --, the other kernels' by the 32-bit counter (a frame has at most 2^22 tiles);
// a batch with more runs as consecutive launches of frames_per_launch whole frames.
struct GuidePlan {
    uint32_t unit_groups, unit_chunks, frame_tiles;   // groups per unit, units per tile, tiles per frame
    uint64_t n_frames, frame_units, frames_per_launch;
    CR_HD uint64_t slice_frames(uint64_t f0) const { return plan_min(frames_per_launch, n_frames - f0); }
    CR_HD uint32_t units(uint64_t fn) const { return (uint32_t)(fn * frame_units); }
};
CR_HD GuidePlan plan_guide_units(uint32_t tiles_x, uint32_t tiles_y, uint32_t groups, bool batch, uint32_t batch_frames, int n_cus, int per_cu, int block,
                                 uint64_t work_counter_max) {
    GuidePlan g;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    g.n_frames = batch ? batch_frames : 1;
    const uint64_t resident = (uint64_t)n_cus * per_cu * (block / 64);
    uint64_t ug = plan_min(groups, plan_max(1, g.n_frames * tiles * groups / (8 * resident)));
    const uint64_t max_units = batch ? plan_max(work_counter_max, tiles) : 0xF0000000ull;
    if (tiles * ((groups + ug - 1) / ug) > max_units) ug = (groups + max_units / tiles - 1) / (max_units / tiles);
    g.unit_groups = (uint32_t)ug;
    g.unit_chunks = (uint32_t)((groups + ug - 1) / ug);
    g.frame_tiles = (uint32_t)tiles;
    g.frame_units = tiles * g.unit_chunks;
    g.frames_per_launch = plan_min(g.n_frames, max_units / g.frame_units);
    return g;
}

}   // namespace cr
