// aov.hpp -- the guide pass (cr_render_aov_*): first-hit albedo, normal, depth and coverage per pixel.  What its units
// share: the kernel's arguments, the accumulator layout and the entry into the kernels' residency ladder.  The kernels
// themselves are in aov_kernel.hpp (aov_f32.hip and aov_f64.hip emit them, aov_counts_f32.hip and aov_counts_f64.hip those at
// a count plane), the host side and the finalize kernel in aov.hip.
//
// A work item is one (pixel, sample): 64 consecutive items are a 4 x 4 pixel tile times 4 consecutive samples, one wave's
// round.  A wave takes a UNIT from the launch's work counter -- `unit_groups` consecutive sample groups of one tile --, adds
// the rounds' values into its LDS slot (16 pixels x 8 words) and sends the slot's non-zero words to the global
// accumulators once per unit.  Per pixel the accumulators are kAovWords 64-bit words:
//   0..2 albedo, 3..5 encoded normal, 6 coverage: sums of rint(x * 2^S) as signed integers (two's complement adds);
//   7 depth: the maximum of ~bits(depth) over the samples that hit, 0 = none did -- positive reals order as their bit
//     patterns, so this is the minimum depth, and a zeroed buffer is the empty state of every word.
// A value that is not finite (or too large for a word) sets the channel's bit in the pixel's flag word instead.
#pragma once
#include "handle.hpp"
#include "aov_counts.hpp"
#include "launch_plan.hpp"   // aov_lds_bytes, the guide pass's unit plan

namespace cr {

constexpr uint32_t kAovWords = 8, kAovDepth = 7, kAovCoverage = 6;
constexpr uint32_t kAovTileLog2 = 4;                                            // 4 x 4 pixels
constexpr uint32_t kAovSlotWords = kAovWords << kAovTileLog2;                   // one wave's LDS slot
static_assert(kAovSlotBytes == kAovSlotWords * sizeof(unsigned long long), "aov_lds_bytes (launch_plan.hpp) counts this slot");

template <typename real> struct AovArgs {
    KernelArgs<real> k;             // what the walk, the camera and the texture code read (prepare_args, render.hip)
    unsigned long long* acc;        // [H * W * kAovWords], zeroed before the launch
    uint32_t* flags;                // [H * W]: bit c set = channel c (0..5) met a value that is not finite
    int32_t layers;                 // CR_AOV_* mask: layers that were not asked for are not computed
    uint32_t groups;                // sample groups (of 4) that cover [sample_begin, sample_end)
    uint32_t unit_groups;           // groups per unit
    uint32_t unit_chunks;           // units per tile
    uint32_t n_units;
    uint32_t acc_lds_off;           // byte offset of the waves' slots in LDS (behind the staged scene)
    // A batch of frames (cr_render_aov_frames_*, the BATCH kernels): the units of n_frames frames one after the other,
    // frame_tiles tiles each.  Frame f's ray times start at frame_times[f]; its accumulators are acc + f * W * H *
    // kAovWords, its flags are flags + f * W * H.  n_frames = 0: a single frame (cr_render_aov_*), none of this is read.
    uint32_t n_frames;
    uint32_t frame_tiles;
    const real* frame_times;
    // cr_render_aov_counts_* (the COUNTS kernels, which are BATCH kernels): pixel p of frame f takes the samples
    // [0, aov_count_clamp(counts[f * reg_w * reg_h + p], samples)); the plane has the accumulators' layout.  Else not read.
    const int32_t* counts;
};

// aov_f32.hip, aov_f64.hip: the residency ladder of the guide kernels.  It asks the rule the render's walk_ladder asks
// (residency.hpp choose_residency: the whole scene in LDS, the top window, global memory; screening records where the
// render walks on them), so both stage the same records.  The trace kernel is launched on the handle's stream; *res
// receives the residency (CrStats.scene_in_lds).
template <typename real>
int32_t aov_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res);
// aov_counts_f32.hip, aov_counts_f64.hip: the same ladder over the COUNTS kernels (a.counts is set; a.n_frames >= 1)
template <typename real>
int32_t aov_counts_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res);
// aov_views_f32.hip, aov_views_f64.hip: the same ladder over the VIEWS kernels (a.k.views is set; a.n_frames >= 1)
template <typename real>
int32_t aov_views_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res);

}   // namespace cr
