// aov_counts.hpp -- the integer rules of the guide pass at a count plane (cr_render_aov_counts_*): how a
// plane's value becomes a pixel's sample count, how many sample groups a tile's unit still has to run, and when the
// finalize divides.  The COUNTS kernels (aov_kernel.hpp) and the counts finalize (aov.hip) call these and nothing else for
// it.  Free of the HIP runtime, so that a plain C++ compiler can check them (tests/aov_counts_check.cpp), as it checks
// residency.hpp and adaptive.hpp.
#pragma once
#include "hd.hpp"

#include <stdint.h>

namespace cr {

// n_p = min(max(counts[p], 0), samples): the samples pixel p takes, the indices [0, n_p).  samples >= 1.
CR_HD uint32_t aov_count_clamp(int32_t count, int32_t samples) {
    return (uint32_t)(count < 0 ? 0 : (count > samples ? samples : count));
}

// The end of a unit's group loop: the unit's own end g1, or the groups of four samples that the tile's largest count
// needs, whichever is smaller.  In uint32_t: tile_max <= INT32_MAX, and INT32_MAX + 3 is not formed in int.  A unit
// whose first group g0 is not below the result has nothing to do.
CR_HD uint32_t aov_count_group_end(uint32_t g1, uint32_t tile_max) {
    const uint32_t need = (tile_max + 3u) >> 2;
    return need < g1 ? need : g1;
}

// Whether the finalize divides pixel p's sums by n_p: means only, and never by zero -- a pixel without samples has
// zero sums and keeps them as +0.0.
CR_HD bool aov_count_divides(uint32_t n_p, int32_t output_sum) { return !output_sum && n_p != 0u; }

}   // namespace cr
