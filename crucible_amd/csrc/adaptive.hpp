// adaptive.hpp -- the arithmetic of cr_render_adaptive_* (include/crucible_hip.h) that the judge kernel and
// the host share: a block's geometry, one term of its difference sum D_b and its threshold T_b.  Free of the HIP runtime,
// so that a plain C++ compiler can check it (tests/adaptive_check.cpp), as it checks fastdiv.hpp and tree.hpp.
#pragma once
#include "hd.hpp"

#include <stdint.h>

namespace cr {

constexpr uint64_t kAdaptiveFlag = 0x8000000000000000ull;   // bit 63 of a relaxed sum: the NaN flag, not part of the magnitude

// d(x, c) = |mag(E) - mag(O)| >> 12 of one channel's two half-frame sums
CR_HD uint64_t adaptive_term(uint64_t e, uint64_t o) {
    const uint64_t a = e & ~kAdaptiveFlag, b = o & ~kAdaptiveFlag;
    return (a > b ? a - b : b - a) >> 12;
}

// T_b = (uint64) min(floor(tolerance * (2^(S-12) * qP * 3 N_b)), 2^63): scale12 = 2^(S-12), qp = q * P (the samples in each
// half), n_b = the block's pixels inside the frame.  The weight is an integer below 2^53 times a power of two, exact in
// f64; then one multiply and one floor.  tolerance >= 0 and finite (the entry checks it); a product at or beyond 2^63,
// infinity included, gives 2^63, which no D_b reaches.
CR_HD uint64_t adaptive_threshold(double tolerance, double scale12, uint32_t qp, uint32_t n_b) {
    const double weight = scale12 * (double)((uint64_t)qp * 3u * (uint64_t)n_b);
    const double t = __builtin_floor(tolerance * weight);
    return t < 0x1.0p63 ? (uint64_t)t : (uint64_t)1 << 63;
}

// Blocks of 2^block_log2 pixels square, anchored at pixel (0, 0), numbered row by row; edge blocks are partial.
CR_HD uint32_t adaptive_blocks_x(int32_t W, uint32_t block_log2) { return ((uint32_t)W + (1u << block_log2) - 1u) >> block_log2; }
CR_HD uint32_t adaptive_blocks_y(int32_t H, uint32_t block_log2) { return ((uint32_t)H + (1u << block_log2) - 1u) >> block_log2; }
// block b's pixels inside the frame: bw columns from x0, bh rows from y0 (N_b = bw * bh)
CR_HD void adaptive_block_rect(int32_t W, int32_t H, uint32_t block_log2, uint32_t b, uint32_t& x0, uint32_t& y0, uint32_t& bw, uint32_t& bh) {
    const uint32_t bx_n = adaptive_blocks_x(W, block_log2), B = 1u << block_log2;
    const uint32_t by = b / bx_n, bx = b - by * bx_n;
    x0 = bx << block_log2; y0 = by << block_log2;
    bw = (uint32_t)W - x0 < B ? (uint32_t)W - x0 : B;
    bh = (uint32_t)H - y0 < B ? (uint32_t)H - y0 : B;
}
// A batch of frames (cr_render_adaptive_frames_*): the judge numbers the blocks of all frames in one row,
// frame after frame -- global block g is block b of frame f ...
CR_HD void adaptive_batch_block(uint32_t g, uint32_t n_blocks, uint32_t& f, uint32_t& b) { f = g / n_blocks; b = g - f * n_blocks; }
// ... and names a tile as the render kernel's batch does: frame f owns the tile rows [f * tiles_y, (f + 1) * tiles_y)
CR_HD uint32_t adaptive_batch_tile(uint32_t f, uint32_t tiles_x, uint32_t tiles_y, uint32_t tx, uint32_t ty) { return (f * tiles_y + ty) * tiles_x + tx; }
// The tiles of 2^lw x 2^lh pixels (lw, lh <= block_log2; tiles_x x tiles_y of them cover the frame) of the block whose
// first pixel is (x0, y0): tw columns from tx0, th rows from ty0.  Blocks and tiles are both anchored at pixel (0, 0),
// so the blocks' tiles partition the tile grid.
CR_HD void adaptive_block_tiles(uint32_t x0, uint32_t y0, uint32_t block_log2, uint32_t lw, uint32_t lh, uint32_t tiles_x, uint32_t tiles_y,
                                uint32_t& tx0, uint32_t& ty0, uint32_t& tw, uint32_t& th) {
    const uint32_t B = 1u << block_log2;
    tx0 = x0 >> lw; ty0 = y0 >> lh;
    tw = (B >> lw) < tiles_x - tx0 ? (B >> lw) : tiles_x - tx0;
    th = (B >> lh) < tiles_y - ty0 ? (B >> lh) : tiles_y - ty0;
}
// the k-th (row by row) of those tw * th tiles, as frame f's batch-wide tile number
CR_HD uint32_t adaptive_block_tile(uint32_t f, uint32_t tiles_x, uint32_t tiles_y, uint32_t tx0, uint32_t ty0, uint32_t tw, uint32_t k) {
    const uint32_t r = k / tw;
    return adaptive_batch_tile(f, tiles_x, tiles_y, tx0 + (k - r * tw), ty0 + r);
}
// A region of a frame (cr_render_adaptive_region_*): the region is judged as if it were the frame, so the
// functions above take the region's width and height and work in region-local pixels; the blocks (and the render
// kernel's tiles) are anchored at the region's origin.  Block b of the region (rx0, ry0, rw, rh), in the frame's pixels:
CR_HD void adaptive_region_block_rect(int32_t rx0, int32_t ry0, int32_t rw, int32_t rh, uint32_t block_log2, uint32_t b,
                                      uint32_t& x0, uint32_t& y0, uint32_t& bw, uint32_t& bh) {
    adaptive_block_rect(rw, rh, block_log2, b, x0, y0, bw, bh);
    x0 += (uint32_t)rx0; y0 += (uint32_t)ry0;
}
// Are the region's blocks blocks of the W x H frame, partial ones included?  The origin on multiples of the block's side,
// and the right and the bottom edge each on such a multiple or on the frame's edge.  Then image and counts of the region
// are the frame's own adaptive render on those pixels, and regions like that which tile a frame give that frame.
// (the region lies inside the frame: the entry point has checked it)
CR_HD bool adaptive_region_aligned(int32_t W, int32_t H, int32_t rx0, int32_t ry0, int32_t rw, int32_t rh, uint32_t block_log2) {
    const int64_t m = ((int64_t)1 << block_log2) - 1, x1 = (int64_t)rx0 + rw, y1 = (int64_t)ry0 + rh;
    return !(rx0 & m) && !(ry0 & m) && (!(x1 & m) || x1 == W) && (!(y1 & m) || y1 == H);
}
// ... and block b of such a region is this block of the frame
CR_HD uint32_t adaptive_region_frame_block(int32_t W, int32_t rx0, int32_t ry0, int32_t rw, uint32_t block_log2, uint32_t b) {
    const uint32_t bx_n = adaptive_blocks_x(rw, block_log2), by = b / bx_n, bx = b - by * bx_n;
    return (((uint32_t)ry0 >> block_log2) + by) * adaptive_blocks_x(W, block_log2) + ((uint32_t)rx0 >> block_log2) + bx;
}
// does a block with difference sum d stop?
CR_HD bool adaptive_stops(uint64_t d, uint64_t t) { return d <= t; }

}   // namespace cr
