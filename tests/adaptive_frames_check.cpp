// adaptive_frames_check.cpp -- the batch functions of crucible_amd/csrc/adaptive.hpp on the CPU (tests/test_adaptive_frames_host.py):
// "W H block_log2 lw lh n_frames" on the command line.  Prints per global block of the batch, in the judge kernel's numbering,
// "g f b x0 y0 bw bh : tile tile ...": the frame and the block in it, the block's rectangle, and its tiles as the batch-wide
// numbers the judge appends to the active-tile list, in the order its lanes write them.
#include "adaptive.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    const uint32_t L = (uint32_t)atoi(argv[3]), lw = (uint32_t)atoi(argv[4]), lh = (uint32_t)atoi(argv[5]), n_frames = (uint32_t)atoi(argv[6]);
    if (W < 1 || H < 1 || lw > L || lh > L || n_frames < 1) return 2;
    const uint32_t tiles_x = ((uint32_t)W + (1u << lw) - 1) >> lw, tiles_y = ((uint32_t)H + (1u << lh) - 1) >> lh;   // as launch() counts them
    const uint32_t n_blocks = cr::adaptive_blocks_x(W, L) * cr::adaptive_blocks_y(H, L);
    for (uint32_t g = 0; g < n_frames * n_blocks; g++) {
        uint32_t f, b, x0, y0, bw, bh, tx0, ty0, tw, th;
        cr::adaptive_batch_block(g, n_blocks, f, b);
        cr::adaptive_block_rect(W, H, L, b, x0, y0, bw, bh);
        cr::adaptive_block_tiles(x0, y0, L, lw, lh, tiles_x, tiles_y, tx0, ty0, tw, th);
        printf("%u %u %u %u %u %u %u :", g, f, b, x0, y0, bw, bh);
        for (uint32_t k = 0; k < tw * th; k++) {
            const uint32_t t = cr::adaptive_block_tile(f, tiles_x, tiles_y, tx0, ty0, tw, k);
            if (t != cr::adaptive_batch_tile(f, tiles_x, tiles_y, tx0 + k % tw, ty0 + k / tw)) return 3;
            printf(" %u", t);
        }
        printf("\n");
    }
    return 0;
}
