// adaptive_region_check.cpp -- the region functions of crucible_amd/csrc/adaptive.hpp on the CPU (tests/test_adaptive_region_host.py):
// "W H x0 y0 w h block_log2" on the command line, a region inside the W x H frame.  Prints "aligned blocks_x blocks_y" -- the
// predicate under which the region's blocks are the frame's, and the region's block grid -- and then per block of the region
// "b x0 y0 bw bh frame_block": its rectangle in the frame's pixels (N_b = bw * bh), and the frame's block it is where the
// region is aligned (-1 elsewhere).
#include "adaptive.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), rx0 = atoi(argv[3]), ry0 = atoi(argv[4]), rw = atoi(argv[5]), rh = atoi(argv[6]);
    const uint32_t L = (uint32_t)atoi(argv[7]);
    if (W < 1 || H < 1 || rx0 < 0 || ry0 < 0 || rw < 1 || rh < 1 || (long long)rx0 + rw > W || (long long)ry0 + rh > H || L < 3 || L > 5) return 2;
    const bool aligned = cr::adaptive_region_aligned(W, H, rx0, ry0, rw, rh, L);
    const uint32_t bx_n = cr::adaptive_blocks_x(rw, L), by_n = cr::adaptive_blocks_y(rh, L);
    printf("%d %u %u\n", aligned ? 1 : 0, bx_n, by_n);
    for (uint32_t b = 0; b < bx_n * by_n; b++) {
        uint32_t x0, y0, bw, bh;
        cr::adaptive_region_block_rect(rx0, ry0, rw, rh, L, b, x0, y0, bw, bh);
        long long fb = -1;
        if (aligned) {
            fb = cr::adaptive_region_frame_block(W, rx0, ry0, rw, L, b);
            // the frame's block of that number is the same rectangle
            uint32_t fx0, fy0, fbw, fbh;
            cr::adaptive_block_rect(W, H, L, (uint32_t)fb, fx0, fy0, fbw, fbh);
            if (fx0 != x0 || fy0 != y0 || fbw != bw || fbh != bh) return 3;
        }
        printf("%u %u %u %u %u %lld\n", b, x0, y0, bw, bh, fb);
    }
    return 0;
}
