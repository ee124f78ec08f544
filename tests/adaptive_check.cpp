// adaptive_check.cpp -- crucible_amd/csrc/adaptive.hpp on the CPU (tests/test_adaptive_host.py): the judge's shared functions
// over a case file.  The file: "W H block_log2 scale_log2 qp tolerance" (tolerance as a C99 hex float), then W * H * 3 pairs
// "E O" of hex words, row-major.  Prints per block "b x0 y0 bw bh D T stops", summing the terms as the judge kernel does.
#include "adaptive.hpp"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int W, H, block_log2, scale_log2;
    unsigned qp;
    char tol_text[64];
    if (fscanf(f, "%d %d %d %d %u %63s", &W, &H, &block_log2, &scale_log2, &qp, tol_text) != 6) return 2;
    const double tolerance = strtod(tol_text, nullptr);
    std::vector<uint64_t> E((size_t)W * H * 3), O(E.size());
    for (size_t i = 0; i < E.size(); i++)
        if (fscanf(f, "%" SCNx64 " %" SCNx64, &E[i], &O[i]) != 2) return 2;
    fclose(f);
    const double scale12 = std::ldexp(1.0, scale_log2 - 12);
    const uint32_t n_blocks = cr::adaptive_blocks_x(W, (uint32_t)block_log2) * cr::adaptive_blocks_y(H, (uint32_t)block_log2);
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint32_t x0, y0, bw, bh;
        cr::adaptive_block_rect(W, H, (uint32_t)block_log2, b, x0, y0, bw, bh);
        uint64_t d = 0;
        for (uint32_t row = 0; row < bh; row++)
            for (uint32_t col = 0; col < bw * 3; col++) {
                const size_t i = ((size_t)(y0 + row) * (size_t)W + x0) * 3 + col;
                d += cr::adaptive_term(E[i], O[i]);
            }
        const uint64_t t = cr::adaptive_threshold(tolerance, scale12, qp, bw * bh);
        printf("%u %u %u %u %u %" PRIu64 " %" PRIu64 " %d\n", b, x0, y0, bw, bh, d, t, cr::adaptive_stops(d, t) ? 1 : 0);
    }
    return 0;
}
