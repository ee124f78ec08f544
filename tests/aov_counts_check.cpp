// aov_counts_check -- crucible_amd/csrc/aov_counts.hpp under a plain C++ compiler (tests/test_aov_counts_host.py builds it with
// g++, plain and with -fsanitize=undefined,address, and compares its lines with the rules restated in Python).
// Reads lines from stdin:  "clamp COUNT SAMPLES" | "end G1 TILE_MAX" | "unit G0 UNIT_GROUPS GROUPS TILE_MAX" | "div N_P OUTPUT_SUM"
// and prints one line each: the clamped count; the group loop's end; the unit's [g0, end) and whether it runs; 0 or 1.
#include "aov_counts.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

int main() {
    char what[16];
    long long a = 0, b = 0, c = 0, d = 0;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        const int n = sscanf(line, "%15s %lld %lld %lld %lld", what, &a, &b, &c, &d);
        if (n < 3) { fprintf(stderr, "bad line: %s", line); return 2; }
        if (!strcmp(what, "clamp")) printf("%" PRIu32 "\n", cr::aov_count_clamp((int32_t)a, (int32_t)b));
        else if (!strcmp(what, "end")) printf("%" PRIu32 "\n", cr::aov_count_group_end((uint32_t)a, (uint32_t)b));
        else if (!strcmp(what, "unit") && n == 5) {   // the kernel's own lines: g1 from the unit, then the bound
            const uint32_t g0 = (uint32_t)a, unit_groups = (uint32_t)b, groups = (uint32_t)c;
            const uint32_t g1 = g0 + unit_groups < groups ? g0 + unit_groups : groups;
            const uint32_t end = cr::aov_count_group_end(g1, (uint32_t)d);
            printf("%" PRIu32 " %" PRIu32 " %d\n", g0, end, g0 < end ? 1 : 0);
        } else if (!strcmp(what, "div")) printf("%d\n", cr::aov_count_divides((uint32_t)a, (int32_t)b) ? 1 : 0);
        else { fprintf(stderr, "bad line: %s", line); return 2; }
    }
    return 0;
}
