// crucible_amd/csrc/fastdiv.hpp on the CPU: compiled with a plain C++ compiler (no device, no HIP runtime) and held to the
// machine's own `/` for tests/test_fastdiv_host.py.
//   fastdiv_check SEED    the listed divisors, each with its listed dividends, then 10^6 pairs (n, d) drawn from SEED; prints
//                         "divisors D edge_cases E random_cases R mismatches M" and the first mismatches, if any.
// Divisors: 1, 2, 3, 5, 7, 128, 480, 16384, 65535, 2^26, 2^31, 2^32 - 1, and 2^k, 2^k - 1, 2^k + 1 for every k in [0, 31]
// (those in [1, 2^32)).  Dividends per divisor d: 0, 1, d - 1, d, d + 1, 2^26 - 1, 2^31, 2^32 - 1, and m * d - 1, m * d, m * d + 1
// for the eight multiples m * d at and below floor((2^32 - 1) / d) (the top of the range, where the 33rd bit of the multiplier matters).
#include "fastdiv.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using namespace cr;

static uint64_t mismatches = 0;
static void check(uint32_t n, uint32_t d, const FastDiv& f) {
    const uint32_t got = fastdiv(n, f), want = n / d;
    if (got != want && mismatches++ < 16) printf("mismatch %u / %u: %u, not %u (mul %u sh1 %u sh2 %u)\n", n, d, got, want, f.mul, f.sh1, f.sh2);
}
static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: fastdiv_check SEED\n"); return 2; }
    uint64_t seed = strtoull(argv[1], nullptr, 0);
    const uint64_t top = 0xffffffffull;
    std::set<uint64_t> ds = {1, 2, 3, 5, 7, 128, 480, 16384, 65535, 1ull << 26, 1ull << 31, top};
    for (int k = 0; k < 32; k++) for (int64_t o = -1; o <= 1; o++) ds.insert((uint64_t)((int64_t)(1ull << k) + o));
    uint64_t n_div = 0, n_edge = 0;
    for (uint64_t d64 : ds) {
        if (d64 < 1 || d64 > top) continue;
        const uint32_t d = (uint32_t)d64;
        const FastDiv f = fastdiv_make(d);
        std::set<uint64_t> ns = {0, 1, d64 - 1, d64, d64 + 1, (1ull << 26) - 1, 1ull << 31, top};
        const uint64_t m_top = top / d64;
        for (uint64_t m = m_top; m + 8 > m_top && m >= 1; m--) for (int64_t o = -1; o <= 1; o++) ns.insert((uint64_t)((int64_t)(m * d64) + o));
        for (uint64_t n : ns) if (n <= top) { check((uint32_t)n, d, f); n_edge++; }
        n_div++;
    }
    // seeded pairs: divisors of every magnitude (a random bit length), dividends over the whole range and near multiples
    const uint64_t n_random = 1000000;
    for (uint64_t i = 0; i < n_random; i++) {
        const uint64_t r = splitmix(seed);
        const uint32_t bits = 1u + (uint32_t)(r % 32u);
        uint32_t d = (uint32_t)(splitmix(seed) >> (64 - bits));
        if (d == 0) d = 1;
        uint32_t n = (uint32_t)splitmix(seed);
        if (r & (1ull << 40)) n = (uint32_t)((uint64_t)(n / d) * d + ((r >> 41) % 3) - 1);   // a multiple of d, one below, one above
        check(n, d, fastdiv_make(d));
    }
    printf("divisors %llu edge_cases %llu random_cases %llu mismatches %llu\n", (unsigned long long)n_div, (unsigned long long)n_edge,
           (unsigned long long)n_random, (unsigned long long)mismatches);
    return mismatches ? 1 : 0;
}
