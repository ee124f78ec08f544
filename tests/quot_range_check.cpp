// Host check for tests/test_quotient_host.py: quot_in_range of crucible_amd/csrc/records.hpp -- the range test of Sphere::hit's
// short quotient, read from the word that holds sign and exponent -- against frexp: 2^-400 <= |x| < 2^400.  Every power of two of
// the format with its two neighbours and a few fractions, both signs; zeros, every kind of subnormal, infinities and NaNs; and
// seeded random bit patterns.  Also: the reciprocal that means "divide" reads as out of range to the guard, and every reciprocal
// of an in-range divisor reads as valid.
// usage: quot_range_check SEED  ->  "cases N mismatches M"
#include "records.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long long cases = 0, bad = 0;

static bool by_frexp(double x) {
    if (!std::isfinite(x) || x == 0.0) return false;
    int e;
    (void)std::frexp(x, &e);   // |x| = m 2^e with 0.5 <= m < 1
    return e >= -399 && e <= 400;
}

static void one(double x) {
    for (int s = 0; s < 2; s++, x = -x) {
        cases++;
        if (cr::quot_in_range(x) != by_frexp(x)) {
            if (bad++ < 10) printf("mismatch at %a: quot_in_range %d, frexp %d\n", x, (int)cr::quot_in_range(x), (int)by_frexp(x));
        }
    }
}

static double from_bits(unsigned long long b) { double x; std::memcpy(&x, &b, 8); return x; }
static unsigned hi_word(double x) { unsigned long long b; std::memcpy(&b, &x, 8); return (unsigned)(b >> 32); }

int main(int argc, char** argv) {
    unsigned long long seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    for (int e = -1074; e <= 1023; e++) {
        const double p = std::ldexp(1.0, e);
        one(p); one(std::nextafter(p, 0.0)); one(std::nextafter(p, INFINITY));
        one(p * 1.5); one(p * 1.9999999999999998);
    }
    one(0.0); one(INFINITY); one(NAN); one(from_bits(0x7ff0000000000001ull)); one(from_bits(0x7fffffffffffffffull));
    one(from_bits(1ull)); one(from_bits(0x00000000ffffffffull)); one(from_bits(0x0000000100000000ull)); one(from_bits(0x000fffffffffffffull));
    for (int i = 0; i < 2000000; i++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        one(from_bits(seed ^ (seed >> 29)));
    }
    // the guard's other operand: max(u, hi(r)) < kQuotSpan << 1 must fail for the sentinel and hold for 2^-400 < r <= 2^400
    const unsigned span2 = cr::kQuotSpan << 1;
    cases += 3;
    if (hi_word(cr::quot_divide<double>()) < span2) { bad++; printf("the sentinel reads as a valid reciprocal\n"); }
    if (!(hi_word(std::ldexp(1.0, 400)) < span2)) { bad++; printf("1 / 2^-400 reads as the sentinel\n"); }
    if (!(hi_word(std::nextafter(std::ldexp(1.0, -400), 1.0)) < span2)) { bad++; printf("the smallest reciprocal reads as the sentinel\n"); }
    printf("cases %llu mismatches %llu\n", cases, bad);
    return 0;
}
