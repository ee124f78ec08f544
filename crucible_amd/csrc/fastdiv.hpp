// fastdiv.hpp -- unsigned 32-bit division by a launch constant without a division: the host turns the divisor into a
// record once, the kernels multiply and shift.  Free of the HIP runtime, so that a plain C++ compiler can check it
// (tests/fastdiv_check.cpp), as it checks tree.hpp.
//
// The round-up scheme of Granlund & Montgomery, "Division by invariant integers using multiplication" (PLDI 1994),
// figure 4.1 with N = 32: for d >= 1 let l = ceil(log2 d) and m = floor(2^32 * (2^l - d) / d) + 1.  Then 2^32 + m is
// the 33-bit multiplier ceil(2^(32 + l) / d) rounded up, and for every n < 2^32
//     t = mulhi(m, n),   n / d = (t + ((n - t) >> sh1)) >> sh2,   sh1 = min(l, 1), sh2 = max(l - 1, 0)
// where n - t never borrows and t + ((n - t) >> sh1) never carries: the 33rd bit is folded into the halved difference.
// Exact for every n in [0, 2^32) and every d in [1, 2^32): d = 1 gives m = 1, t = 0 and both shifts 0 (n itself), a
// power of two gives m = 1, t = 0 and a plain shift by l.
#pragma once
#include "hd.hpp"

#include <stdint.h>

namespace cr {

struct FastDiv {
    uint32_t mul;    // m: the low 32 bits of the 33-bit multiplier
    uint32_t sh1;    // 0 for d = 1, else 1
    uint32_t sh2;    // ceil(log2 d) - 1 (0 for d = 1)
};

// the record of a divisor d >= 1 (host side; d = 0 has no quotient and gets the record of 1)
inline FastDiv fastdiv_make(uint32_t d) {
    if (d == 0) d = 1;
    uint32_t l = 0;
    while (l < 32 && ((uint64_t)1 << l) < d) l++;
    FastDiv f;
    f.mul = (uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 1 ? l - 1 : 0;
    return f;
}

// n / d for the record of d
CR_HD uint32_t fastdiv(uint32_t n, const FastDiv& f) {
    const uint32_t t = (uint32_t)(((uint64_t)f.mul * n) >> 32);   // (one v_mul_hi_u32 on the device)
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

}   // namespace cr
