// intersect.hpp -- device only: what a ray meets.  The diagnostic build's Diag and CR_DIAG_* macros, Hit, the
// box tests (Aabb::hit and its min/max form), Sphere::hit and Triangle::hit with the short quotient, the index conversions, and
// the work counters (NoCount, WaveSum, flush_counters).  Included by shade.hpp and walk.hpp; the reference citations are
// pathtrace.hpp's.
#pragma once
#include "records.hpp"

#if defined(__HIPCC__)

namespace cr {

// Diagnostic build (-DCR_DIAG, scripts/diag only): per-lane event counts that the megakernel sums per wave and adds
// to counters[16 + i]; "wave" counts are taken by the first active lane of the wave at that point, "lane" counts by
// every active lane, so lane / (64 * wave) is the lane occupancy of that piece of code.  The product build compiles
// none of it (Diag is empty, CR_DIAG_* expand to nothing).
#ifdef CR_DIAG
enum { DG_BOX_WAVE = 0, DG_BOX_LANE, DG_PRIM_WAVE, DG_PRIM_LANE, DG_ROUND_WAVE, DG_ROUND_LANE, DG_LEAFPH_WAVE, DG_LEAFPH_LANE,
       DG_SHADE_WAVE, DG_SHADE_LANE, DG_LAMB_LANE, DG_METAL_LANE, DG_DIEL_LANE, DG_SKY_LANE, DG_RUV_WAVE, DG_RUV_LANE,
       DG_REGEN_WAVE, DG_REGEN_LANE, DG_OUTER_WAVE, DG_UNWIND_WAVE, DG_UNWIND_LANE, DG_HITSH_WAVE, DG_HITSH_LANE, DG_BAND_WAVE, DG_BAND_LANE,
       DG_ROOT2_WAVE, DG_ROOT2_LANE, DG_QUOT_WAVE, DG_QUOT_LANE, DG_QUOTDIV_WAVE, DG_QUOTDIV_LANE, DG_N };
struct Diag { uint32_t v[DG_N]; };
#define CR_DIAG_LEADER() ((threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)__ballot(1)) - 1))
#define CR_DIAG_HIT(dg, wave_i, lane_i) do { if (dg) { (dg)->v[lane_i]++; if (CR_DIAG_LEADER()) (dg)->v[wave_i]++; } } while (0)
#define CR_DIAG_LANE(dg, lane_i) do { if (dg) (dg)->v[lane_i]++; } while (0)
#else
struct Diag {};
#define CR_DIAG_HIT(dg, wave_i, lane_i) ((void)0)
#define CR_DIAG_LANE(dg, lane_i) ((void)0)
#endif

template <typename real> struct Hit {
    real t;
    int32_t prim;     // leaf-order index, -1 = miss
};

// Aabb::hit (bvh.rs:96-132) with 1/dir hoisted (same value every node).  The per-axis
// early return is folded into one final test: once max <= min holds it keeps holding,
// because new_min >= min and new_max <= max for non-NaN min/max.
template <typename real>
CR_D bool box_hit(const real* b, V3<real> o, V3<real> inv, real tmin, real tmax) {
    real t0 = (b[0] - o.x) * inv.x, t1 = (b[1] - o.x) * inv.x;
    real nmin, nmax;
    if (t0 < t1) { nmin = t0 > tmin ? t0 : tmin; nmax = t1 < tmax ? t1 : tmax; }
    else { nmin = t1 > tmin ? t1 : tmin; nmax = t0 < tmax ? t0 : tmax; }
    tmin = nmin; tmax = nmax;
    t0 = (b[2] - o.y) * inv.y; t1 = (b[3] - o.y) * inv.y;
    if (t0 < t1) { nmin = t0 > tmin ? t0 : tmin; nmax = t1 < tmax ? t1 : tmax; }
    else { nmin = t1 > tmin ? t1 : tmin; nmax = t0 < tmax ? t0 : tmax; }
    tmin = nmin; tmax = nmax;
    t0 = (b[4] - o.z) * inv.z; t1 = (b[5] - o.z) * inv.z;
    if (t0 < t1) { nmin = t0 > tmin ? t0 : tmin; nmax = t1 < tmax ? t1 : tmax; }
    else { nmin = t1 > tmin ? t1 : tmin; nmax = t0 < tmax ? t0 : tmax; }
    return !(nmax <= nmin);
}

// The same test in min/max form on (min,max) pairs, which the compiler maps onto
// v_pk_add_f32 / v_pk_mul_f32.  Identical to box_hit whenever no slab distance is NaN, i.e.
// whenever 1/dir is finite on every axis (then `t0 < t1 ? .. : ..` is min/max of two non-NaN
// numbers and `a > b ? a : b` is max; signed zeros only ever feed comparisons).  Rays with an
// infinite 1/dir component walk with box_hit instead.
template <typename real> using Pair = real __attribute__((ext_vector_type(2)));
CR_D float r_min(float a, float b) { return __builtin_fminf(a, b); }
CR_D float r_max(float a, float b) { return __builtin_fmaxf(a, b); }
CR_D double r_min(double a, double b) { return __builtin_fmin(a, b); }
CR_D double r_max(double a, double b) { return __builtin_fmax(a, b); }
template <typename real>
CR_D bool box_hit_fast(const real* b, Pair<real> ox, Pair<real> oy, Pair<real> oz, Pair<real> ix, Pair<real> iy, Pair<real> iz,
                       real tmin, real tmax) {
    Pair<real> tx = (Pair<real>{b[0], b[1]} - ox) * ix;
    Pair<real> ty = (Pair<real>{b[2], b[3]} - oy) * iy;
    Pair<real> tz = (Pair<real>{b[4], b[5]} - oz) * iz;
    real lo = r_max(r_max(r_min(tx.x, tx.y), r_min(ty.x, ty.y)), r_max(r_min(tz.x, tz.y), tmin));
    real hi = r_min(r_min(r_max(tx.x, tx.y), r_max(ty.x, ty.y)), r_min(r_max(tz.x, tz.y), tmax));
    return !(hi <= lo);
}
// The complement, for callers that combine it with other masks: Aabb::hit's `max <= min -> miss`.
// min(h, tmax) <= lo is evaluated as h <= lo || tmax <= lo: identical for every input the fast path sees (the slab
// distances are never NaN there, and a NaN tmax is ignored by either form), and one instruction shorter because
// v_min would first have to canonicalise tmax.
template <typename real>
CR_D bool box_miss_fast(const real* b, Pair<real> ox, Pair<real> oy, Pair<real> oz, Pair<real> ix, Pair<real> iy, Pair<real> iz,
                        real tmin, real tmax) {
    Pair<real> tx = (Pair<real>{b[0], b[1]} - ox) * ix;
    Pair<real> ty = (Pair<real>{b[2], b[3]} - oy) * iy;
    Pair<real> tz = (Pair<real>{b[4], b[5]} - oz) * iz;
    real lo = r_max(r_max(r_min(tx.x, tx.y), r_min(ty.x, ty.y)), r_max(r_min(tz.x, tz.y), tmin));
    real hi = r_min(r_min(r_max(tx.x, tx.y), r_max(ty.x, ty.y)), r_max(tz.x, tz.y));
    return (hi <= lo) | (tmax <= lo);
}

// Sphere::hit root search (sphere.rs:72-95): returns t or a negative number for a miss.
// The reference divides twice, root1 = (h - sqrtd) / a and, when that one is out of range, root2 = (h + sqrtd) / a.  An
// IEEE division is ~16 VALU instructions and a wave runs the second one as soon as ONE lane asks for it -- and every
// scattered ray starts on the sphere it left, reaches that sphere's leaf and finds both roots near zero there.  So the
// outcome of the second test is decided without dividing wherever that is provable; a lane that still divides computes
// what the reference computes.  With n1 = fl(h - sqrtd), n2 = fl(h + sqrtd), a = |d|^2 (+0 or above, or NaN: a sum of
// squares) and root1 outside (tmin, tmax):
//   Rule A: !(root1 <= tmin) -> miss.  Then root1 > tmin or root1 is NaN.
//     root1 > tmin: the first test failed at its upper end, !(root1 < tmax), so tmax is NaN (every `< tmax` fails) or
//       root1 >= tmax.  sqrtd >= 0 (or -0) gives h - sqrtd <= h + sqrtd exactly, rounding to nearest is monotone, so
//       n2 >= n1, and for a > 0 the rounded quotients keep that order: root2 >= root1 >= tmax.  a subnormal: the quotients
//       may overflow to +inf, which keeps the order.  a = 0: root1 = +inf here, so n2 >= n1 > 0 and root2 = +inf as well.
//       (sqrtd = +inf with a finite h, or h = -inf, give n1 = -inf: root1 <= tmin, not this rule.)
//     root1 NaN: then root2 is NaN or +inf, and neither is below any tmax.  Case by case: a NaN -> root2 NaN.  n1 NaN: h or
//       sqrtd is NaN (a NaN disc passes `disc < 0`) -> n2 NaN; or h = sqrtd = +inf -> n2 = +inf, root2 = +inf (NaN for
//       a = +inf).  n1 = +-0 over a = 0: n2 >= 0, root2 = NaN or +inf.  n1 = +-inf over a = +inf: n2 is +inf or NaN, root2 NaN.
//   Rule B: hi(n2) < hi(a) - 11 * 2^M as signed integers (hi: the word holding sign and exponent, M: the exponent's bit
//     position in it) -> miss, valid for tmin >= 2^-10; tmin is 0.001 in every walk.  a is not NaN here (rule A took it).
//     hi(n2) < 0: n2 is negative, -0 or a negative NaN, and n2 / a is negative, -0, -inf or NaN for every a >= +0.
//     hi(n2) >= 0: then hi(a) > hi(n2) + 11 * 2^M, so a >= 2^11 * the smallest normal and n2 is finite and not NaN.  Let v
//       be n2 with 11 added to its exponent field: v = 2^11 n2 for a normal n2 and v >= 2^11 n2 for a subnormal or zero
//       one ((1 + m) 2^e >= 2 m 2^e for a fraction m < 1).  hi(v) < hi(a), both non-negative, gives v < a, so exactly
//       n2 / a < 2^-11, the rounded quotient is <= 2^-11 < tmin, and `tmin < root2` fails (a = +inf: root2 = 0).
//     No product is formed, so nothing underflows.  (`n2 > 0` alone is provable in a line but is not enough: on the sphere
//     a ray leaves, n2 is rounding noise of either sign, and one lane that asks is enough to run the division for the wave.)
// tests/sphere_roots_check.hip compares this with the two divisions written out, on the device.
CR_D bool root2_below_tmin(double n2, double a, double tmin) {
    if (!(tmin >= 0x1.0p-10)) return false;
    const int32_t hn = (int32_t)((uint64_t)__double_as_longlong(n2) >> 32), ha = (int32_t)((uint64_t)__double_as_longlong(a) >> 32);
    return hn < ha - (11 << 20);
}
CR_D bool root2_below_tmin(float n2, float a, float tmin) {
    if (!(tmin >= 0x1.0p-10f)) return false;
    return __float_as_int(n2) < __float_as_int(a) - (11 << 23);
}
// Sphere::hit's quotients with one reciprocal per path segment (f64 kernels; SHARED below).  Both roots divide by a = |d|^2,
// the same number for every sphere a segment tests, and the compiler's IEEE division refines 1/a again each time:
//     s0 = div_scale(a, a, n)   s1 = div_scale(n, a, n)               (the operands, scaled by 2^+-128 near the range's ends)
//     r0 = rcp(s0)   e0 = fma(-s0, r0, 1)   r1 = fma(r0, e0, r0)   e1 = fma(-s0, r1, 1)   r = fma(r1, e1, r1)
//     q  = s1 * r    m  = fma(-s0, q, s1)   div_fmas(m, r, q)  [= fma(m, r, q), rescaled when s1 was]   div_fixup(., a, n)
// For 2^-400 <= a < 2^400 and 2^-400 <= |n| < 2^400 neither div_scale scales (they do so for a subnormal operand, an exponent
// of n at most 2^-970, one of a beyond 2^+-1021 or a difference of the two beyond 768 or towards a subnormal quotient -- all at
// least 200 binades away), so s0 = a, s1 = n; div_fmas is the plain FMA; and div_fixup, which replaces the value for NaN, zero
// and infinite operands and for an exponent difference beyond the format, only puts sign(n) ^ sign(a) on |value| -- the sign it
// has: 2^-800 < |n / a| < 2^800 is an ordinary number and so is every intermediate.  Then r depends on a alone,
//     shared_rcp(a) = r,       n / a = fma(fma(-a, q, n), r, q)  with  q = n * r,
// the same operations on the same operands in the same order, hence the same bits: three instructions for twelve
// (tests/quotient_check.hip compares the two on the device, 2^22 pairs and the edges of the range; the first comparison, over
// 2^24 pairs, is in profiles/experiments/r03_small_experiments.txt).
//   operand                         short form would give          n / a gives            so the wave
//   |n| or a in [2^-400, 2^400)     the bits of n / a              --                     takes the short form
//   n = +0                          +0 (0 r = 0, m = +0, +0)       +0                     divides: the guard reads the word
//   n = -0                          +0 (m = fma(-a, -0, -0) = +0)  -0                       with sign and exponent only, where
//   n subnormal                     not proven (s1 is scaled)      the quotient             +-0 and a subnormal are one value
//   n = +-inf, NaN                  NaN (inf - inf in m)           +-inf, NaN             divides
//   |n| outside the range           not proven                     the quotient           divides
//   a = 0, subnormal, +inf, NaN,    r is the sentinel              NaN, +-inf, +-0 or     divides
//     or outside the range                                           the quotient
// A zero numerator is not rare enough to ignore and not worth a third instruction: n1 = h - sqrtd is rounding noise around zero
// on the sphere a refracted ray enters from (section 3.8 of DESIGN.md), exactly 0 there now and then; only its sign would differ
// (-0 for +0 -- invisible to `tmin < root`, `root <= tmin` and `root < tmax`, and t_out is never a zero), but the helper promises the
// bits of n / a, so a zero divides.  The -DCR_DIAG build counts the wave-level quotients and those that divided
// (profiles/experiments/shared_reciprocal_ab.txt has the share).
// The guard is wave-uniform like r_sqrt's: one active lane outside the range sends the wave to `/`, which is right for every
// operand.  Per lane it is two integer instructions and a compare: u = (hi(n) << 1) - (0x26f00000 << 1) drops n's sign and is
// below 800 << 21 exactly for an exponent field in [1023 - 400, 1023 + 400); max(u, hi(r)) folds the sentinel in, because a
// valid r lies in (2^-400, 2^400] -- hi(r) <= 0x58f00000 < 800 << 21 = 0x64000000 -- and the sentinel, a NaN, has hi = 0x7ff80000.
// (kQuotLo, kQuotSpan, quot_in_range and quot_divide stand with r_sqrt at the top of the file: the host can compile them)
CR_D double shared_rcp(double a) {
    double r = __builtin_amdgcn_rcp(a);
    r = __builtin_fma(r, __builtin_fma(-a, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-a, r, 1.0), r);
    return quot_in_range(a) ? r : quot_divide<double>();
}
CR_D float shared_rcp(float) { return quot_divide<float>(); }
// n / a, bit for bit; r = shared_rcp(a) or quot_divide().  SHARED = false is the division alone.
template <bool SHARED>
CR_D double sphere_quot(double n, double a, double r, Diag* dg = nullptr) {
    if constexpr (SHARED) {
        CR_DIAG_HIT(dg, DG_QUOT_WAVE, DG_QUOT_LANE);
        typedef uint32_t Words __attribute__((ext_vector_type(2)));   // (the high word as a register of its own, not a 64-bit shift)
        const uint32_t hn = __builtin_bit_cast(Words, n).y, hr = __builtin_bit_cast(Words, r).y;
        const uint32_t u = (hn << 1) - (kQuotLo << 1);
        const bool ok = (u > hr ? u : hr) < (kQuotSpan << 1);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) == 0ull, 1)) {
            const double q = n * r;
            return __builtin_fma(__builtin_fma(-a, q, n), r, q);
        }
        CR_DIAG_HIT(dg, DG_QUOTDIV_WAVE, DG_QUOTDIV_LANE);
        // (two empty statements the compiler cannot move, around this division: without them it computes both forms in every
        // test and selects one)
        asm volatile("" : "+v"(n));
        double q = n / a;
        asm volatile("" : "+v"(q));
        return q;
    }
    return n / a;
}
template <bool SHARED>
CR_D float sphere_quot(float n, float a, float, Diag* = nullptr) { return n / a; }

// RULE_B = false keeps rule A alone: the extra exit costs the f64 kernels that read their tree from global memory (RES_GLOBAL,
// RES_TOP) two VGPR spills in the shading code, and the frames that run them and test few or no spheres lost 0.6-1.1 %
// (teapot, the orbit movie; profiles/experiments/decided_early_ab.txt), so walk_round asked for rule B in the RES_LDS kernels only.
// Since the f64 kernels without keyed primitives stopped spilling (profiles/experiments/uniform_and_decode_ab.txt) they take
// rule B under every residency; in the f32 kernels below the LDS window it would cost a wave per SIMD, in the keyed f64 ones spills.
// SHARED: the two quotients go through sphere_quot with ra = shared_rcp(a) (WalkState::rda); without it, or with the default
// ra, they are the divisions.
template <bool RULE_B = true, bool SHARED = false, typename real>
CR_D bool sphere_t(real cx, real cy, real cz, real radius, V3<real> o, V3<real> d, real a /* |d|^2 */, real tmin, real tmax, real& t_out,
                   Diag* dg = nullptr, real ra = quot_divide<real>()) {
    V3<real> oc = sub(mk<real>(cx, cy, cz), o);
    real h = dot(d, oc);
    real c = len2(oc) - radius * radius;
    real disc = h * h - a * c;
    if (disc < real(0)) return false;
    real sqrtd = r_sqrt(disc);
    real root = sphere_quot<SHARED>(h - sqrtd, a, ra, dg);
    if (!(tmin < root && root < tmax)) {
        if (!(root <= tmin)) return false;                 // rule A
        const real n2 = h + sqrtd;
        if (RULE_B && root2_below_tmin(n2, a, tmin)) return false;   // rule B
        CR_DIAG_HIT(dg, DG_ROOT2_WAVE, DG_ROOT2_LANE);
        root = sphere_quot<SHARED>(n2, a, ra, dg);
        if (!(tmin < root && root < tmax)) return false;
    }
    t_out = root;
    return true;
}

// Triangle::hit up to t (triangle.rs:95-123)
template <typename real>
CR_D bool triangle_t(V3<real> a, V3<real> b, V3<real> c, V3<real> o, V3<real> d, real tmin, real tmax, real& t_out) {
    V3<real> e1 = sub(b, a), e2 = sub(c, a);
    V3<real> rce2 = cross(d, e2);
    real det = dot(e1, rce2);
    if (det > -RealTraits<real>::eps && det < RealTraits<real>::eps) return false;
    real inv_det = real(1) / det;
    V3<real> s = sub(o, a);
    real u = inv_det * dot(s, rce2);
    if (!(real(0) <= u && u <= real(1))) return false;
    V3<real> sce1 = cross(s, e1);
    real v = inv_det * dot(d, sce1);
    if (v < real(0) || u + v > real(1)) return false;
    real t = inv_det * dot(e2, sce1);
    if (!(tmin < t && t < tmax)) return false;
    t_out = t;
    return true;
}

// Rust `as i32`: truncation toward zero, saturating, NaN -> 0 -- which is what v_cvt_i32_f32 / v_cvt_i32_f64 do (ISA: out-of-range
// values and infinities saturate, NaN converts to 0).  Written as the instruction: C++'s cast is undefined out of range, and the
// guarded form costs three compares and their branches per conversion (the checker texture makes three per hit).
// tests/sqrt_check.hip compares it with as_i32_reference on the device.
template <typename real> CR_HD int32_t as_i32_reference(real x) {
    if (!(x == x)) return 0;
    if (x <= real(-2147483648.0)) return INT32_MIN;
    if (x >= real(2147483647.0)) return INT32_MAX;
    return (int32_t)x;
}
CR_D int32_t as_i32(float x) { int32_t r; asm("v_cvt_i32_f32_e32 %0, %1" : "=v"(r) : "v"(x)); return r; }
CR_D int32_t as_i32(double x) { int32_t r; asm("v_cvt_i32_f64_e32 %0, %1" : "=v"(r) : "v"(x)); return r; }
template <typename real> CR_D uint32_t as_index(real x, int32_t n) {   // `as usize` then clamp to n-1 (img_loader.rs:72-73)
    if (!(x == x) || x <= real(0)) return 0;
    if (x >= (real)n) return (uint32_t)(n - 1);
    return (uint32_t)x;
}

// The work counters of a kernel that keeps none (pathtrace_body's COUNT == false): no storage, and every ++ and +=
// compiles away.  image_lookup, shade and walk_round take their counters' types as they come.
struct NoCount {
    CR_D void operator++(int) {}
    template <typename T> CR_D void operator+=(T) {}
};

// A kernel's end: its work counters, summed over the wave, into KernelArgs::counters -- one atomic per counter per wave:
// flush_counters(WaveSum{}, A.counters, lane, c_seg, c_node, c_prim, c_tex).  A counter of type NoCount is one the kernel
// does not keep: no sum and no atomic for it.
// (The caller creates the wave sum, a function object: with a plain function, or the object made in here, the megakernels'
// registers are initialised in another order -- the same instructions, not the same text; scripts/isa_diff.py.)
struct WaveSum {
    __device__ unsigned long long operator()(unsigned long long v) const {
        unsigned long long s = v;
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        return s;
    }
    __device__ NoCount operator()(NoCount) const { return {}; }
};
CR_D void add_counter(uint64_t* counter, unsigned long long s) { atomicAdd((unsigned long long*)counter, s); }
CR_D void add_counter(uint64_t*, NoCount) {}
template <typename C0, typename C1, typename C2, typename C3>
CR_D void flush_counters(const WaveSum& wave_sum, uint64_t* counters, uint32_t lane, C0 c_seg, C1 c_node, C2 c_prim, C3 c_tex) {
    const auto s0 = wave_sum(c_seg);
    const auto s1 = wave_sum(c_node);
    const auto s2 = wave_sum(c_prim);
    const auto s3 = wave_sum(c_tex);
    if (lane == 0) { add_counter(&counters[0], s0); add_counter(&counters[1], s1); add_counter(&counters[2], s2); add_counter(&counters[3], s3); }
}

}   // namespace cr

#endif   // __HIPCC__
