// walk.hpp -- device only: the stackless BVH walk.  Reads of a wrapper from LDS or global memory, the
// screened box steps of the f64 kernels, WalkState and the headline kernels' WalkOffset, walk_begin / walk_begin_screened, the
// experiment switches of the sphere test (CR_QUOT_FORM, CR_SPHERE_LOOP, CR_SHADE_DD, CR_LAZY_INV) and of the work around the
// box step (CR_WALK_OFFSET, CR_WALK_PRIO), and walk_round, which every pipeline and the guide pass call.
// Its text has been settled against the register allocator: an edit is held to compiling every kernel it does
// not mean to change to the code it had (scripts/kernel_resources.py and the ISA tests; DESIGN.md 3.13 for the last one).
#pragma once
#include "intersect.hpp"

#if defined(__HIPCC__)

namespace cr {

// RES_TOP reads a wrapper from the LDS window or from global memory.  A select between the two pointers compiles to
// one flat_load, which is unordered against both counters (every use waits for vmcnt(0) and lgkmcnt(0)) and pays the
// aperture check; loads through address-space-qualified pointers in the two arms of a branch compile to ds_read and
// global_load.  Measured on one box, f64: the 1M-sphere frame +8 %, the movie frame +2 %, the teapot +1 %.
template <typename T> using LdsPtr = const __attribute__((address_space(3))) T*;
template <typename T> using GlobPtr = const __attribute__((address_space(1))) T*;
template <typename real, int RES>
CR_D Entry<real> fetch_entry(const Entry<real>* lds, const Entry<real>* glob, int32_t lds_entries, int32_t idx) {
    if (RES == RES_LDS) return lds[idx];
    if (RES == RES_TOP) {
        Entry<real> e;
        if (idx < lds_entries) {
            const Entry<real>* s = lds + idx;
            LdsPtr<real> b = (LdsPtr<real>)s->b;
            for (int k = 0; k < 6; k++) e.b[k] = b[k];
            e.skip = *(LdsPtr<int32_t>)&s->skip; e.leaf = *(LdsPtr<int32_t>)&s->leaf;
        } else {
            const Entry<real>* s = glob + idx;
            GlobPtr<real> b = (GlobPtr<real>)s->b;
            for (int k = 0; k < 6; k++) e.b[k] = b[k];
            e.skip = *(GlobPtr<int32_t>)&s->skip; e.leaf = *(GlobPtr<int32_t>)&s->leaf;
        }
        return e;
    }
    return glob[idx];
}
// The ordered layout read into the same record: skip = the link of the ray's octant.
template <typename real, int RES>
CR_D Entry<real> fetch_entry_ordered(const Entry<real>* lds, const Entry<real>* glob, int32_t lds_entries, int32_t idx, int32_t oct) {
    auto rd = [&](const EntryO<real>* p) {
        const EntryO<real>& s = p[idx];
        Entry<real> e;
        for (int k = 0; k < 6; k++) e.b[k] = s.b[k];
        e.leaf = s.leaf;
        e.skip = s.skip[oct];
        return e;
    };
    if (RES == RES_LDS) return rd((const EntryO<real>*)lds);
    if (RES == RES_TOP) {
        Entry<real> e;
        if (idx < lds_entries) {
            const EntryO<real>* s = (const EntryO<real>*)lds + idx;
            LdsPtr<real> b = (LdsPtr<real>)s->b;
            for (int k = 0; k < 6; k++) e.b[k] = b[k];
            e.leaf = *(LdsPtr<int32_t>)&s->leaf; e.skip = ((LdsPtr<int32_t>)s->skip)[oct];
        } else {
            const EntryO<real>* s = (const EntryO<real>*)glob + idx;
            GlobPtr<real> b = (GlobPtr<real>)s->b;
            for (int k = 0; k < 6; k++) e.b[k] = b[k];
            e.leaf = *(GlobPtr<int32_t>)&s->leaf; e.skip = ((GlobPtr<int32_t>)s->skip)[oct];
        }
        return e;
    }
    return rd((const EntryO<real>*)glob);
}

// A kernel that holds ALL screening records in LDS (RES_LDS) rewrites the links of its copy into LDS addresses while staging
// it, so that the walk's position is the address of the next ds_read as it stands: the address the copy starts at.
template <int RES> CR_D uint32_t screen_lds_base(const void* lds) { return RES == RES_LDS ? (uint32_t)(uintptr_t)(LdsPtr<char>)lds : 0u; }
// A screening record by its byte offset, from the LDS copy or from global memory (RES_TOP: the LDS window holds the first
// lds_bytes of the array).
template <int RES>
CR_D ScreenEntry fetch_screen(const ScreenEntry* lds, const ScreenEntry* glob, uint32_t lds_bytes, uint32_t off) {
    static_assert(sizeof(ScreenEntry) == 32, "offsets are index << 5");
    typedef uint32_t Quad __attribute__((ext_vector_type(4)));   // 16-byte aligned: two ds_read_b128 / global_load_dwordx4
    if (RES == RES_LDS) {   // the staged copy holds LDS addresses (screen_lds_base): `off` is one
        ScreenEntry e;
        Quad* o = reinterpret_cast<Quad*>(&e);
        LdsPtr<Quad> s = (LdsPtr<Quad>)(uintptr_t)off;
        o[0] = s[0]; o[1] = s[1];
        return e;
    }
    if (RES == RES_TOP) {
        ScreenEntry e;
        Quad* o = reinterpret_cast<Quad*>(&e);
        if (off < lds_bytes) {
            LdsPtr<Quad> s = (LdsPtr<Quad>)(const void*)((const char*)lds + off);
            o[0] = s[0]; o[1] = s[1];
        } else {
            GlobPtr<Quad> s = (GlobPtr<Quad>)(const void*)((const char*)glob + off);
            o[0] = s[0]; o[1] = s[1];
        }
        return e;
    }
    return *(const ScreenEntry*)((const char*)glob + off);
}

// The ordered layout's screening record by its byte offset: the box, {axis, hit} and the skip link of the ray's octant
// (octoff = 32 + 4 * octant, the byte offset of skip[octant] in the record).
struct ScreenStepO { float b[6]; uint32_t axis, hit, skip; };
template <int RES>
CR_D ScreenStepO fetch_screen_ordered(const ScreenEntryO* lds, const ScreenEntryO* glob, uint32_t lds_bytes, uint32_t off, uint32_t octoff) {
    static_assert(sizeof(ScreenEntryO) == 64, "offsets are index << 6");
    typedef uint32_t Quad __attribute__((ext_vector_type(4)));
    ScreenStepO e;
    Quad q0, q1;
    if (RES == RES_LDS) {   // the staged copy holds LDS addresses: `off` is one
        LdsPtr<Quad> s = (LdsPtr<Quad>)(uintptr_t)off;
        q0 = s[0]; q1 = s[1];
        e.skip = *(LdsPtr<uint32_t>)(uintptr_t)(off + octoff);
    } else if (RES == RES_TOP && off < lds_bytes) {
        LdsPtr<Quad> s = (LdsPtr<Quad>)(const void*)((const char*)lds + off);
        q0 = s[0]; q1 = s[1];
        e.skip = *(LdsPtr<uint32_t>)(const void*)((const char*)lds + off + octoff);
    } else {
        GlobPtr<Quad> s = (GlobPtr<Quad>)(const void*)((const char*)glob + off);
        q0 = s[0]; q1 = s[1];
        e.skip = *(GlobPtr<uint32_t>)(const void*)((const char*)glob + off + octoff);
    }
    uint32_t w[8];
    __builtin_memcpy(w, &q0, 16); __builtin_memcpy(w + 4, &q1, 16);
    for (int k = 0; k < 6; k++) e.b[k] = __builtin_bit_cast(float, w[k]);
    e.axis = w[6]; e.hit = w[7];
    return e;
}

// The per-ray state of BVHWrapper::hit's walk, kept in registers so a walk can be suspended and resumed.
// What walk_begin_screened alone fills (the f64 kernels of lazy_inv(), which neither make nor read `inv` and `exact_box`);
// an f32 walk has no such form and carries no such fields
template <typename real> struct WalkScreened {};
template <> struct WalkScreened<double> {
    V3<float> invf;      // the screen's f32 1/direction (`if` in the derivation above screen_extents)
    bool unscreened;     // the ray is outside screen_in_range: every step is Aabb::hit's compare/select form on the f64 record
};
template <typename real> struct WalkState : WalkScreened<real> {
    V3<real> inv;        // 1 / direction
    real dd;             // |direction|^2: Sphere::hit's `a`, the same for every sphere of the segment
    real rda;            // shared_rcp(dd) in the kernels that share it (quot_form() == 1), quot_divide() in the others
    real best_t;         // closest hit so far = the interval's max handed to the next wrapper
    int32_t best;        // leaf-order index of that primitive, -1 = none
    int32_t idx;         // next wrapper to visit; n_entries = walk finished
    bool exact_box;      // an infinite 1/dir component: Aabb::hit's compare/select form is required
    int32_t oct;         // ordered walk: bit a set when direction[a] < 0
    int32_t pending;     // a leaf wrapper whose box was hit and whose primitives are still to be tested (-1: none)
};

// The state of the kernels of walk_offset() (the headline's two: static f64, relaxed sums, screening records of an unordered tree,
// the whole scene in LDS): the position is `off`, the LDS address of the next screening record as fetch_screen<RES_LDS> reads
// it, carried across rounds and outer iterations; screen_lds_base + (n_entries << 5) = walk finished.  An index is made of it
// only where one is read: the band branch's f64 fetch and the compare/select loop.  No `inv`, `exact_box` or `oct`: a
// LAZY_INV walk of an unordered tree reads none of them.
struct WalkOffset : WalkScreened<double> {
    double dd, rda, best_t;   // as WalkState's
    int32_t best;
    uint32_t off;             // next record to visit, an LDS address
    int32_t pending;
    static constexpr int32_t oct = 0;   // (named by walk_round's ordered reads, which these kernels do not compile)
};

// A state that walks nothing, every field set; `idx`: the kernel's own "no walk" (n_entries where walk_round may see the state
// before a walk_begin).  The cross-check pipelines and the walk check programs begin with it; pathtrace_body and aov_body keep
// lines of their own that leave unset what their kernels never read: setting that too changes the ordered kernels' code (6.8b).
template <typename real> CR_D void walk_reset(WalkState<real>& ws, int32_t idx) {
    ws.inv = mk<real>(0, 0, 0); ws.dd = 0; ws.rda = quot_divide<real>(); ws.best_t = 0; ws.best = -1; ws.idx = idx; ws.exact_box = false; ws.oct = 0; ws.pending = -1;
    if constexpr (std::is_same<real, double>::value) { ws.invf = mk<float>(0, 0, 0); ws.unscreened = false; }
}
// KernelArgs::exact_boxes, for the kernels that can meet such a tree: the f64 kernels compile to what they were
CR_D bool tree_walks_exact(const KernelArgs<float>& A) { return A.exact_boxes != 0; }
CR_D constexpr bool tree_walks_exact(const KernelArgs<double>&) { return false; }

template <bool SHARED = false, typename real> CR_D void walk_begin(WalkState<real>& w, V3<real> rd, bool exact_tree = false) {
    w.inv = mk<real>(real(1) / rd.x, real(1) / rd.y, real(1) / rd.z);
    // 1/dir infinite on some axis (zero or denormal component): slab distances can be NaN, where only the
    // compare/select form reproduces Aabb::hit; exact_tree: a box plane can be (tree_walks_exact)
    w.exact_box = exact_tree || (r_abs(w.inv.x) == r_inf(real(0))) || (r_abs(w.inv.y) == r_inf(real(0))) || (r_abs(w.inv.z) == r_inf(real(0)));
    w.dd = len2(rd);
    w.rda = SHARED ? shared_rcp(w.dd) : quot_divide<real>();
    w.idx = 0; w.best_t = r_inf(real(0)); w.best = -1; w.pending = -1;
    w.oct = (rd.x < real(0) ? 1 : 0) | (rd.y < real(0) ? 2 : 0) | (rd.z < real(0) ? 4 : 0);
}
// The same for the f64 SCREEN kernels of lazy_inv(): the screen's f32 1/direction without the three IEEE divisions, and the
// ray's classification, once per segment (screen_inv, above screen_q, has the argument).  `inv` and `exact_box` are left as they
// are: walk_round<..., LAZY_INV = true> reads neither, and divides 1.0 / rd itself where Aabb::hit's f64 form runs.
template <bool SHARED = false, typename real> CR_D void walk_begin_screened(WalkState<real>& w, V3<real> ro, V3<real> rd);
// `start`: the address of the tree's first record (screen_lds_base of the staged copy)
template <bool SHARED = false> CR_D void walk_begin_screened(WalkOffset& w, V3<double> ro, V3<double> rd, uint32_t start);

// One round of the while-while walk for the lanes with `walking` set: step through wrappers in the reference's
// order (left child on a box hit, skip link on a miss) until the lane reaches a leaf wrapper, runs out of wrappers
// or has made `budget` steps (0 = unbounded); then the lanes parked on a leaf intersect its primitives together.
// Per lane this is exactly BVHWrapper::hit's sequence (bvhwrapper.rs:96-126); the round structure only decides
// when lanes wait for each other.
// ORD: the ordered layout (EntryO behind the same pointers) -- near child first, per-octant skip links.
// SCREEN kernels walk on the 32-byte ScreenEntry (64-byte ScreenEntryO) records: byte-offset links in the form the loop consumes.
// f32 kernels (unordered trees): the record holds the wrapper's own box and the test on it is Aabb::hit (EXACT below).
// f64 kernels: Aabb::hit decided on the f32 screening record wherever f32 can decide it:
// Notation: b, o, inv = an f64 box plane, the origin component and 1/direction on that axis; bf, of, if their f32
// roundings; u = 2^-24; T = (b - o) * inv; p = fl(of * if), computed once per ray; t32 = fl(bf * if - p), one FMA, the
// f32 slab distance (the screen is the project's own estimate, not the reference's arithmetic: the parity rule's
// -ffp-contract=off does not bind it, the bound below does).  For normal f32 values write bf = b (1 + B), of = o (1 + W),
// if = inv (1 + I), p = of if (1 + P) and t32 = x (1 + F) with x = bf if - p exact inside the FMA; |B|, |W|, |I|, |P|,
// |F| <= u.  Then
//     x - T = b inv (B + I + B I) - o inv (W + I + P + W I + W P + I P + W I P)
//     |x - T| <= (2u + u^2) |b inv| + (3u + 3u^2 + u^3) |o inv|,    |t32 - x| <= u |t32|       (round to nearest)
// and with |b inv| <= |T| + |o inv| and |T| <= |t32| + E, E = |t32 - T|:  E (1 - 2u - u^2) <= (3u + u^2) |t32| +
// (5u + 4u^2 + u^3) |o inv|, i.e.
//     |t32 - T| <= 3.01 u |t32| + 5.02 u |p|         (|o inv| <= (1 + 3.01 u) |p|; the f64 test's own roundings, 2^-52 |T|,
//                                                     vanish in the slack).
// Below the normal f32 range each rounding errs by at most 2^-150 absolutely instead: bf and of add 2^-150 |if| each to
// |x - T| (times 1 + 2u), p and the FMA 2^-150 each -- per slab at most 2^-149 (|if| + 1) (1 + 3u).
// lo32 = max(nears, 0.001) and hi32 = min(fars, tmax32) (min and max are exact): if operand i wins in f32 and j in f64,
// lo32 - lo <= E_i and lo - lo32 <= E_j with |t32_j| <= |lo32| + E_i + E_j, so each end errs by the bound above in
// |lo32| resp. |hi32| (to first order in u; an end that is 0.001 or tmax32 was rounded once, u |end|, which is less).  A
// slab distance that overflows is +-inf on the side of T: it loses to a finite end on both sides, or makes M infinite.
// The subtraction hi32 - lo32 rounds once more (u |hi32 - lo32| <= 2u M).  With M = max(|lo32|, |hi32|) and
// Q = max over the axes of |p|:
//     |(hi32 - lo32) - (hi - lo)| <= (2 * 3.01 + 2) u M + 2 * 5.02 u Q + 2^-148 (max |if| + 1)  =  8.02 u M + 10.04 u Q + ...
// and 1.5 times that is 12.03 u M + 15.06 u Q + 1.5 * 2^-148 (max |if| + 1).  The kernel uses
//     TH = 2^-20 M + 2^-20 Q + 2^-147 max |if| + 1e-35
// (16u M and 16u Q, each rounded in f32 at most twice: >= 15.99u; 2^-147 = 4 * 2^-149 > 1.5 * 2^-148; 1e-35 covers the rest,
// and the 2^-147 term itself where it underflows).  A product p beyond the f32 range is inf: then TH = inf and every
// test of the ray lands in the band.  Hence hi32 - lo32 < -TH proves Aabb::hit's
// `max <= min` (a miss), hi32 - lo32 > TH proves a hit, and only a lane with |hi32 - lo32| <= TH evaluates Aabb::hit in f64
// on the f64 box.  Overflow and NaN land there too (every comparison with them is false), and the round uses the screen only
// when |if| lies in [2^-100, 2^100] and |of| <= 2^100 on every axis, on trees whose f64 planes all lie in the f32 range
// (screen_from_entries_kernel reports any other; render.hip then walks without the screen).  The decisions -- hence the walk, the counters and the image -- are those of the f64 test.
// SCREEN is a kernel variant of its own: a kernel that carried both the f32 loop and the f64 min/max loop lost 5 % on the
// teapot frames to register pressure.  In a SCREEN kernel a ray whose
// 1/direction is infinite, or outside the f32 range above, walks with Aabb::hit's compare/select form (valid for every ray).
// The screen's pieces, one record at a time (tests/walk_check.hip runs them on the device).  of*, if*: the f32 roundings of
// the origin and of 1/direction; mo = max |of|, pmax / pmin = max / min |if|.  screen_in_range: a ray the f64 screen may decide
// (finite 1/direction, and the range above); screen_th0: from Q's three terms screen_q, the part of TH
// that does not depend on the box -- 2^-20 Q, plus what rounding a box plane or an origin component BELOW the normal f32
// range can add (2^-150 each, times |if| <= 2^100), plus a product or an FMA that underflows.
CR_D void screen_extents(float ofx, float ofy, float ofz, float ifx, float ify, float ifz, float& mo, float& pmax, float& pmin) {
    mo = r_max(r_max(__builtin_fabsf(ofx), __builtin_fabsf(ofy)), __builtin_fabsf(ofz));
    pmax = r_max(r_max(__builtin_fabsf(ifx), __builtin_fabsf(ify)), __builtin_fabsf(ifz));
    pmin = r_min(r_min(__builtin_fabsf(ifx), __builtin_fabsf(ify)), __builtin_fabsf(ifz));
}
CR_D bool screen_in_range(bool exact_box, float mo, float pmax, float pmin) {
    return !exact_box && pmin >= 0x1.0p-100f && pmax <= 0x1.0p100f && mo <= 0x1.0p100f;
}
// The f64 SCREEN kernels of lazy_inv() begin a walk with walk_begin_screened, which makes `if` without the IEEE division:
//     r0 = v_rcp_f64(d),    r1 = fma(r0, fma(-d, r0, 1), r0),    if = (float)r1.
// The derivation above takes if = inv (1 + I) with |I| <= u and rounds its constants up: 3.01u and 5.02u stand for 3u + u^2 and
// 5u + 4u^2 + u^3 over 1 - 2u - u^2, i.e. for 3.0000004u and 5.0000007u.  With r1 = inv (1 + R) the rounding to f32 gives
// |I| <= u + |R| (1 + u), which enters the bound wherever I does: at most twice in E's |t32| term and |o inv| term (B + I + B I,
// W + I + P + ...).  2 |R| (1 + u) <= 0.009u, i.e. |R| <= 0.0045u = 2^-31.8, keeps both constants below 3.01u and 5.02u, so TH
// stands as it is.  v_rcp_f64 is an approximation, not the rounded reciprocal (the compiler's own division refines it twice
// before it trusts it); with r0 = inv (1 - e0) one Newton step gives r1 = inv (1 - e0^2) before its own two roundings of 2^-53
// each, so |e0| <= 2^-21 is all the requirement asks of the instruction.  No published precision of the instruction is relied
// on here: that the device meets the requirement is an empirical guarantee, the test's.  tests/test_gpu_screen_inv.py holds it to
// |r1 d - 1| <= 2^-40 over every binade of the range, 2^8 under the requirement (measured: 2^-48.7 at worst, and (float)r1
// equal to (float)(1.0 / d) for each of 3 * 10^6 components).  Outside the range nothing is asked of r1
// but to leave the range: a zero, subnormal, infinite or NaN component makes r0 infinite, zero or NaN and r1 NaN or infinite
// (inf - inf, 0 * inf inside the step), |d| beyond 2^+-100 makes |r1| leave [2^-100, 2^100] with it, and every comparison below
// is false for a NaN.  Such a ray takes Aabb::hit's compare/select form on the f64 records, with 1.0 / d divided where that form
// runs (walk_round's LAZY_INV): valid for every ray, so a ray within rounding of the range's ends may fall on either side.
CR_D double screen_rcp1(double d) {   // r1
    const double r0 = __builtin_amdgcn_rcp(d);
    return __builtin_fma(r0, __builtin_fma(-d, r0, 1.0), r0);
}
CR_D float screen_inv(double d) { return (float)screen_rcp1(d); }
CR_D float screen_inv(float d) { return 1.0f / d; }   // (never used: the f32 kernels' record is the box itself)
CR_D bool screen_in_range_lazy(float mo, float ifx, float ify, float ifz) {
    const float ax = __builtin_fabsf(ifx), ay = __builtin_fabsf(ify), az = __builtin_fabsf(ifz);
    return ax >= 0x1.0p-100f && ax <= 0x1.0p100f && ay >= 0x1.0p-100f && ay <= 0x1.0p100f && az >= 0x1.0p-100f && az <= 0x1.0p100f &&
           mo <= 0x1.0p100f;
}
CR_D float screen_q(float of, float inv_f) { return __builtin_fabsf(of * inv_f); }   // |of if| on one axis
CR_D float screen_th0(float qx, float qy, float qz, float pmax) {
    return __builtin_fmaf(0x1.0p-20f, r_max(r_max(qx, qy), qz), __builtin_fmaf(pmax * 0x1.0p-100f, 0x1.0p-47f, 1e-35f));
}
template <bool SHARED, typename real> CR_D void walk_begin_screened(WalkState<real>& w, V3<real> ro, V3<real> rd) {
    static_assert(std::is_same<real, double>::value, "the f32 kernels' record is the wrapper's own box: they begin with walk_begin");
    w.invf = mk<float>(screen_inv(rd.x), screen_inv(rd.y), screen_inv(rd.z));
    const float mo = r_max(r_max(__builtin_fabsf((float)ro.x), __builtin_fabsf((float)ro.y)), __builtin_fabsf((float)ro.z));
    w.unscreened = !screen_in_range_lazy(mo, w.invf.x, w.invf.y, w.invf.z);
    w.dd = len2(rd);
    w.rda = SHARED ? shared_rcp(w.dd) : quot_divide<real>();
    w.idx = 0; w.best_t = r_inf(real(0)); w.best = -1; w.pending = -1;
    w.oct = (rd.x < real(0) ? 1 : 0) | (rd.y < real(0) ? 2 : 0) | (rd.z < real(0) ? 4 : 0);
}
template <bool SHARED> CR_D void walk_begin_screened(WalkOffset& w, V3<double> ro, V3<double> rd, uint32_t start) {
    w.invf = mk<float>(screen_inv(rd.x), screen_inv(rd.y), screen_inv(rd.z));
    const float mo = r_max(r_max(__builtin_fabsf((float)ro.x), __builtin_fabsf((float)ro.y)), __builtin_fabsf((float)ro.z));
    w.unscreened = !screen_in_range_lazy(mo, w.invf.x, w.invf.y, w.invf.z);
    w.dd = len2(rd);
    w.rda = SHARED ? shared_rcp(w.dd) : quot_divide<double>();
    w.off = start; w.best_t = r_inf(0.0); w.best = -1; w.pending = -1;
}
// f64 kernels: hi32 - lo32 on the screening box b, and its TH in `th`.  The decision is d < -th (miss) or d > th (hit);
// anything else (NaN included) is left to Aabb::hit in f64.
// hi = r_min(r_min(fx, fy), r_min(fz, tmaxf)) and m = r_max(|lo|, |hi|), written out: the compiler re-quiets the
// loop-invariant tmaxf with a v_max_f32 x, x at every step (instruction selection works block by block and
// cannot see that it is a number), and one VALU instruction in the walk loop is about 1.5 % of the frame
CR_D float screen_box_d(const float* b, Pair<float> fox, Pair<float> foy, Pair<float> foz, Pair<float> fix, Pair<float> fiy, Pair<float> fiz,
                        float tminf, float tmaxf, float th0, float& th) {
    // t = fma(bf, if, -p) with p = fl(of if), the same product as screen_q: loop-invariant, so the compiler hoists it and
    // each axis is one v_pk_fma_f32 (the bound above is derived for this form; -ffp-contract=off does not bind the screen)
    const Pair<float> tx = __builtin_elementwise_fma(Pair<float>{b[0], b[1]}, fix, -(fox * fix));
    const Pair<float> ty = __builtin_elementwise_fma(Pair<float>{b[2], b[3]}, fiy, -(foy * fiy));
    const Pair<float> tz = __builtin_elementwise_fma(Pair<float>{b[4], b[5]}, fiz, -(foz * fiz));
    const float nx = r_min(tx.x, tx.y), ny = r_min(ty.x, ty.y), nz = r_min(tz.x, tz.y);
    const float fx = r_max(tx.x, tx.y), fy = r_max(ty.x, ty.y), fz = r_max(tz.x, tz.y);
    const float lo = r_max(r_max(nx, ny), r_max(nz, tminf));
    float hi, m;
    asm("v_min_f32_e32 %0, %2, %3\n\tv_min3_f32 %0, %4, %5, %0\n\tv_max_f32_e64 %1, |%6|, |%0|"
        : "=&v"(hi), "=v"(m) : "v"(fz), "v"(tmaxf), "v"(fx), "v"(fy), "v"(lo));
    th = __builtin_fmaf(0x1.0p-20f, m, th0);
    return hi - lo;
}
// f32 kernels (EXACT): Aabb::hit's `max <= min -> miss` on the record, with the same operations as box_miss_fast (min(h, tmax)
// <= lo there is h <= lo || tmax <= lo)
CR_D bool screen_box_miss_exact(const float* b, Pair<float> fox, Pair<float> foy, Pair<float> foz, Pair<float> fix, Pair<float> fiy,
                                Pair<float> fiz, float tminf, float tmaxf) {
    const Pair<float> tx = (Pair<float>{b[0], b[1]} - fox) * fix;
    const Pair<float> ty = (Pair<float>{b[2], b[3]} - foy) * fiy;
    const Pair<float> tz = (Pair<float>{b[4], b[5]} - foz) * fiz;
    const float nx = r_min(tx.x, tx.y), ny = r_min(ty.x, ty.y), nz = r_min(tz.x, tz.y);
    const float fx = r_max(tx.x, tx.y), fy = r_max(ty.x, ty.y), fz = r_max(tz.x, tz.y);
    const float lo = r_max(r_max(nx, ny), r_max(nz, tminf));
    float hi;
    asm("v_min_f32_e32 %0, %1, %2\n\tv_min3_f32 %0, %3, %4, %0" : "=&v"(hi) : "v"(fz), "v"(tmaxf), "v"(fx), "v"(fy));
    return hi <= lo;
}

// Where Sphere::hit's shared reciprocal lives (sphere_quot): 0 -- nowhere, the kernel divides; 1 -- WalkState::rda, made once per
// segment in walk_begin<true>; 2 -- made in walk_round at the head of each leaf phase, live inside the primitive loop only.
// Decided kernel by kernel from the compiler's allocation (scripts/kernel_resources.py; the table is in DESIGN.md section 3.10):
// no kernel may gain a spill.  The f64 render kernels that walk on screening records with the tree in LDS or its top there take
// form 1 -- the headline's, the 1M-sphere frame's, their region, batch and listed twins.  Of the other f64 render kernels, those
// with the whole tree in global memory or its top in LDS without the screen gain an SGPR spill under some sum order or camera and
// the keyed ones (ANIM) with relaxed sums 6-12 spilled VGPRs; the guide-layer kernels (aov_kernel.hpp: one segment per sample,
// nothing to share) would spill too: those divide, as do the f32 kernels and the cross-check pipelines.
// -DCR_QUOT_FORM=0|1|2 builds one form into the same kernels (profiles/experiments/shared_reciprocal_ab.txt).
template <typename real, int RES, bool ANIM, bool SCREEN> constexpr int quot_form() {
    constexpr bool fits = std::is_same<real, double>::value && !ANIM && SCREEN && RES != RES_GLOBAL;
#ifdef CR_QUOT_FORM
    return fits ? CR_QUOT_FORM : 0;
#else
    return fits ? 1 : 0;
#endif
}

// -DCR_SPHERE_LOOP=0, -DCR_SHADE_DD=0: the A/B switches of the spheres-only primitive loop (walk_round) and of shade's reuse of
// WalkState::dd in the render kernels (profiles/experiments/segment_setup_ab.txt)
#ifndef CR_SPHERE_LOOP
#define CR_SPHERE_LOOP 1
#endif
#ifndef CR_SHADE_DD
#define CR_SHADE_DD 1
#endif
// The A/B switches of the work around the box step (profiles/experiments/round_overhead_ab.txt), both in
// the kernels of walk_offset() -- the headline's counted and quiet kernel:
// -DCR_WALK_OFFSET=0: the position across rounds is WalkState's index, not WalkOffset's LDS address.
// -DCR_WALK_PRIO=0:   no s_setprio around the rounds loop (1: the walking wave at priority 1, a shading wave at 0).
#ifndef CR_WALK_OFFSET
#define CR_WALK_OFFSET 1
#endif
#ifndef CR_WALK_PRIO
#define CR_WALK_PRIO 1
#endif
// Which kernels begin a segment with walk_begin_screened and walk with LAZY_INV: decided like quot_form(), from the compiler's
// allocation and the A/B (DESIGN.md section 3.11 has the table) -- the static f64 render kernels that walk on screening records
// of an unordered tree.  The keyed and batch kernels (ANIM, CAMK) would gain SGPR spills, the ordered-tree kernels measured
// 0.8 % slower with it; they, the guide-layer kernels, the cross-check pipelines and every f32 kernel keep walk_begin.
// -DCR_LAZY_INV=0 builds the kernels without it.
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK, bool SCREEN> constexpr bool lazy_inv() {
#if defined(CR_LAZY_INV) && CR_LAZY_INV == 0
    return false;
#else
    return std::is_same<real, double>::value && SCREEN && !ANIM && !ORD && !CAMK;
#endif
}
// Which kernels test a scene of spheres alone in a loop of its own (walk_round's SPHERE_LOOP): by the same rule
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK, bool SCREEN> constexpr bool sphere_loop() {
    return CR_SPHERE_LOOP && std::is_same<real, double>::value && SCREEN && RES == RES_LDS && !ANIM && !ORD && !CAMK;
}

// The headline's kernels: the ones the switches above apply to
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK, bool RELAX, bool SCREEN> constexpr bool walk_offset() {
    return lazy_inv<real, RES, ANIM, ORD, CAMK, SCREEN>() && RES == RES_LDS && RELAX;
}

// 1 / direction as walk_begin divides it, for Aabb::hit's f64 form where a LAZY_INV walk runs it
// (the direction passes through an empty asm: the divisions are loop-invariant and free of side effects, and the optimiser
// hoisted them out of the band branch and the rounds loop to where walk_begin had them, once per outer iteration)
template <typename real> CR_D V3<real> inv_of(V3<real> rd) {
    asm volatile("" : "+v"(rd.x), "+v"(rd.y), "+v"(rd.z));
    return mk<real>(real(1) / rd.x, real(1) / rd.y, real(1) / rd.z);
}

// SHARE: the caller began the walk with walk_begin<quot_form() == 1>; the guide-layer kernels and the cross-check pipelines do not.
// LAZY_INV (f64 SCREEN kernels): the caller began it with walk_begin_screened; 1 / direction is divided where f64 needs it.
// SPHERE_LOOP (sphere_loop()'s kernels): the leaf phase tests a scene of spheres alone in a loop of its own.
// CN, CP: the node and primitive counters' types -- NoCount in the kernels that keep no work counters (pathtrace_kernel_quiet).
template <typename real, int RES, bool ANIM, bool ORD = false, bool SCREEN = false, bool SHARE = false, bool LAZY_INV = false, bool SPHERE_LOOP = false,
          typename CN = unsigned long long, typename CP = uint32_t, typename WS = WalkState<real>>
CR_D void walk_round(const KernelArgs<real>& A, const Entry<real>* lds_entries, const Prim<real>* prims, V3<real> ro, V3<real> rd, real rtime,
                     WS& w, bool walking, uint32_t budget, CN& c_node, CP& c_prim, Diag* dg = nullptr,
                     const void* lds_screen = nullptr) {
    constexpr bool COUNT = !std::is_same<CN, NoCount>::value;
    // WS = WalkOffset: the position is the LDS address w.off (obase: the first record's, oend: walk finished)
    constexpr bool OFFS = std::is_same<WS, WalkOffset>::value;
    static_assert(!OFFS || (LAZY_INV && RES == RES_LDS && !ORD), "WalkOffset is the state of walk_offset()'s kernels");
    uint32_t obase = 0u, oend = 0u;
    if constexpr (OFFS) { obase = screen_lds_base<RES>(lds_screen); oend = obase + ((uint32_t)A.n_entries << 5); }
    // f64: decisions on the f32 copy where f32 can decide; f32 (EXACT below): the record IS the wrapper's box, in the link layout of ScreenEntry
    constexpr bool EXACT = std::is_same<real, float>::value;
    static_assert(!(SCREEN && EXACT && ORD), "the f32 kernels use ScreenEntry records for unordered trees only");
    static_assert(!LAZY_INV || (SCREEN && !EXACT), "LAZY_INV is a form of the f64 SCREEN kernels");
    const real tmin = real(0.001);
    const int32_t n_entries = A.n_entries;
    // SCREEN kernels keep only screening records in LDS: the rare f64 record is read from global memory
    constexpr int RES64 = SCREEN ? RES_GLOBAL : RES;
    const int32_t lds_n64 = SCREEN ? 0 : A.lds_entries;
    int32_t leaf = w.pending;
    if (walking && leaf < 0) {
        CR_DIAG_HIT(dg, DG_ROUND_WAVE, DG_ROUND_LANE);
        // SCREEN kernels: steps the f32 loop could not take -- one, for a lane it left at a box too close to call, or all of
        // them for a ray outside its range -- are made below with Aabb::hit's own compare/select form on the f64 records
        uint32_t exact_steps = 0u;
        if constexpr (!LAZY_INV) exact_steps = w.exact_box ? 0xffffffffu : 0u;
        if constexpr (SCREEN) {
            const float ofx = (float)ro.x, ofy = (float)ro.y, ofz = (float)ro.z;
            float ifx, ify, ifz;
            if constexpr (LAZY_INV) { ifx = w.invf.x; ify = w.invf.y; ifz = w.invf.z; }
            else { ifx = (float)w.inv.x; ify = (float)w.inv.y; ifz = (float)w.inv.z; }
            float mo, pmax, pmin;
            if constexpr (LAZY_INV) pmax = r_max(r_max(__builtin_fabsf(ifx), __builtin_fabsf(ify)), __builtin_fabsf(ifz));   // (classified at the segment's start)
            else screen_extents(ofx, ofy, ofz, ifx, ify, ifz, mo, pmax, pmin);
            // (an f32 kernel's test on the record is Aabb::hit itself for every ray with finite 1/direction: no range to respect)
            bool screened;
            if constexpr (LAZY_INV) screened = !w.unscreened;   // walk_begin_screened decided, once per segment
            else if constexpr (EXACT) screened = !w.exact_box;
            else screened = screen_in_range(w.exact_box, mo, pmax, pmin);
            if (!screened) exact_steps = 0xffffffffu;
            else {
                const float qx = screen_q(ofx, ifx), qy = screen_q(ofy, ify), qz = screen_q(ofz, ifz);
                const Pair<float> fox = {ofx, ofx}, foy = {ofy, ofy}, foz = {ofz, ofz};
                const Pair<float> fix = {ifx, ifx}, fiy = {ify, ify}, fiz = {ifz, ifz};
                const float tminf = 0.001f;
                float tmaxf = (float)w.best_t;   // tmax cannot change inside the loop
                const float th0 = screen_th0(qx, qy, qz, pmax);
                asm volatile("" : "+v"(tmaxf));   // keep it in a register: the allocator would re-convert tmax at every step
                uint32_t nodes = 0;
                // Aabb::hit of the wrapper at index `idx` decided on its screening box `b`: true = miss
                auto box_miss = [&](const float* b, int32_t idx) -> bool {
                    if constexpr (EXACT) {
                        const bool miss = screen_box_miss_exact(b, fox, foy, foz, fix, fiy, fiz, tminf, tmaxf);
                        nodes++;
                        CR_DIAG_HIT(dg, DG_BOX_WAVE, DG_BOX_LANE);
                        return miss;
                    }
                    float th;
                    float d = screen_box_d(b, fox, foy, foz, fix, fiy, fiz, tminf, tmaxf, th0, th);
                    nodes++;
                    CR_DIAG_HIT(dg, DG_BOX_WAVE, DG_BOX_LANE);
                    // too close to call in f32: Aabb::hit in f64 on the f64 box.  (The wave tests "any lane?" with a scalar branch and
                    // the rare lane overwrites d, so that the common path carries no mask bookkeeping for the merge.)
                    const bool band = !(__builtin_fabsf(d) > th);
                    if (__builtin_expect(__ballot(band) != 0ull, 0)) {
                        if (band) {
                            CR_DIAG_HIT(dg, DG_BAND_WAVE, DG_BAND_LANE);
                            const Entry<real> e = ORD ? fetch_entry_ordered<real, RES64>(lds_entries, A.entries, lds_n64, idx, w.oct)
                                                      : fetch_entry<real, RES64>(lds_entries, A.entries, lds_n64, idx);
                            if constexpr (LAZY_INV) d = box_hit(e.b, ro, inv_of(rd), tmin, w.best_t) ? 1.0f : -1.0f;
                            else d = box_hit(e.b, ro, w.inv, tmin, w.best_t) ? 1.0f : -1.0f;
                        }
                    }
                    return d < 0.0f;
                };
                // `it` is the same in every lane still in the loop (a scalar register)
                if constexpr (ORD) {
                    // near child first: the same loop on ScreenEntryO records -- the skip link is the octant's, the hit link the left
                    // child's plus one record when the ray points down the split axis
                    const uint32_t base = screen_lds_base<RES>(lds_screen);
                    const uint32_t end = base + ((uint32_t)n_entries << 6);
                    const uint32_t oct = (uint32_t)w.oct, octoff = 32u + (oct << 2);
                    uint32_t off = base + ((uint32_t)w.idx << 6), after_leaf = 0;
                    if (off < end) {
                        for (uint32_t it = 0;; it++) {
                            const ScreenStepO se = fetch_screen_ordered<RES>((const ScreenEntryO*)lds_screen, (const ScreenEntryO*)A.screen, (uint32_t)A.lds_entries << 6, off, octoff);
                            const bool miss = box_miss(se.b, (int32_t)((off - base) >> 6));
                            after_leaf = se.skip;
                            off = miss ? se.skip : se.hit + (__builtin_amdgcn_ubfe(oct, se.axis, 1u) << 6);
                            uint32_t limit = (it + 1 == budget) ? 0u : end;   // (as below)
                            asm("" : "+s"(limit));
                            if (off >= limit) break;
                        }
                        if (off & kScreenLeaf) { leaf = (int32_t)(off & ~kScreenLeaf); off = after_leaf; }
                        w.idx = (int32_t)((off - base) >> 6);
                    }
                } else {
                    // the lane's position as a byte offset into the record array (ScreenEntry): a lane leaves the loop at the
                    // end of the array or with a leaf in hand, and one compare sees both
                    const uint32_t base = screen_lds_base<RES>(lds_screen);
                    const uint32_t end = base + ((uint32_t)n_entries << 5);
                    uint32_t off, after_leaf = 0;
                    if constexpr (OFFS) off = w.off; else off = base + ((uint32_t)w.idx << 5);
                    if (off < end) {
                        for (uint32_t it = 0;; it++) {
                            const ScreenEntry se = fetch_screen<RES>((const ScreenEntry*)lds_screen, (const ScreenEntry*)A.screen, (uint32_t)A.lds_entries << 5, off);
                            const bool miss = box_miss(se.b, (int32_t)((off - base) >> 5));
                            after_leaf = se.skip;
                            off = miss ? se.skip : se.hit;
                            // the round's last step ends it for every lane: a scalar select of the limit (hidden from the optimiser,
                            // which would turn it back into a second exit mask)
                            // (!COUNT: without the per-lane node count beside it the step count would become a per-lane
                            // countdown, one vector instruction more than the scalar add it replaces: it is pinned to its register)
                            if constexpr (!COUNT) asm volatile("" : "+s"(it));
                            uint32_t limit = (it + 1 == budget) ? 0u : end;
                            asm("" : "+s"(limit));
                            if (off >= limit) break;
                        }
                        if (off & kScreenLeaf) { leaf = (int32_t)(off & ~kScreenLeaf); off = after_leaf; }
                        if constexpr (OFFS) w.off = off; else w.idx = (int32_t)((off - base) >> 5);
                    }
                }
                c_node += nodes;
            }
        } else if (!w.exact_box) {
            const Pair<real> ox = {ro.x, ro.x}, oy = {ro.y, ro.y}, oz = {ro.z, ro.z};
            const Pair<real> ix = {w.inv.x, w.inv.x}, iy = {w.inv.y, w.inv.y}, iz = {w.inv.z, w.inv.z};
            // `it` is the same in every lane still in the loop (a scalar register); tmax cannot change inside it
            const real tmax = w.best_t;
            uint32_t nodes = 0;
            for (uint32_t it = 0; w.idx < n_entries; it++) {
                const Entry<real> e = ORD ? fetch_entry_ordered<real, RES64>(lds_entries, A.entries, lds_n64, w.idx, w.oct)
                                          : fetch_entry<real, RES64>(lds_entries, A.entries, lds_n64, w.idx);
                nodes++;
                CR_DIAG_HIT(dg, DG_BOX_WAVE, DG_BOX_LANE);
                const bool miss = box_miss_fast(e.b, ox, oy, oz, ix, iy, iz, tmin, tmax);
                const bool inner = e.leaf < 0;
                w.idx = (inner && !miss) ? (ORD ? ordered_near(e.leaf, w.oct) : -e.leaf) : e.skip;
                if (!(miss || inner)) { leaf = e.leaf; break; }
                if (it + 1 == budget) break;
            }
            c_node += nodes;
        }
        V3<real> inv_lazy = mk<real>(0, 0, 0);   // LAZY_INV: the divisions only where the loop runs
        if constexpr (OFFS) {
            // The same loop for a position kept as an address: the index is made where the loop runs, and turned back behind it.
            // A copy, not the loop below on a reference to either index: that form changed the code of the kernels that keep
            // WalkState (the counted headline kernel with both switches off no longer compiled to the parent's assembly) and
            // moved the headline kernels' own allocation.
            if (exact_steps != 0u && w.off < oend) {
                inv_lazy = inv_of(rd);
                int32_t idx = (int32_t)((w.off - obase) >> 5);
                for (; exact_steps != 0u && idx < n_entries; exact_steps--) {
                    const Entry<real> e = fetch_entry<real, RES64>(lds_entries, A.entries, lds_n64, idx);
                    c_node++;
                    const bool hit = box_hit(e.b, ro, inv_lazy, tmin, w.best_t);
                    idx = (hit && e.leaf < 0) ? -e.leaf : e.skip;
                    if (hit && e.leaf >= 0) { leaf = e.leaf; break; }
                }
                w.off = obase + ((uint32_t)idx << 5);
            }
        } else {
        if constexpr (LAZY_INV) { if (exact_steps != 0u && w.idx < n_entries) inv_lazy = inv_of(rd); }
        for (; exact_steps != 0u && w.idx < n_entries; exact_steps--) {
            const Entry<real> e = ORD ? fetch_entry_ordered<real, RES64>(lds_entries, A.entries, lds_n64, w.idx, w.oct)
                                      : fetch_entry<real, RES64>(lds_entries, A.entries, lds_n64, w.idx);
            c_node++;
            bool hit;
            if constexpr (LAZY_INV) hit = box_hit(e.b, ro, inv_lazy, tmin, w.best_t);
            else hit = box_hit(e.b, ro, w.inv, tmin, w.best_t);
            w.idx = (hit && e.leaf < 0) ? (ORD ? ordered_near(e.leaf, w.oct) : -e.leaf) : e.skip;
            if (hit && e.leaf >= 0) { leaf = e.leaf; break; }
        }
        }
    }
    // The parked lanes intersect their leaves together; with walk_leaf_min set, a thin group waits (parked) while other lanes
    // of the wave can still step, so that the expensive primitive test runs with more lanes.  Per lane the sequence of
    // operations is unchanged: a parked lane does nothing until its leaf is tested.
    w.pending = leaf;
    if (A.walk_leaf_min > 0u) {
        const uint32_t parked = (uint32_t)__popcll(__ballot(leaf >= 0));
        bool stepping;
        if constexpr (OFFS) stepping = walking && leaf < 0 && w.off < oend;
        else stepping = walking && leaf < 0 && w.idx < n_entries;
        const bool can_step = __ballot(stepping) != 0ull;
        if (parked < A.walk_leaf_min && can_step) return;
    }
    w.pending = -1;
    if (leaf >= 0) {
        CR_DIAG_HIT(dg, DG_LEAFPH_WAVE, DG_LEAFPH_LANE);
        constexpr int QF = SHARE ? quot_form<real, RES, ANIM, SCREEN>() : 0;
        const real ra = QF == 1 ? w.rda : (QF == 2 ? shared_rcp(w.dd) : quot_divide<real>());
        auto test = [&](int32_t pi) {
            const Prim<real>& p = prims[pi];
            c_prim++;
            CR_DIAG_HIT(dg, DG_PRIM_WAVE, DG_PRIM_LANE);
            real t;
            bool h;
            real g0 = p.g[0], g1 = p.g[1], g2 = p.g[2], g3 = p.g[3];
            const int32_t kind = A.uniform_kind >= 0 ? A.uniform_kind : p.kind();   // a scalar test; one load fewer per primitive when it holds
            if (kind == 0) {
                if (ANIM && p.key_count) timeline_eval(A.keys + p.key_first, p.key_count, rtime, g0, g1, g2, g3);
                h = sphere_t<RES == RES_LDS || (std::is_same<real, double>::value && !ANIM), QF != 0>(g0, g1, g2, g3, ro, rd, w.dd, tmin, w.best_t, t, dg, ra);
            } else {
                V3<real> a = mk<real>(g0, g1, g2), b = mk<real>(g3, p.g[4], p.g[5]), c = mk<real>(p.g[6], p.g[7], p.g[8]);
                if (ANIM && p.key_count) {
                    a = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, a);
                    b = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, b);
                    c = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, c);
                }
                h = triangle_t(a, b, c, ro, rd, tmin, w.best_t, t);
            }
            if (h) { w.best_t = t; w.best = pi; }
        };
        // Scenes with a HitList element run the ANIM kernels (render.hip), so the static kernels -- the headline's -- keep
        // the one-or-two-record loop alone; A.leaf_runs is null unless such an element exists (a scalar test)
        if (!ANIM || A.leaf_runs == nullptr || !(leaf & kLeafRun)) {
            const int32_t first = leaf >> 1, count = (leaf & 1) + 1;
            if constexpr (RES != RES_LDS && !ANIM) {
                // primitives in global memory: touch the second record's lines while the first is being tested, so that its own
                // loads hit L1 instead of waiting a second L2 round trip (teapot +1.5 %, 1M spheres +1.4 %)
                // (the second word touched lies inside that record: byte 80 of the 96-byte f64 record, the last word of the
                // 48-byte f32 one -- the record may be the last of an exactly sized array)
                constexpr uint32_t touch = sizeof(Prim<real>) == 96 ? 20u : (uint32_t)(sizeof(Prim<real>) / 4 - 1);
                static_assert((touch + 1) * 4 <= sizeof(Prim<real>), "the touched word must lie inside the record");
                GlobPtr<uint32_t> nx = (GlobPtr<uint32_t>)(const void*)(prims + first + (count - 1));
                const uint32_t t0 = nx[0], t1 = nx[touch];
                test(first);
                asm volatile("" :: "v"(t0), "v"(t1));
                if (count == 2) test(first + 1);
            } else if constexpr (SPHERE_LOOP) {
                // sphere_loop()'s kernels: a scene of spheres alone (book1: A.uniform_kind == 0, a scalar test made once per
                // leaf phase and not in every test) runs a copy of the loop without the triangle test and the divergent region
                // around it; the second record hangs on the leaf code's count bit, not on a second induction variable
                static_assert(RES == RES_LDS && !ANIM, "the one-or-two-record loop on primitives in LDS");
                if (A.uniform_kind == 0) {
                    auto sphere = [&](int32_t pi) {   // `test`, for a record that is known to be a sphere
                        const Prim<real>& p = prims[pi];
                        c_prim++;
                        CR_DIAG_HIT(dg, DG_PRIM_WAVE, DG_PRIM_LANE);
                        real t;
                        if (sphere_t<true, QF != 0>(p.g[0], p.g[1], p.g[2], p.g[3], ro, rd, w.dd, tmin, w.best_t, t, dg, ra)) { w.best_t = t; w.best = pi; }
                    };
                    sphere(first);
                    if (leaf & 1) sphere(first + 1);
                } else {
                    test(first);
                    if (leaf & 1) test(first + 1);
                }
            } else
            for (int32_t k = 0; k < count; k++) test(first + k);
        } else {
            const int32_t first = A.leaf_runs[2 * (leaf & kLeafRunIndex)], count = A.leaf_runs[2 * (leaf & kLeafRunIndex) + 1];
            for (int32_t k = 0; k < count; k++) test(first + k);
        }
    }
}

}   // namespace cr

#endif   // __HIPCC__
