// records.hpp -- the path tracer's bottom layer, shared by host and device: scalar traits and the r_*
// helpers, V3 and the clamped Color operations, the RNG, the record types of a device scene (Entry, EntryO, ScreenEntry,
// ScreenEntryO, Prim, Mat, Tex, ImageRef, Key), CamConst, KernelArgs with the asserts on its layout, the timeline and the camera
// frame, and the launch constants the host asks about (MaxBlock, LatencyBlock).  What the host units, the tree builders and
// the refit read; no kernel code.  Free of the HIP runtime: with hd.hpp, fastdiv.hpp and residency.hpp it compiles under a
// plain C++ compiler (tests/test_headers_host.py, tests/quot_range_check.cpp).  The reference citations are pathtrace.hpp's.
// Every expression keeps the reference's operand order; the build uses -ffp-contract=off so no FMA is formed, and IEEE div/sqrt.
#pragma once
#include "hd.hpp"
#include "fastdiv.hpp"
#include "residency.hpp"   // RES_GLOBAL / RES_LDS / RES_TOP, where the scene is read from, and the rule that picks one

#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace cr {

// ------------------------------------------------------------------ scalar traits
template <typename real> struct RealTraits;
template <> struct RealTraits<float> {
    static constexpr float eps = 1.1920928955078125e-07f;   // FLT_EPSILON (f32 twin of f64::EPSILON, triangle.rs:101)
    static constexpr float tiny = 0.0f;                     // 1e-160 rounds to 0 in f32 (utils.rs:131)
    static constexpr float pi = 3.14159265358979323846f;
};
template <> struct RealTraits<double> {
    static constexpr double eps = 2.220446049250313e-16;    // f64::EPSILON
    static constexpr double tiny = 1e-160;
    static constexpr double pi = 3.14159265358979323846;
};

CR_HD float r_sqrt(float x) { return __builtin_sqrtf(x); }
// f64 on the device: the compiler expands a correctly rounded square root into v_rsq_f64 and two Newton steps on
// g ~ sqrt(x), h ~ 1/(2 sqrt(x)), wrapped in a scale-up of inputs below 2^-767, the scale-down of the result and a select for
// 0 and +inf -- eight instructions that do nothing for an ordinary number.  When every active lane of the wave holds one (one
// scalar branch), the same ten-instruction core runs without them and returns the same bits (tests/test_gpu_sqrt.py compares
// the two on the device); any other wave takes the compiler's sequence.  The sphere test runs ~8 times per path segment.
CR_HD double r_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t hi = (uint32_t)((unsigned long long)__builtin_bit_cast(long long, x) >> 32);
    const bool ordinary = (hi - 0x10000000u) < (0x7ff00000u - 0x10000000u);   // 2^-767 <= x < +inf
    if (__builtin_amdgcn_ballot_w64(!ordinary) == 0ull) {
        const double y = __builtin_amdgcn_rsq(x);
        double g = x * y, h = y * 0.5;
        const double r = __builtin_fma(-h, g, 0.5);
        g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
        double d = __builtin_fma(-g, g, x);
        g = __builtin_fma(d, h, g);
        d = __builtin_fma(-g, g, x);
        return __builtin_fma(d, h, g);
    }
#endif
    return __builtin_sqrt(x);
}
// The operand range of Sphere::hit's short quotient (sphere_quot in intersect.hpp, where the argument stands): 2^-400 <= |x| < 2^400, read
// from the word that holds sign and exponent.  kQuotLo: that word for 2^-400; kQuotSpan: 800 binades of exponent field.
// tests/quot_range_check.cpp holds quot_in_range to frexp on the host.
constexpr uint32_t kQuotLo = 0x26f00000u, kQuotSpan = 800u << 20;
CR_HD bool quot_in_range(double x) {
    const uint32_t hi = (uint32_t)((unsigned long long)__builtin_bit_cast(long long, x) >> 32);
    return ((hi << 1) - (kQuotLo << 1)) < (kQuotSpan << 1);
}
// the reciprocal that means "divide": every quotient by it takes `/` (a NaN; the f32 kernels keep `/` and never read theirs)
template <typename real> CR_HD real quot_divide() { return real(0); }
template <> CR_HD double quot_divide<double>() { return __builtin_bit_cast(double, 0x7ff8000000000000ll); }
CR_HD float r_abs(float x) { return __builtin_fabsf(x); }
CR_HD double r_abs(double x) { return __builtin_fabs(x); }
CR_HD float r_floor(float x) { return __builtin_floorf(x); }
CR_HD double r_floor(double x) { return __builtin_floor(x); }
CR_HD float r_inf(float) { return __builtin_huge_valf(); }
CR_HD double r_inf(double) { return __builtin_huge_val(); }
// f64::min: the non-NaN operand when one is NaN (== fmin)
CR_HD float r_fmin(float a, float b) { return __builtin_fminf(a, b); }
CR_HD double r_fmin(double a, double b) { return __builtin_fmin(a, b); }
CR_HD float r_fmax(float a, float b) { return __builtin_fmaxf(a, b); }
CR_HD double r_fmax(double a, double b) { return __builtin_fmax(a, b); }

// ------------------------------------------------------------------ Vec3 (utils.rs:72-340)
template <typename real> struct V3 { real x, y, z; };

template <typename real> CR_HD V3<real> mk(real x, real y, real z) { return V3<real>{x, y, z}; }
template <typename real> CR_HD V3<real> neg(V3<real> a) { return mk<real>(-a.x, -a.y, -a.z); }
template <typename real> CR_HD V3<real> add(V3<real> a, V3<real> b) { return mk<real>(a.x + b.x, a.y + b.y, a.z + b.z); }
template <typename real> CR_HD V3<real> sub(V3<real> a, V3<real> b) { return add(a, neg(b)); }   // self + (-rhs), utils.rs:293-298
template <typename real> CR_HD V3<real> scale(real s, V3<real> a) { return mk<real>(s * a.x, s * a.y, s * a.z); }
template <typename real> CR_HD V3<real> divs(V3<real> a, real s) { return scale(real(1) / s, a); }   // (1.0/rhs)*self, utils.rs:335-340
template <typename real> CR_HD real len2(V3<real> a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
template <typename real> CR_HD real dot(V3<real> a, V3<real> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <typename real> CR_HD V3<real> cross(V3<real> a, V3<real> b) {
    return mk<real>(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
template <typename real> CR_HD V3<real> unit(V3<real> a) { return divs(a, r_sqrt(len2(a))); }
template <typename real> CR_HD V3<real> reflect(V3<real> v, V3<real> n) { return sub(v, scale(real(2) * dot(v, n), n)); }   // utils.rs:149-151
template <typename real> CR_HD V3<real> refract(V3<real> v, V3<real> n, real eta) {   // utils.rs:157-163
    real cos_theta = r_fmin(dot(neg(v), n), real(1));
    V3<real> perp = scale(eta, add(v, scale(cos_theta, n)));
    V3<real> par = scale(-(r_sqrt(r_abs(real(1) - len2(perp)))), n);
    return add(perp, par);
}

template <typename real> CR_HD real clamp01(real x) { return x < real(0) ? real(0) : (x > real(1) ? real(1) : x); }   // f64::clamp

// clamped Color ops (utils.rs:445-607); a Color is a V3 with r,g,b in x,y,z
template <typename real> CR_HD V3<real> c_neg(V3<real> c) {
    real lo = c.x < c.y ? c.x : c.y; lo = lo < c.z ? lo : c.z;
    real hi = c.x > c.y ? c.x : c.y; hi = hi > c.z ? hi : c.z;
    real k = lo + hi;
    return mk<real>(r_abs(k - c.x), r_abs(k - c.y), r_abs(k - c.z));
}
template <typename real> CR_HD V3<real> c_add(V3<real> a, V3<real> b) { return mk<real>(clamp01(a.x + b.x), clamp01(a.y + b.y), clamp01(a.z + b.z)); }
template <typename real> CR_HD V3<real> c_scale(real s, V3<real> c) {   // impl Mul<Color> for f64
    V3<real> m = (s < real(0)) ? c_neg(c) : c;
    real p = r_abs(s);
    return mk<real>(clamp01(p * m.x), clamp01(p * m.y), clamp01(p * m.z));
}
template <typename real> CR_HD V3<real> c_mul(V3<real> a, V3<real> b) { return mk<real>(clamp01(a.x * b.x), clamp01(a.y * b.y), clamp01(a.z * b.z)); }
template <typename real> CR_HD V3<real> c_div(V3<real> c, real s) {
    V3<real> m = (s < real(0)) ? c_neg(c) : c;
    return c_scale(real(1) / r_abs(s), m);
}

// ------------------------------------------------------------------ RNG (DESIGN.md "RNG")
// One stream per (seed, pixel, sample): the key is SplitMix64's finaliser of those three (mix64), the draws are
// xorshift64* (Marsaglia's 12/25/27 xorshift scrambled by one multiply; Vigna, "An experimental exploration of
// Marsaglia's xorshift generators, scrambled", 2016) started from that key.  One 64-bit multiply per draw instead
// of SplitMix64's two -- 64-bit multiplies are quarter-rate here and the draws were ~10 % of the kernel.  Only the
// top 24 (f32) / 53 (f64) bits of an output are used, so f32 uniforms are truncations of the f64 ones.
constexpr uint64_t RNG_GAMMA = 0x9E3779B97F4A7C15ULL;
CR_HD uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
CR_HD uint64_t rng_key(uint64_t seed_mixed, uint32_t pixel, uint32_t sample) {
    const uint64_t k = mix64(seed_mixed ^ (((uint64_t)pixel << 32) | (uint64_t)sample));
    return k ? k : RNG_GAMMA;   // xorshift state must not be zero
}
CR_HD void rng_step(uint64_t& s) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; }   // the state alone: a draw whose value nobody reads
CR_HD uint64_t rng_next(uint64_t& s) {
    rng_step(s);
    return s * 0x2545F4914F6CDD1DULL;
}
// The conversions go through 32-bit words (exact: 24 resp. 21+32 significant bits), which is much
// cheaper on the GPU than the generic u64 -> float sequence and yields the same value.
CR_HD float u01(uint64_t u, float) { return (float)(uint32_t)(u >> 40) * 0x1.0p-24f; }
CR_HD double u01(uint64_t u, double) {
    const uint64_t v = u >> 11;
    return ((double)(uint32_t)(v >> 32) * 4294967296.0 + (double)(uint32_t)v) * 0x1.0p-53;
}
template <typename real> CR_HD real rng_uniform(uint64_t& s) { return u01(rng_next(s), real(0)); }
template <typename real> CR_HD real rng_range(uint64_t& s, real lo, real hi) { return lo + (hi - lo) * rng_uniform<real>(s); }

template <typename real> CR_HD V3<real> random_unit_vector(uint64_t& s) {   // utils.rs:127-136
    for (;;) {
        real x = rng_range<real>(s, real(-1), real(1));
        real y = rng_range<real>(s, real(-1), real(1));
        real z = rng_range<real>(s, real(-1), real(1));
        V3<real> p = mk<real>(x, y, z);
        real lensq = len2(p);
        if (RealTraits<real>::tiny < lensq && lensq <= real(1)) return divs(p, r_sqrt(lensq));
    }
}

// ------------------------------------------------------------------ device scene layout
// Threaded BVH: the reference's wrapper tree (bvhwrapper.rs:46-78) with explicit links.
// A walk that goes to the left child on a box hit and to `skip` (the next wrapper in DFS
// pre-order after this subtree; n_entries = none) on a miss or after a leaf visits exactly the
// wrappers BVHWrapper::hit visits, in the same order (left subtree, then right).
// leaf < 0: inner wrapper, left child = -leaf.  leaf >= 0: span-1 or span-2 wrapper whose
// children are primitives: first = leaf >> 1, count = (leaf & 1) + 1, in leaf order.
// leaf >= 0 with kLeafRun set: a leaf that holds a HitList element; its primitives are the run
// (first, count) = leaf_runs[2 * (leaf & kLeafRunIndex)], [.. + 1] -- the list's visible objects and the wrapper's other
// child in the order BVHWrapper::hit and HitList::hit visit them (bvhwrapper.rs:108-120, hitlist.rs:55-61).
// Entries are stored level by level (BFS), so the first K entries are the top of the tree:
// scenes too large for LDS keep those K in LDS and read the rest through L2.
template <typename real> struct alignas(16) Entry {
    real b[6];      // xmin, xmax, ymin, ymax, zmin, zmax
    int32_t skip;
    int32_t leaf;
};
// CR_BVH_SAH_ORDERED: the same wrapper with one skip link per ray-direction octant, so the walk can take the
// child on the ray's side of the split first and still be stackless.  Siblings are adjacent in the level-order
// array, hence an inner wrapper stores only its left child and the split axis: leaf = -(left * 4 + axis), and the
// near child of a ray with octant bits oct (bit a set: direction[a] < 0) is left + ((oct >> axis) & 1).
// skip[oct] = the wrapper to visit after this subtree under that octant's order.  The head (b, leaf) overlays
// Entry's, so a refit or an export can read either.
template <typename real> struct alignas(16) EntryO {
    real b[6];
    int32_t unused;
    int32_t leaf;
    int32_t skip[8];
};
template <typename real, bool ORD> struct EntryOf { using type = Entry<real>; };
template <typename real> struct EntryOf<real, true> { using type = EntryO<real>; };
// f64 kernels: the f32 SCREENING copy of a wrapper -- the box rounded to f32, the same links.  The walk decides most box
// tests on this 32-byte record (half the bytes of Entry<double>) and reads the f64 box only when the f32 result is too
// close to call (screen_step below; DESIGN.md section 3.4 has the error bound).
// The links are stored the way the walk's inner loop consumes them: `skip` = BYTE offset of the wrapper to visit after a
// miss (index * 32; n_entries * 32 ends the walk) and `hit` = what a box hit leads to -- the byte offset of the left child, or
// kScreenLeaf | leaf code for a leaf wrapper.  One select picks the next offset and ONE unsigned compare (next >= n_entries * 32)
// sees both ways out of the loop; the offset is the LDS address / the 32-bit offset of a global load as it stands.
struct alignas(16) ScreenEntry {
    float b[6];
    uint32_t skip;
    uint32_t hit;
};
constexpr uint32_t kScreenLeaf = 0x80000000u;
constexpr int32_t kScreenMaxEntries = 1 << 26;   // offsets stay below bit 31
// ... and of an EntryO (CR_BVH_SAH_ORDERED): 64 bytes instead of 96.
// Links as in ScreenEntry (byte offsets into this array, index * 64): `hit` = the LEFT child's offset or kScreenLeaf | leaf
// code, `axis` = the split axis (3 for a leaf), `skip[o]` = the wrapper after a miss for a ray of direction octant o.  The
// near child is one bit-field extract and one shift-add away: hit + (((octant >> axis) & 1) << 6) -- and a leaf's axis 3 selects
// a bit no octant has, so the same two instructions leave its code alone.
struct alignas(16) ScreenEntryO {
    float b[6];
    uint32_t axis;
    uint32_t hit;
    uint32_t skip[8];
};
constexpr int32_t kScreenMaxEntriesO = 1 << 25;   // offsets stay below bit 31
template <bool ORD> struct ScreenOf { using type = ScreenEntry; };
template <> struct ScreenOf<true> { using type = ScreenEntryO; };
constexpr int32_t kLeafRun = 0x40000000;
constexpr int32_t kLeafPseudo = 0x20000000;   // with kLeafRun: the record stands for a primitive / list that BVHWrapper::hit tests without a box
constexpr int32_t kLeafRunIndex = 0x1fffffff;
CR_HD int32_t ordered_left(int32_t leaf) { return (-leaf) >> 2; }
CR_HD int32_t ordered_near(int32_t leaf, int32_t oct) { const int32_t v = -leaf; return (v >> 2) + ((oct >> (v & 3)) & 1); }

// Primitive record in leaf order.  g[0..3] sphere centre+radius, or g[0..8] a,b,c.
template <typename real> struct alignas(16) Prim {
    real g[9];
    int32_t kind_mat;   // kind in bit 0, material index above it
    int32_t key_first;
    int32_t key_count;
    CR_HD int32_t kind() const { return kind_mat & 1; }
    CR_HD int32_t mat() const { return kind_mat >> 1; }
};
template <typename real> struct alignas(16) Mat {
    real albedo[3];   // metal albedo | lambertian colour when its texture is solid | dielectric: {1/ior, r0(1/ior), r0(ior)}
    real param;       // scatter_prob | fuzz | refraction_index
    int32_t kind;
    int32_t tex;      // lambertian: texture index, or -1 when albedo[] already holds the solid colour
    real aux;         // lambertian: 1/|scatter_prob|, the factor Color / f64 multiplies by (utils.rs:599-607)
};
// Per-material / per-primitive values the reference recomputes at every hit are computed once at upload with
// the same IEEE operations: 1/radius for static spheres (Prim::g[4]; sphere.rs:97 `/ radius` = (1/radius)*v),
// 1/scatter_prob, 1/ior and Schlick's r0 = ((1-ri)/(1+ri))^2 for both orientations (dielectric.rs:21-38).
template <typename real> struct alignas(16) Tex {
    real color[3];
    real inv_scale;
    int32_t kind, even, odd, image;
};
struct ImageRef { int32_t w, h; uint32_t offset; uint32_t pad; };   // texels: RGBA8 at texels[offset + y*w + x]
template <typename real> struct Key { real t0, t1, a, b; int32_t channel, interp; };

// Camera in `real`.  The four scalars are computed in f64 at set-up as fix_viewport does
// (rendering_compute.rs:5-11,71-73) and rounded once; everything per-sample is `real`.
template <typename real> struct CamConst {
    int32_t W, H;
    real viewport_width, viewport_height, focus_dist, defocus_radius;
    int32_t defocus_on, animated;
    V3<real> from, at, vup;
    int32_t from_key_first, from_key_count, at_key_first, at_key_count;
    // static camera: the per-sample vectors, precomputed with the same expression tree
    V3<real> p00, pdu, pdv, ddu, ddv;
};

template <typename real> struct KernelArgs {
    const Entry<real>* entries;
    const Prim<real>* prims;
    const Mat<real>* mats;
    const Tex<real>* texs;
    const ImageRef* images;
    const uint32_t* texels;
    const Key<real>* keys;
    const Key<real>* cam_keys;   // this launch's camera keyframes (look_from keys, then look_at keys)
    const int32_t* leaf_runs;    // (first, count) pairs for the leaves flagged kLeafRun
    const void* screen;          // f64 SCREEN kernels: one screening record per wrapper (ScreenEntry, or ScreenEntryO for an ordered tree)
    int32_t n_entries, n_prims, n_mats, n_texs;
    int32_t lds_entries;      // entries staged in LDS (all of them, or the top levels of a large tree)
    int32_t lds_side;         // RES_TOP: materials and textures follow the entry window in LDS (they are small even when
                              // the tree is not: the teapot scenes have 2 materials), so shading reads no global tables
    int32_t sky_kind, sky_image;
    CamConst<real> cam;
    int32_t sample_begin, sample_end, samples_total, max_depth;
    uint64_t seed_mixed;      // mix64(seed + GAMMA)
    real current_time, shutter_length;
    int32_t output_sum;
    uint32_t tiles_x, tiles_y;
    uint32_t reg_x0;          // a region's origin in the frame (see n_frames below)
    uint32_t* work_counter;   // zeroed before launch
    // Sample-granular scheduling (megakernel; speed only).  sg_on = 0: a lane owns a pixel and sums its samples
    // in a register.  sg_on = 1: a work item is one (pixel, sample); 64 consecutive items are a tile of
    // 2^sg_lw x 2^sg_lh pixels times 64 >> (sg_lw + sg_lh) consecutive samples, tiles_x/tiles_y count those tiles,
    // sg_groups such groups cover a tile's samples [sample_begin, sample_end), and each finished sample's colour
    // goes to sample_buf[item * 3 .. +2], item = its work-item index: the 64 colours of a group are one contiguous run
    // written by one wave (they merge in that XCD's L2 into whole lines), and sg_finalize_kernel adds them in order.
    uint32_t sg_on, sg_lw, sg_lh, sg_groups;
    uint32_t sg_total;        // work items of the launch (tiles * sg_groups * 64)
    uint32_t sg_chunk;        // work items a wave takes per atomic on the counter (a multiple of 64)
    real* sample_buf;
    uint64_t* counters;       // [0] segments [1] node tests [2] prim tests [3] texel fetches
    real* att_stack;          // max_depth * n_threads records of 3 reals, level-major
    uint32_t n_threads;
    uint32_t reg_y0;
    real* out;
    uint32_t walk_exit_lanes;   // megakernel: leave the walk once this many lanes are done walking (speed only)
    uint32_t walk_round_steps;  // wrappers a lane may step through before the wave intersects the parked leaves (speed only)
    uint32_t walk_leaf_min;     // parked lanes a leaf phase waits for while other lanes can still step (speed only; 0 = every round)
    int32_t uniform_kind;       // 0 / 1: every primitive is a sphere / a triangle (the test need not load the record's kind word); -1: mixed
    uint32_t queue_walk_waves;  // queue_kernel: how many of the workgroup's 16 waves walk (the rest shade)
    uint32_t queue_min_batch, queue_patience;   // queue_kernel: shaders wait for this many hits, at most this many polls
    uint32_t reg_w;             // a region's size
    // CR_SUM_RELAXED (the RELAX kernels): per-pixel fixed-point sums instead of per-sample colours.  A finished sample adds
    // round(colour * fx_scale) to three 64-bit integers of its pixel -- integer adds commute, so the image does not
    // depend on which wave finished which sample when.  Bit 63 of a sum is the NaN flag (a colour that is not a number).
    unsigned long long* fx_acc;   // [H * W * 3], zeroed before the first launch of a render
    double fx_scale;              // 2^S, S = 52 for up to 2047 samples per pixel
    uint32_t fx_lds_off;          // byte offset of the waves' LDS accumulators: 2 slots per wave, each one work tile
                                  // (2^(sg_lw + sg_lh) pixels x 3 channels) of 64-bit words
    // A batch of frames in one launch (cr_render_frames_*: the RELAX kernels with keys, see pathtrace_body).  The tile rows of the n_frames frames
    // follow each other -- frame f owns the tile rows [f * tiles_y, (f + 1) * tiles_y) -- so a work item's pix_j counts
    // the rows of the whole batch (tiles_y << sg_lh per frame, edge padding included) and no tile straddles two frames.
    // Frame f's ray times start at frame_times[f] and its sums sit at fx_acc + f * reg_w * reg_h * 3.  n_frames = 1: a single
    // render, whose times start at current_time (frame_times is not read).
    uint32_t n_frames;
    const real* frame_times;
    // A region of the frame (cr_render_region_*, on the same kernels): the launch's tiles are anchored at pixel (reg_x0, reg_y0)
    // of the frame and cover reg_w x reg_h pixels, so pix_i / pix_j count within the region, fx_acc holds reg_w * reg_h pixels
    // (per frame of a batch) and only camera_ray sees the frame's own pixel (reg_x0 + pix_i, reg_y0 + pix_j): cam.W and cam.H
    // stay the whole frame's (the viewport, the pixel deltas, the RNG's pixel index).  A whole frame is the region
    // (0, 0, cam.W, cam.H), which prepare_args sets for every launch; the kernels without the frame arithmetic read cam.W / cam.H.
    // The four words reg_x0, reg_y0, reg_w, reg_h each sit where the record had four bytes of alignment padding (behind
    // tiles_y, n_threads, queue_patience and fd_tiles_y), so no other argument moved and the kernels that do not read them
    // compile to what they were (the static_asserts below hold the layout).
    // Work items are decoded without a division (fastdiv.hpp): the records of sg_groups, tiles_x and tiles_y, filled
    // wherever those are (set_tiles, set_groups).
    FastDiv fd_groups, fd_tiles_x, fd_tiles_y;
    uint32_t reg_h;
    // The launch's tiles by name (cr_render_adaptive_*, pathtrace_kernel_listed): work item w belongs
    // to tile tile_list[w / (sg_groups * 64)] of the frame instead of tile w / (sg_groups * 64), and sg_total counts the listed
    // tiles only.  Read by pathtrace_kernel_listed alone.  Everything behind the decode sees the frame's own tile number and pixel: the RNG key, the LDS slots, the
    // addresses in fx_acc (a whole frame's).  nullptr, as prepare_args leaves it: every tile of the launch, in order.  The word
    // follows the record's last one, so no other argument moved.
    const int32_t* tile_list;
    // A box of the tree has a plane that is not a number.  Only an f32 tree can (a sphere whose centre AND radius round to
    // infinity: inf - inf; cr_upload_scene and cr_update_primitives take finite f64 values only), and only in its
    // construction-time boxes (a refit unites no sample box that is not a number).  The min/max forms of the box test pass
    // over a NaN where Aabb::hit's comparisons fail on it, so every ray of such a launch walks like a ray with an infinite
    // 1/direction: walk_begin's exact_box.  Read by the f32 kernels alone (tree_walks_exact); the word follows the record's
    // last one, so no other argument moved.
    int32_t exact_boxes;
    // Several cameras in one launch (cr_render_views_*, the VIEWS kernels): view f of the launch -- frame f of
    // the batch's work layout above -- takes its camera from views[f] instead of `cam`, a record packed as `cam` is, whose
    // *_key_first count from the start of cam_keys (the views' keys lie there one view after the other).  `cam` holds view 0's
    // record: every view has its W and H.  Read by the VIEWS kernels alone; the word follows the record's last one, so no
    // other argument moved.
    const CamConst<real>* views;
};
static_assert(sizeof(KernelArgs<float>) == 504 && sizeof(KernelArgs<double>) == 624 && offsetof(KernelArgs<float>, tile_list) == 480 &&
              offsetof(KernelArgs<double>, tile_list) == 600 && offsetof(KernelArgs<float>, exact_boxes) == 488 && offsetof(KernelArgs<double>, exact_boxes) == 608 &&
              offsetof(KernelArgs<float>, views) == 496 && offsetof(KernelArgs<double>, views) == 616,
              "the region's words fill padding, the tile list, exact_boxes and the views' table follow the record");
static_assert(offsetof(KernelArgs<float>, work_counter) == 304 && offsetof(KernelArgs<float>, out) == 368 && offsetof(KernelArgs<float>, fx_acc) == 408 &&
              offsetof(KernelArgs<float>, fd_tiles_y) == 464, "the region's words fill padding: no argument moved");
template <typename real> inline void set_tiles(KernelArgs<real>& a, uint32_t tiles_x, uint32_t tiles_y) {
    a.tiles_x = tiles_x; a.tiles_y = tiles_y;
    a.fd_tiles_x = fastdiv_make(tiles_x); a.fd_tiles_y = fastdiv_make(tiles_y);
}
template <typename real> inline void set_groups(KernelArgs<real>& a, uint32_t groups) {
    a.sg_groups = groups; a.fd_groups = fastdiv_make(groups);
}
// a tile's column and row among the launch's tiles
template <typename real> CR_HD void tile_xy(const KernelArgs<real>& A, uint32_t tile, uint32_t& tx, uint32_t& ty) {
    ty = fastdiv(tile, A.fd_tiles_x);
    tx = tile - ty * A.tiles_x;
}
// the frame of the batch that a batch-wide pixel row belongs to (0 in a single render)
template <typename real> CR_HD uint32_t batch_frame(const KernelArgs<real>& A, uint32_t pix_j) {
    return A.n_frames > 1u ? fastdiv(pix_j >> A.sg_lh, A.fd_tiles_y) : 0u;
}
constexpr unsigned long long kFxNaN = 0x8000000000000000ull;

// ------------------------------------------------------------------ timeline (timeline/mod.rs:233-263)
// combine_and_compute = S * T * (0,0,0,1): T's last column is the initial position plus every active translate
// value, added in list order; S is the LAST active scale transform (:249-255) -- the initial one (sphere:
// diag(1,1,1,r); others: diag(s,s,s,s), s = 1), a ScaleR key (radius), or a ScaleX / ScaleY / ScaleZ key
// (transform_builder.rs:101-346).  x,y,z come back as T's column, w as the scale value, *skind as the channel of
// the scale key that won (-1: the initial scale).
template <typename real> CR_HD void timeline_eval(const Key<real>* keys, int n, real t, real& x, real& y, real& z, real& w, int32_t* skind = nullptr) {
    x = real(0) + x; y = real(0) + y; z = real(0) + z;   // identity * initial translate
    int32_t sk = -1;
    for (int i = 0; i < n; i++) {
        Key<real> k = keys[i];
        bool active = (t > k.t1) || (k.t0 <= t && t <= k.t1);   // is_less(t) || contains(t)
        if (!active) continue;
        real s = clamp01((t - k.t0) / (k.t1 - k.t0));
        if (k.channel <= 2) {
            real val = k.interp ? k.a * s : k.a;
            if (k.channel == 0) x = x + val; else if (k.channel == 1) y = y + val; else z = z + val;
        } else {
            w = k.interp ? k.a + (k.b - k.a) * s : k.a;
            sk = k.channel;
        }
    }
    if (skind) *skind = sk;
}
// S * (x, y, z, 1) for a non-sphere point (a triangle vertex; the 4th component is dropped, triangle.rs:95-97).
// ScaleX is diag(v,1,1,1) and ScaleZ diag(1,1,v,1); ScaleY writes v into row 1, column 0 and leaves the diagonal
// at 1 (transform_builder.rs:228-246), so it shears y by v*x.  Rows of S that hold only a unit diagonal return the
// coordinate unchanged (1*y plus zeros).
template <typename real> CR_HD V3<real> scale_point(int32_t skind, real v, real x, real y, real z) {
    if (skind == 4) return mk<real>(v * x, y, z);
    if (skind == 5) return mk<real>(x, v * x + y, z);
    if (skind == 6) return mk<real>(x, y, v * z);
    return mk<real>(v * x, v * y, v * z);   // build_other_scaler, matrix_builder.rs:63-86
}
// One vertex timeline of a triangle (a_timeline / b_timeline / c_timeline share their keys, scene_animator.rs).
template <typename real> CR_HD V3<real> timeline_vertex(const Key<real>* keys, int n, real t, V3<real> p) {
    real w = real(1);
    int32_t sk;
    timeline_eval(keys, n, t, p.x, p.y, p.z, w, &sk);
    return scale_point(sk, w, p.x, p.y, p.z);
}

// ------------------------------------------------------------------ camera (rendering_compute.rs)
template <typename real> struct CamFrame { V3<real> from, p00, pdu, pdv, ddu, ddv; };

template <typename real> CR_HD CamFrame<real> camera_frame(const CamConst<real>& c, V3<real> from, V3<real> at) {
    CamFrame<real> f;
    f.from = from;
    V3<real> w = unit(sub(from, at));                           // w_basis :91-96
    V3<real> u = unit(cross(c.vup, w));                         // u_basis :81-83
    V3<real> v = cross(w, u);                                   // v_basis :86-88
    V3<real> vu = scale(c.viewport_width, u);                   // viewport_u :18-20
    V3<real> vv = scale(c.viewport_height, neg(v));             // viewport_v :25-28
    f.pdu = divs(vu, (real)c.W);                                // pixel_delta_u :34-36
    f.pdv = divs(vv, (real)c.H);                                // pixel_delta_v :42-44
    V3<real> ul = sub(from, scale(c.focus_dist, w));            // viewport_upperleft :51-56
    ul = sub(ul, divs(vu, real(2)));
    ul = sub(ul, divs(vv, real(2)));
    f.p00 = add(ul, scale(real(0.5), add(f.pdu, f.pdv)));       // pixel_start_location :59-61
    f.ddu = scale(c.defocus_radius, u);                         // defocus_disk_u :99-101
    f.ddv = scale(c.defocus_radius, v);                         // defocus_disk_v :104-106
    return f;
}

// ------------------------------------------------------------------ launch constants
// Largest workgroup the kernels may be launched with.  The launch bound caps the register allocation:
// 1024 threads = 4 waves/SIMD = 128 VGPRs.  The f32 kernels need ~103; the f64 kernels sit at the cap with 10-18 VGPRs
// spilled to scratch (profiles/r03_kernel_resources.json) -- in round 1 the f64 kernel at 4 waves/SIMD with its spills
// measured 7 % faster than at 2 waves/SIMD without, and 5 waves/SIMD (<= 96 VGPRs, 78 spills) loses 32 %.
template <typename real> struct MaxBlock { static constexpr int value = 1024; };

// The workgroup of the 6-waves-per-SIMD entry point (megakernel.hpp pathtrace_kernel_latency): 512 threads, <= 80 VGPRs
constexpr int LatencyBlock = 512;

#if defined(__HIPCC__)
// One plane of a screening record (screen.hpp's kernels make the records): the f64 plane rounded to the nearest f32 (the
// band of walk_round allows for either direction).  A finite f64 plane beyond the f32 range becomes an infinite f32 plane,
// an error TH does not cover (an f32 box that reaches to infinity decides hits that Aabb::hit misses): such a plane sets
// *overflow, and the caller then walks the tree without the screen.
CR_D void screen_plane(double b, float& f, int32_t* overflow) {
    f = (float)b;
    if (__builtin_fabsf(f) == __builtin_inff() && __builtin_fabs(b) != __builtin_inf()) *overflow = 1;
}
CR_D void screen_plane(float b, float& f, int32_t*) { f = b; }
#endif   // __HIPCC__

}   // namespace cr
