// pathtrace.hpp -- the gfx950 path-tracing megakernel and the math it shares with
// the host-side camera set-up.  Hand-written for CDNA4: wave64, one persistent
// launch, scene staged in LDS when it fits, stackless fixed-order BVH walk,
// ballot/prefix regeneration of finished lanes.  No MFMA (branchy traversal).
//
// Reference semantics (citations relative to the Crucible tree):
//   Camera::cast_ray / ray_color / average_samples   src/camera/ray_casting.rs:64-173
//   viewport + basis math                            src/camera/rendering_compute.rs
//   BVHWrapper::hit, Aabb::hit                       src/objects/bvhwrapper.rs:96-126, bvh.rs:96-132
//   Sphere::hit, Triangle::hit                       src/objects/sphere.rs:60-105, triangle.rs:84-140
//   Materials::scatter                               src/materials/{lambertian,metal,dielectric}.rs
//   Textures::value, SkyboxImage::get_color          src/textures/*.rs, src/scene/mod.rs:37-45
//   Point3 / Color / Interval arithmetic             src/utils.rs:78-697
// Every expression keeps the reference's operand order; the build uses
// -ffp-contract=off so no FMA is formed, and IEEE div/sqrt.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#define CR_HD __host__ __device__ __forceinline__
#define CR_D __device__ __forceinline__
#include "fastdiv.hpp"
#include "residency.hpp"   // RES_GLOBAL / RES_LDS / RES_TOP, where the scene is read from, and the rule that picks one
#include "launch_plan.hpp"   // fx_lds_bytes: the LDS of the relaxed sums' slots, and the rest of what sizes a launch

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
// The operand range of Sphere::hit's short quotient (sphere_quot below, where the argument stands): 2^-400 <= |x| < 2^400, read
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

#if defined(__HIPCC__)
// ================================================================== device only

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

template <typename real, typename CT>
CR_D V3<real> image_lookup(const ImageRef* images, const uint32_t* texels, int image, real u, real v, CT& n_texel) {
    ImageRef im = images[image];
    u = clamp01(u);
    v = real(1) - clamp01(v);
    uint32_t i = as_index(u * (real)im.w, im.w);
    uint32_t j = as_index(v * (real)im.h, im.h);
    uint32_t px = texels[im.offset + j * (uint32_t)im.w + i];
    n_texel++;
    return mk<real>((real)(px & 255u) / real(255), (real)((px >> 8) & 255u) / real(255), (real)((px >> 16) & 255u) / real(255));
}

// ------------------------------------------------------------------ software atan2 / asin / acos
// The reference calls f64::atan2 / asin / acos (ray_casting.rs:137-138, sphere.rs:42-43): the platform libm, whose
// last-ulp behaviour differs between glibc and the device's ocml -- enough to move a texel index.  The library and
// the oracle therefore evaluate ONE documented algorithm with +, -, *, /, sqrt only (DESIGN.md "software
// trigonometry"; coefficients from scripts/gen_trig_coeffs.py), which makes the image-texture and spherical-sky
// scenes bit-exact:
//   atan:  fdlibm's argument reduction at 7/16, 11/16, 19/16, 39/16, then atan(t) = t - t*(z*A(z)), z = t*t,
//          result = hi - ((t*(z*A(z)) - lo) - t) with hi + lo = atan(0.5), pi/4, atan(1.5), pi/2;
//   asin:  |x| < 0.5: x + x*(z*S(z)), z = x*x; else pi/2 - 2*asin(sqrt((1 - |x|)/2)); acos likewise;
//   A, S:  Horner from the highest coefficient, multiply then add.  Within 1-3 ulp of the correctly rounded value.
template <typename real> struct TrigK;
template <> struct TrigK<double> {
    static CR_HD double A(double z) {
        double p = -0x1.e4167464d3de8p-7;
        p = p * z + 0x1.0f62bba6a2558p-5; p = p * z + -0x1.7001816fd063fp-5; p = p * z + 0x1.ab59b417b2d3fp-5;
        p = p * z + -0x1.e170800a46210p-5; p = p * z + 0x1.110c9ce7b0572p-4; p = p * z + -0x1.3b1375ce5bdc6p-4;
        p = p * z + 0x1.745d154c84f7ap-4; p = p * z + -0x1.c71c71bd2b8bcp-4; p = p * z + 0x1.2492492485503p-3;
        p = p * z + -0x1.99999999998c5p-3; p = p * z + 0x1.5555555555555p-2;
        return p;
    }
    static CR_HD double S(double z) {
        double p = 0x1.06c051be25377p-5;
        p = p * z + -0x1.dfdd83264a978p-6; p = p * z + 0x1.b20b9dc229eb5p-6; p = p * z + -0x1.641b6703bb104p-9;
        p = p * z + 0x1.1e6dafec868fcp-7; p = p * z + 0x1.c232290f7ae75p-8; p = p * z + 0x1.14f7ebcffc822p-7;
        p = p * z + 0x1.3fa92e3923959p-7; p = p * z + 0x1.7a8b73dc1b007p-7; p = p * z + 0x1.c99964e8e2de8p-7;
        p = p * z + 0x1.1c4ec5dfe81d9p-6; p = p * z + 0x1.6e8ba2e2f8089p-6; p = p * z + 0x1.f1c71c71dc217p-6;
        p = p * z + 0x1.6db6db6db6c75p-5; p = p * z + 0x1.3333333333334p-4; p = p * z + 0x1.5555555555555p-3;
        return p;
    }
    static constexpr double at_hi0 = 0x1.dac670561bb4fp-2, at_lo0 = 0x1.a2b7f222f65e2p-56;   // atan(0.5)
    static constexpr double at_hi1 = 0x1.921fb54442d18p-1, at_lo1 = 0x1.1a62633145c07p-55;   // pi/4
    static constexpr double at_hi2 = 0x1.f730bd281f69bp-1, at_lo2 = 0x1.007887af0cbbdp-56;   // atan(1.5)
    static constexpr double pio2_hi = 0x1.921fb54442d18p+0, pio2_lo = 0x1.1a62633145c07p-54;
    static constexpr double pi_hi = 0x1.921fb54442d18p+1, pi_lo = 0x1.1a62633145c07p-53;
};
template <> struct TrigK<float> {
    static CR_HD float A(float z) {
        float p = -0x1.8b0b06p-5f;
        p = p * z + 0x1.5d79d8p-4f; p = p * z + -0x1.c4f1ecp-4f; p = p * z + 0x1.248626p-3f; p = p * z + -0x1.999968p-3f;
        p = p * z + 0x1.555556p-2f;
        return p;
    }
    static CR_HD float S(float z) {
        float p = 0x1.fb7ca4p-6f;
        p = p * z + 0x1.5a80ap-7f; p = p * z + 0x1.82db24p-6f; p = p * z + 0x1.efedf8p-6f; p = p * z + 0x1.6dc0fp-5f;
        p = p * z + 0x1.33331ep-4f; p = p * z + 0x1.555556p-3f;
        return p;
    }
    static constexpr float at_hi0 = 0.46364760398864746f, at_lo0 = 5.01215868808913e-09f;
    static constexpr float at_hi1 = 0.7853981852531433f, at_lo1 = -2.1855694143368964e-08f;
    static constexpr float at_hi2 = 0.9827937483787537f, at_lo2 = -2.5131424052915463e-08f;
    static constexpr float pio2_hi = 1.5707963705062866f, pio2_lo = -4.371138828673793e-08f;
    static constexpr float pi_hi = 3.1415927410125732f, pi_lo = -8.742277657347586e-08f;
};
// atan(x) for x >= 0 (also +inf; NaN propagates)
template <typename real> CR_HD real soft_atan_pos(real x) {
    using K = TrigK<real>;
    real t, hi = real(0), lo = real(0);
    bool reduced = true;
    if (x < real(0.4375)) { t = x; reduced = false; }
    else if (x < real(0.6875)) { t = (real(2) * x - real(1)) / (real(2) + x); hi = K::at_hi0; lo = K::at_lo0; }
    else if (x < real(1.1875)) { t = (x - real(1)) / (x + real(1)); hi = K::at_hi1; lo = K::at_lo1; }
    else if (x < real(2.4375)) { t = (x - real(1.5)) / (real(1) + real(1.5) * x); hi = K::at_hi2; lo = K::at_lo2; }
    else { t = real(-1) / x; hi = K::pio2_hi; lo = K::pio2_lo; }
    const real z = t * t;
    const real s = t * (z * K::A(z));
    return reduced ? hi - ((s - lo) - t) : t - s;
}
template <typename real> CR_HD real soft_atan2(real y, real x) {
    using K = TrigK<real>;
    if (x != x || y != y) return x + y;
    const bool sx = __builtin_signbit(x), sy = __builtin_signbit(y);
    const real inf = r_inf(real(0));
    if (y == real(0)) return sx ? (sy ? -K::pi_hi : K::pi_hi) : y;
    if (x == real(0)) return sy ? -K::pio2_hi : K::pio2_hi;
    const real ax = r_abs(x), ay = r_abs(y);
    if (ax == inf) {
        if (ay == inf) { const real q = sx ? real(3) * K::at_hi1 : K::at_hi1; return sy ? -q : q; }
        const real q = sx ? K::pi_hi : real(0);
        return sy ? -q : q;
    }
    if (ay == inf) return sy ? -K::pio2_hi : K::pio2_hi;
    const real z = soft_atan_pos(ay / ax);
    const real res = sx ? K::pi_hi - (z - K::pi_lo) : z;
    return sy ? -res : res;
}
template <typename real> CR_HD real soft_asin(real x) {
    using K = TrigK<real>;
    const real ax = r_abs(x);
    if (ax < real(0.5)) { const real z = x * x; return x + x * (z * K::S(z)); }
    if (!(ax <= real(1))) return (x - x) / (x - x);
    const real t = (real(1) - ax) * real(0.5);
    const real s = r_sqrt(t);
    const real res = K::pio2_hi - (real(2) * (s + s * (t * K::S(t))) - K::pio2_lo);
    return x < real(0) ? -res : res;
}
template <typename real> CR_HD real soft_acos(real x) {
    using K = TrigK<real>;
    const real ax = r_abs(x);
    if (ax < real(0.5)) { const real z = x * x; return K::pio2_hi - (x - (K::pio2_lo - x * (z * K::S(z)))); }
    if (!(ax <= real(1))) return (x - x) / (x - x);
    if (x < real(0)) {
        const real t = (real(1) + x) * real(0.5);
        const real s = r_sqrt(t);
        const real w = (t * K::S(t)) * s - K::pio2_lo;
        return K::pi_hi - real(2) * (s + w);
    }
    const real t = (real(1) - x) * real(0.5);
    const real s = r_sqrt(t);
    return real(2) * (s + s * (t * K::S(t)));
}
// What the kernels call (the spherical sky map and Sphere's uv on an image texture: once per missed sample, or never).
// f64: real calls.  Inlined, the ~25 registers of coefficients were hoisted out of the kernels' outer loop and held, or
// spilled, for the whole launch, in frames that never evaluate them too; as callees they load them where they are used.
// The same expressions, so the same bits.  f32: inlined as before (profiles/experiments/uniform_and_decode_ab.txt).
CR_D float r_atan2(float y, float x) { return soft_atan2(y, x); }
CR_D float r_asin(float x) { return soft_asin(x); }
CR_D float r_acos(float x) { return soft_acos(x); }
#define CR_D_CALL static __device__ __attribute__((noinline))
CR_D_CALL double r_atan2(double y, double x) { return soft_atan2(y, x); }
CR_D_CALL double r_asin(double x) { return soft_asin(x); }
CR_D_CALL double r_acos(double x) { return soft_acos(x); }

// random_unit_vector (utils.rs:127-136) and random_in_unit_disk (utils.rs:110-124) for the f64 kernel, with the
// rejection test SCREENED in f32.  A wave leaves a rejection loop only when its slowest lane does (six rounds for a
// unit vector with ~36 lanes drawing), and in f64 most of a round is converting three 64-bit draws to doubles just to
// throw half of them away.  The screen uses the top 24 bits of each draw: xf = -1 + 2*(u >> 40)*2^-24 is EXACT in f32
// and within 2^-23 of the f64 coordinate, so the f32 squared length lf differs from the f64 one by less than 2e-6
// (3 * 2 * 2^-23 from the truncation; lf is one product and two FMAs, each rounded once: < 4e-7 from f32 rounding).  Hence
//     lf > 1 + 1e-5              =>  the reference's test `lensq <= 1` fails      -> next round, nothing converted
//     1e-5 < lf < 1 - 1e-5       =>  it passes (1e-160 < lensq <= 1)             -> leave the loop with the raw draws
// and only a candidate inside the 2e-5 band (or with lf <= 1e-5) is decided by evaluating the reference's f64
// expression on the spot -- a branch no lane takes in ~99.9 % of the rounds.  The accepted candidate is converted to
// f64 once, after the loop, with the reference's expression tree; draws consumed and results are those of the plain
// loop, bit for bit (the parity tests run every f64 scene through this).
CR_D float screen_coord(uint64_t u) {   // -1 + 2 * u01(u, float): (top24 - 2^23) * 2^-23, exact
    return (float)((int32_t)(uint32_t)(u >> 40) - (int32_t)(1 << 23)) * 0x1.0p-23f;
}
template <typename real> CR_D V3<real> random_unit_vector_dev(uint64_t& s) {
    if constexpr (!std::is_same<real, double>::value) return random_unit_vector<real>(s);
    else {
        uint64_t ux, uy, uz;
        for (;;) {
            ux = rng_next(s); uy = rng_next(s); uz = rng_next(s);
            const float fx = screen_coord(ux), fy = screen_coord(uy), fz = screen_coord(uz);
            const float lf = __builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx));
            if (lf > 1.0f + 1e-5f) continue;
            if (lf > 1e-5f && lf < 1.0f - 1e-5f) break;
            const double x = -1.0 + 2.0 * u01(ux, 0.0), y = -1.0 + 2.0 * u01(uy, 0.0), z = -1.0 + 2.0 * u01(uz, 0.0);
            const double lensq = x * x + y * y + z * z;
            if (RealTraits<double>::tiny < lensq && lensq <= 1.0) break;
        }
        // rng_range(-1, 1) = lo + (hi - lo) * u with hi - lo = 2 exactly
        const V3<double> p = mk<double>(-1.0 + 2.0 * u01(ux, 0.0), -1.0 + 2.0 * u01(uy, 0.0), -1.0 + 2.0 * u01(uz, 0.0));
        return divs(p, r_sqrt(len2(p)));
    }
}
template <typename real> CR_D void random_in_unit_disk_dev(uint64_t& s, real& px, real& py) {
    if constexpr (!std::is_same<real, double>::value) {
        for (;;) {
            px = rng_range<real>(s, real(-1), real(1));
            py = rng_range<real>(s, real(-1), real(1));
            if (px * px + py * py + real(0) * real(0) < real(1)) break;
        }
    } else {
        uint64_t ux, uy;
        for (;;) {
            ux = rng_next(s); uy = rng_next(s);
            const float fx = screen_coord(ux), fy = screen_coord(uy);
            const float lf = __builtin_fmaf(fy, fy, fx * fx);
            if (lf > 1.0f + 1e-5f) continue;
            if (lf < 1.0f - 1e-5f) break;
            const double x = -1.0 + 2.0 * u01(ux, 0.0), y = -1.0 + 2.0 * u01(uy, 0.0);
            if (x * x + y * y + 0.0 * 0.0 < 1.0) break;
        }
        px = -1.0 + 2.0 * u01(ux, 0.0); py = -1.0 + 2.0 * u01(uy, 0.0);
    }
}

// Camera::cast_ray's per-sample ray (ray_casting.rs:82-105): seeds the sample's RNG stream and draws
// time, pixel offset and (with defocus) the lens point, in the reference's order.
// ANIM: the kernels for keyed primitives, which also follow a keyed camera (cam.animated, per launch).  CAMK: the
// static-primitive kernels with the camera keys compiled in -- a movie that only moves the camera keeps the static walk
// (the teapot orbit frame: +6.5 % in f64 over running it on the ANIM kernels; folding the camera code into the plain
// static kernels instead cost book1 0.9 % f64 / 1.8 % f32, so it is a variant of its own).
// `current_time`: the frame's first ray time (a frame of a batch has its own; pix_j is then the row within that frame).
// camera_ray_of: the same through a camera record of the caller's choice -- the launch's own, or a view's (KernelArgs::views:
// the record may then differ from lane to lane, and with it cam.animated, cam.defocus_on and the key counts).
template <typename real, bool ANIM, bool CAMK = false>
CR_D void camera_ray_of(const KernelArgs<real>& A, const CamConst<real>& cam, uint32_t pix_i, uint32_t pix_j, int32_t sample, uint64_t& rng, V3<real>& ro,
                        V3<real>& rd, real& rtime, real current_time) {
    uint32_t pixel = pix_j * (uint32_t)cam.W + pix_i;
    rng = rng_key(A.seed_mixed, pixel, (uint32_t)sample);
    real ts = current_time + rng_range<real>(rng, real(0), A.shutter_length);
    real ox = rng_uniform<real>(rng) - real(0.5);   // sample_square, camera/mod.rs:368-376
    real oy = rng_uniform<real>(rng) - real(0.5);
    CamFrame<real> f;
    if ((ANIM || CAMK) && cam.animated) {
        real fx = cam.from.x, fy = cam.from.y, fz = cam.from.z, fw = real(1);
        real ax = cam.at.x, ay = cam.at.y, az = cam.at.z, aw = real(1);
        timeline_eval(A.cam_keys + cam.from_key_first, cam.from_key_count, ts, fx, fy, fz, fw);
        timeline_eval(A.cam_keys + cam.at_key_first, cam.at_key_count, ts, ax, ay, az, aw);
        f = camera_frame(cam, mk<real>(fw * fx, fw * fy, fw * fz), mk<real>(aw * ax, aw * ay, aw * az));
    } else {
        f.from = cam.from; f.p00 = cam.p00; f.pdu = cam.pdu; f.pdv = cam.pdv; f.ddu = cam.ddu; f.ddv = cam.ddv;
    }
    V3<real> ps = add(add(f.p00, scale((real)pix_i + ox, f.pdu)), scale((real)pix_j + oy, f.pdv));   // get_pixel_pos :64-68
    V3<real> orig = f.from;
    if (cam.defocus_on) {   // defocus_disk_sample :104-110, random_in_unit_disk utils.rs:110-124
        real px, py;
        random_in_unit_disk_dev<real>(rng, px, py);
        orig = add(add(f.from, scale(px, f.ddu)), scale(py, f.ddv));
    }
    ro = orig; rd = sub(ps, orig); rtime = ts;
}
template <typename real, bool ANIM, bool CAMK = false>
CR_D void camera_ray(const KernelArgs<real>& A, uint32_t pix_i, uint32_t pix_j, int32_t sample, uint64_t& rng, V3<real>& ro, V3<real>& rd,
                     real& rtime, real current_time) {
    camera_ray_of<real, ANIM, CAMK>(A, A.cam, pix_i, pix_j, sample, rng, ro, rd, rtime, current_time);
}
template <typename real, bool ANIM, bool CAMK = false>
CR_D void camera_ray(const KernelArgs<real>& A, uint32_t pix_i, uint32_t pix_j, int32_t sample, uint64_t& rng, V3<real>& ro, V3<real>& rd,
                     real& rtime) {
    camera_ray<real, ANIM, CAMK>(A, pix_i, pix_j, sample, rng, ro, rd, rtime, A.current_time);
}

// A record of a table that sits either in LDS or in global memory (RES_TOP's materials and textures, decided per
// launch): loaded word by word through an address-space-qualified pointer under a wave-uniform branch, so that the
// compiler emits ds_read / global_load rather than a flat_load through the generic pointer.
template <typename T> CR_D T load_rec(const T* p, bool in_lds) {
    static_assert(sizeof(T) % 4 == 0, "records are whole words");
    T out;
    uint32_t* o = reinterpret_cast<uint32_t*>(&out);
    if (in_lds) {
        const __attribute__((address_space(3))) uint32_t* s = (const __attribute__((address_space(3))) uint32_t*)(const void*)p;
        for (size_t k = 0; k < sizeof(T) / 4; k++) o[k] = s[k];
    } else {
        const __attribute__((address_space(1))) uint32_t* s = (const __attribute__((address_space(1))) uint32_t*)(const void*)p;
        for (size_t k = 0; k < sizeof(T) / 4; k++) o[k] = s[k];
    }
    return out;
}

// The texture a hit at p reads: nested checkers resolved down to a solid or image texture (checker_texture.rs:38-51; at most
// CR_MAX_CHECKER_DEPTH levels, checked at upload).  ti / tx: the material's texture index and record on entry, the leaf's
// on exit.  The parity of the three floors is taken on their wrapping 32-bit sum, as the reference's i32 additions wrap in
// release builds.  A macro rather than a function so that shade() compiles to the code of the loop written in place: as a
// function (by value or by reference, with or without #pragma nounroll) the kernels' code changed and grew by ~5 %.
// tests/shade_check.hip drives it with chosen points.
#define CR_CHECKER_LEAF(tex_at, ti, tx, p)                                                                                          \
    for (int guard = 0; guard < 32 && tx.kind == 1; guard++) {                                                                   \
        int32_t s = (int32_t)((uint32_t)as_i32(r_floor(tx.inv_scale * p.x)) + (uint32_t)as_i32(r_floor(tx.inv_scale * p.y)) +   \
                              (uint32_t)as_i32(r_floor(tx.inv_scale * p.z)));                                                      \
        ti = (s % 2 == 0) ? tx.even : tx.odd;                                                                                    \
        tx = tex_at(ti);                                                                                                         \
    }

// What ray_color does after the closest-hit query (ray_casting.rs:122-151) for a path whose hit is
// (best_t, best) -- best < 0 is a miss.  Returns true when the path is finished (col = the colour the
// outermost ray_color call returns), false when it scattered (ro/rd replaced, depth_left decremented).
// The path's non-unit attenuations live at att_stack[(level * stack_stride + stack_slot) * 3 .. +2]: one record per
// level, so a push is one contiguous store and an unwind step one contiguous load.
// RELAX (CR_SUM_RELAXED): no stack -- *thr carries the product of the attenuations met so far (a_1 * a_2 * ... in path
// order; the same multiplies as the reference's a_1 * (a_2 * (...)), associated the other way) and the colour handed
// back is thr * sky.  Every factor is in [0, 1] or NaN, so Color's clamp (utils.rs:553-563) never changes a product.
template <typename real, bool ANIM, bool SIDE_SPLIT = false, bool RELAX = false, typename CT = uint32_t>
CR_D bool shade(const KernelArgs<real>& A, const Prim<real>* prims, const Mat<real>* mats, const Tex<real>* texs, V3<real>& ro, V3<real>& rd,
                real rtime, uint64_t& rng, int32_t& depth_left, int32_t& stack_n, real best_t, int32_t best, uint32_t stack_stride,
                uint32_t stack_slot, CT& c_tex, V3<real>& col, Diag* dg = nullptr, V3<real>* thr = nullptr, const real* dd = nullptr) {
    CR_DIAG_HIT(dg, DG_SHADE_WAVE, DG_SHADE_LANE);
    // unit(rd) of the incoming ray.  dd: the segment's |rd|^2 where the caller has it (WalkState::dd, walk_begin's len2(rd) of
    // this rd: the same expression on the same operands, and -ffp-contract=off keeps it the same bits)
    auto unit_rd = [&]() -> V3<real> { return divs(rd, r_sqrt(dd ? *dd : len2(rd))); };
    if (best >= 0) {
        CR_DIAG_HIT(dg, DG_HITSH_WAVE, DG_HITSH_LANE);
        const Prim<real>& p = prims[best];
        V3<real> loc = add(ro, scale(best_t, rd));   // Ray::at
        V3<real> n;
        real tu = 0, tv = 0;
        // SIDE_SPLIT (RES_TOP): the two tables are in LDS or in global memory, per launch
        auto mat_at = [&](int32_t i) { return SIDE_SPLIT ? load_rec(mats + i, A.lds_side != 0) : mats[i]; };
        auto tex_at = [&](int32_t i) { return SIDE_SPLIT ? load_rec(texs + i, A.lds_side != 0) : texs[i]; };
        const Mat<real> m = mat_at(p.mat());
        bool need_uv = false;
        int32_t leaf_tex = -1;
        if (m.kind == 0 && m.tex >= 0) {   // only image textures read u,v
            int ti = m.tex;
            Tex<real> tx = tex_at(ti);
            CR_CHECKER_LEAF(tex_at, ti, tx, loc)
            need_uv = tx.kind == 2;
            leaf_tex = ti;
        }
        if (p.kind() == 0) {
            real g0 = p.g[0], g1 = p.g[1], g2 = p.g[2], g3 = p.g[3];
            if (ANIM && p.key_count) {
                timeline_eval(A.keys + p.key_first, p.key_count, rtime, g0, g1, g2, g3);
                n = divs(sub(loc, mk<real>(g0, g1, g2)), g3);   // sphere.rs:97
            } else n = scale(p.g[4], sub(loc, mk<real>(g0, g1, g2)));   // p.g[4] = 1/radius
            if (need_uv) {                                  // get_sphere_uv, sphere.rs:41-46
                real theta = r_acos(-n.y);
                real phi = r_atan2(-n.z, n.x) + RealTraits<real>::pi;
                tu = phi / (real(2) * RealTraits<real>::pi);
                tv = theta / RealTraits<real>::pi;
            }
        } else {
            V3<real> a = mk<real>(p.g[0], p.g[1], p.g[2]), b = mk<real>(p.g[3], p.g[4], p.g[5]), c = mk<real>(p.g[6], p.g[7], p.g[8]);
            if (ANIM && p.key_count) {
                a = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, a);
                b = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, b);
                c = timeline_vertex(A.keys + p.key_first, p.key_count, rtime, c);
            }
            n = unit(cross(sub(b, a), sub(c, a)));          // safe_new, objects/mod.rs:76
            tu = 0; tv = 0;                                 // triangle.rs:130-131
        }
        bool front = dot(rd, n) < real(0);                  // HitRecord::new
        if (!front) n = neg(n);

        V3<real> att = mk<real>(0, 0, 0), ndir = rd;
        bool some;
        // Lambertian and Metal both begin their draws with random_unit_vector() (lambertian.rs:41,
        // metal.rs:31): one shared pass of the rejection loop serves both groups of lanes
        V3<real> ruv = mk<real>(0, 0, 0);
#ifdef CR_DIAG
        if (m.kind != 2) {   // random_unit_vector with its rounds counted
            for (;;) {
                CR_DIAG_HIT(dg, DG_RUV_WAVE, DG_RUV_LANE);
                real x = rng_range<real>(rng, real(-1), real(1)), y = rng_range<real>(rng, real(-1), real(1)), z = rng_range<real>(rng, real(-1), real(1));
                V3<real> pp = mk<real>(x, y, z);
                real lensq = len2(pp);
                if (RealTraits<real>::tiny < lensq && lensq <= real(1)) { ruv = divs(pp, r_sqrt(lensq)); break; }
            }
        }
        CR_DIAG_LANE(dg, m.kind == 0 ? DG_LAMB_LANE : (m.kind == 1 ? DG_METAL_LANE : DG_DIEL_LANE));
#else
        if (m.kind != 2) ruv = random_unit_vector_dev<real>(rng);
#endif
        if (m.kind == 0) {                                  // lambertian.rs:40-61
            V3<real> dir = add(n, ruv);
            real tol = real(1e-8);
            if (r_abs(dir.x) < tol && r_abs(dir.y) < tol && r_abs(dir.z) < tol) dir = n;
            V3<real> tc;
            if (m.tex < 0) tc = mk<real>(m.albedo[0], m.albedo[1], m.albedo[2]);
            else {
                const Tex<real> lt = tex_at(leaf_tex);
                if (need_uv) tc = image_lookup(A.images, A.texels, lt.image, tu, tv, c_tex);
                else tc = mk<real>(lt.color[0], lt.color[1], lt.color[2]);
            }
            att = c_scale(m.aux, (m.param < real(0)) ? c_neg(tc) : tc);   // tc / scatter_prob
            ndir = dir;
            // Lambertian scatters when a uniform draw u <= scatter_prob (lambertian.rs:55).  u = k * 2^-53 (2^-24 in f32)
            // with k below 2^53 (2^24), so u <= 1 - 2^-53 < 1 and the test holds whatever the draw once scatter_prob >= 1:
            // every Lambertian of the book scenes.  When all Lambertian lanes of the wave are of that kind (one ballot, a
            // scalar branch) the stream advances by its state step alone -- the output multiply (64-bit, quarter rate) and
            // the conversion are never formed.  A smaller or NaN probability in any lane: the reference's test, whole wave.
            if (__ballot(!(m.param >= real(1))) == 0ull) { rng_step(rng); some = true; }
            else some = rng_uniform<real>(rng) <= m.param;
        } else if (m.kind == 1) {                           // metal.rs:29-42
            V3<real> refl = reflect(rd, n);
            refl = add(unit(refl), scale(m.param, ruv));
            att = mk<real>(m.albedo[0], m.albedo[1], m.albedo[2]);
            ndir = refl;
            some = dot(refl, n) > real(0);
        } else {                                            // dielectric.rs:30-55
            att = mk<real>(1, 1, 1);
            real ri = front ? m.albedo[0] : m.param;
            V3<real> ud = unit_rd();
            real cos_theta = -(r_fmin(dot(ud, n), real(1)));
            real sin_theta = r_sqrt(real(1) - cos_theta * cos_theta);
            bool refl = ri * sin_theta > real(1);
            if (!refl) {
                real r0 = front ? m.albedo[1] : m.albedo[2];
                real x = real(1) - cos_theta;
                real x2 = x * x;
                real x5 = x * (x2 * x2);
                refl = (r0 + (real(1) - r0) * x5) > rng_uniform<real>(rng);
            }
            ndir = refl ? reflect(ud, n) : refract(ud, n, ri);
            some = true;
        }
        if (!some) { col = mk<real>(0, 0, 0); return true; }   // scatter None -> black
        // attenuation * ray_color(scattered): the product is formed innermost-first, so remember the
        // factor and multiply on the way back (ray_casting.rs:128).  (1,1,1) multiplies exactly and
        // need not be stored.
        if (m.kind != 2) {
            if constexpr (RELAX) { thr->x = thr->x * att.x; thr->y = thr->y * att.y; thr->z = thr->z * att.z; }
            else {
                real* rec = A.att_stack + ((size_t)stack_n * stack_stride + stack_slot) * 3;
                rec[0] = att.x; rec[1] = att.y; rec[2] = att.z;
                stack_n++;
            }
        }
        ro = loc; rd = ndir; depth_left--;
        return false;
    }
    // sky (ray_casting.rs:133-151)
    CR_DIAG_LANE(dg, DG_SKY_LANE);
    V3<real> ud = unit_rd();
    if (A.sky_kind == 1) {
        real theta = r_atan2(ud.x, ud.z);
        real phi = r_asin(ud.y);
        real u = (theta / (real(2) * RealTraits<real>::pi)) + real(0.5);
        real v = (phi / RealTraits<real>::pi) + real(0.5);
        col = image_lookup(A.images, A.texels, A.sky_image, u, v, c_tex);
    } else {
        real a = real(0.5) * (ud.y + real(1));
        col = c_add(c_scale(real(1) - a, mk<real>(1, 1, 1)), c_scale(a, mk<real>(real(0.5), real(0.7), real(1))));
    }
    if constexpr (RELAX) { col = mk<real>(thr->x * col.x, thr->y * col.y, thr->z * col.z); return true; }
    // unwind: a_1 * (a_2 * ( ... (a_n * sky))).  The factors live in global memory; four levels are fetched
    // per round trip and applied innermost-first, so the product is formed in the reference's order.
    int32_t k = stack_n - 1;
    for (; k >= 3; k -= 4) {
        CR_DIAG_HIT(dg, DG_UNWIND_WAVE, DG_UNWIND_LANE);
        V3<real> a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const real* rec = A.att_stack + ((size_t)(k - j) * stack_stride + stack_slot) * 3;
            a[j] = mk<real>(rec[0], rec[1], rec[2]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) col = c_mul(a[j], col);
    }
    for (; k >= 0; k--) {
        CR_DIAG_HIT(dg, DG_UNWIND_WAVE, DG_UNWIND_LANE);
        const real* rec = A.att_stack + ((size_t)k * stack_stride + stack_slot) * 3;
        V3<real> a_k = mk<real>(rec[0], rec[1], rec[2]);
        col = c_mul(a_k, col);
    }
    return true;
}

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
          typename CN = unsigned long long, typename CP = uint32_t>
CR_D void walk_round(const KernelArgs<real>& A, const Entry<real>* lds_entries, const Prim<real>* prims, V3<real> ro, V3<real> rd, real rtime,
                     WalkState<real>& w, bool walking, uint32_t budget, CN& c_node, CP& c_prim, Diag* dg = nullptr,
                     const void* lds_screen = nullptr) {
    constexpr bool COUNT = !std::is_same<CN, NoCount>::value;
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
                    uint32_t off = base + ((uint32_t)w.idx << 5), after_leaf = 0;
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
                        w.idx = (int32_t)((off - base) >> 5);
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
    // The parked lanes intersect their leaves together; with walk_leaf_min set, a thin group waits (parked) while other lanes
    // of the wave can still step, so that the expensive primitive test runs with more lanes.  Per lane the sequence of
    // operations is unchanged: a parked lane does nothing until its leaf is tested.
    w.pending = leaf;
    if (A.walk_leaf_min > 0u) {
        const uint32_t parked = (uint32_t)__popcll(__ballot(leaf >= 0));
        const bool can_step = __ballot(walking && leaf < 0 && w.idx < n_entries) != 0ull;
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

// Diagnostic build: per-wave phase clocks go to counters[9..12] (regeneration, walk, shade, total).
#ifdef CR_DIAG
#define CR_DIAG_ONLY(...) __VA_ARGS__
#else
#define CR_DIAG_ONLY(...)
#endif

// TRACE: has a ray whose walk has not begun; WALK: walking (state kept across rounds of the outer loop);
// SHADE: closest hit known.
enum : int { ST_NEED_PIXEL = 0, ST_NEED_SAMPLE = 1, ST_TRACE = 2, ST_DONE = 3, ST_WALK = 4, ST_SHADE = 5 };

// Largest workgroup the kernels may be launched with.  The launch bound caps the register allocation:
// 1024 threads = 4 waves/SIMD = 128 VGPRs.  The f32 kernels need ~103; the f64 kernels sit at the cap with 10-18 VGPRs
// spilled to scratch (profiles/r03_kernel_resources.json) -- in round 1 the f64 kernel at 4 waves/SIMD with its spills
// measured 7 % faster than at 2 waves/SIMD without, and 5 waves/SIMD (<= 96 VGPRs, 78 spills) loses 32 %.
template <typename real> struct MaxBlock { static constexpr int value = 1024; };

// How many lanes below this one are set in a ballot: v_mbcnt on the ballot's scalar halves, no per-lane mask
CR_D uint32_t wave_rank(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// What stage_scene answers: the staged copies, else the launch's global tables (lds_entries, lds_screen: null); `end`: the first LDS byte behind the scene
template <typename real> struct SceneStage {
    const Entry<real>* lds_entries;
    const void* lds_screen;
    const Prim<real>* prims;
    const Mat<real>* mats;
    const Tex<real>* texs;
    size_t end;
};

// Stages the scene in LDS as residency.hpp's scene_layout lays it out, whole workgroup, barrier at the end.  RES_LDS: all
// records, primitives, materials, textures; RES_TOP: the window of A.lds_entries records and, where A.lds_side says so,
// materials and textures; RES_GLOBAL: nothing.  SCREEN kernels stage the f32 screening records instead of the wrappers
// (twice as many in the same bytes); with the whole tree there (RES_LDS) the caller then turns the records' links into LDS
// addresses, after this routine's barrier and before one of its own -- the loop stands in pathtrace_body and aov_body,
// because in here (or in any function) it changes nine reference-order and f32 megakernels.
// SIDE = false: geometry only -- a kernel that does not shade (wf_extend_kernel).
// It names the extern __shared__ array itself (as an argument the array is a generic pointer and the whole kernel's register
// allocation moves), and keeps the shape the kernels' text was settled with (scripts/isa_diff.py).
template <typename real, int RES, bool ORD, bool SCREEN, bool SIDE = true>
CR_D SceneStage<real> stage_scene(const KernelArgs<real>& A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Entry<real>* lds_entries = nullptr;
    const void* lds_screen = nullptr;
    const Prim<real>* prims = A.prims;
    const Mat<real>* mats = A.mats;
    const Tex<real>* texs = A.texs;
    size_t end = 0;
    if (RES != RES_GLOBAL) {
        auto copy = [&](const void* src, size_t off, size_t bytes) {
            const uint32_t* s = (const uint32_t*)src;
            uint32_t* d = (uint32_t*)(smem + off);
            for (size_t i = threadIdx.x; i < bytes / 4; i += blockDim.x) d[i] = s[i];
        };
        using ScreenT = typename ScreenOf<ORD>::type;
        constexpr size_t window_rec = SCREEN ? sizeof(ScreenT) : sizeof(typename EntryOf<real, ORD>::type);
        copy(SCREEN ? A.screen : (const void*)A.entries, 0, (size_t)A.lds_entries * window_rec);
        lds_entries = (const Entry<real>*)smem;
        if (SCREEN) lds_screen = (const void*)smem;
        if (RES == RES_LDS) {   // the whole scene
            const SceneLayout L = scene_layout((size_t)A.n_entries * window_rec, (size_t)A.n_prims * sizeof(Prim<real>), (size_t)A.n_mats * sizeof(Mat<real>),
                                               (size_t)A.n_texs * sizeof(Tex<real>), true, SIDE);
            copy(A.prims, L.prims, (size_t)A.n_prims * sizeof(Prim<real>));
            if (SIDE) {
                copy(A.mats, L.mats, (size_t)A.n_mats * sizeof(Mat<real>));
                copy(A.texs, L.texs, (size_t)A.n_texs * sizeof(Tex<real>));
            }
            prims = (const Prim<real>*)(smem + L.prims);
            if (SIDE) {
                mats = (const Mat<real>*)(smem + L.mats);
                texs = (const Tex<real>*)(smem + L.texs);
            }
            end = L.end();
        } else if (SIDE && A.lds_side) {   // RES_TOP: the window, and the side tables behind it
            const SceneLayout L = scene_layout((size_t)A.lds_entries * window_rec, 0, (size_t)A.n_mats * sizeof(Mat<real>), (size_t)A.n_texs * sizeof(Tex<real>), false, true);
            copy(A.mats, L.mats, (size_t)A.n_mats * sizeof(Mat<real>));
            copy(A.texs, L.texs, (size_t)A.n_texs * sizeof(Tex<real>));
            mats = (const Mat<real>*)(smem + L.mats);
            texs = (const Tex<real>*)(smem + L.texs);
            end = L.end();
        } else end = scene_layout((size_t)A.lds_entries * window_rec, 0, 0, 0, false, false).end();   // RES_TOP: the window alone
        __syncthreads();
    }
    return {lds_entries, lds_screen, prims, mats, texs, end};
}

// The persistent kernel body.  A work item is one (pixel, sample) handed out in chunks from one global counter (sample-granular
// mode, the default); the reference-order variants keep per-sample colours for the ordered sum, the RELAX variants add into
// fixed-point per-pixel sums.  (sg_on = 0, a fallback: one lane owns a pixel and sums its samples in draw order itself.)
// RELAX: CR_SUM_RELAXED -- the same paths (same draws, same walks, same counters); a finished sample's colour is
// thr * sky and goes into fixed-point per-pixel sums.  Each wave owns two LDS accumulators, one work tile (<= 16
// pixels x 3 channels) each: ds_add_u64 there, and one global atomic per word when the wave moves on to another tile
// -- about 48 global atomics per 1024 samples instead of 3 per sample (global atomics execute at the memory side, one
// request per lane when the lanes' addresses are scattered).  A straggler whose tile has already been flushed adds to
// the global sums directly.
// BATCH: the kernels that render a batch of frames (KernelArgs::n_frames) -- the RELAX kernels movies run on, with a keyed
// camera (CAMK) or keyed primitives (ANIM); a batch of a scene without keys runs on the CAMK kernel.  The static kernels
// (the stills, the headline among them) do not carry the frame arithmetic: in them it moved the register allocation.
// The ~70 launch parameters are read where they are used, through the kernarg segment's own address (constant address
// space: s_load, served by the scalar cache).  As a by-value parameter they were all loaded at kernel entry and stayed
// live for the whole launch: the f64 kernel spilled 97 of them to VGPR lanes (230 v_readlane / v_writelane, 20 VGPRs
// pushed to scratch); read this way it spills 6 (19, and 6).
template <typename real> CR_D const KernelArgs<real>& kernel_args() {
    return *(const KernelArgs<real>*)(const __attribute__((address_space(4))) KernelArgs<real>*)__builtin_amdgcn_kernarg_segment_ptr();
}
// REG: the body carries a region's offsets where it carries the frame arithmetic (BATCH).  The 6-waves-per-SIMD entry point
// passes false: at its 80 VGPRs the offsets cost spills, so region renders stay on pathtrace_kernel (render.hpp walk_ladder)
// and the latency kernels compile to what they were.  A parameter of the body, not of a kernel: the kernels stay the same set.
// LIST: the work decode names its tiles through KernelArgs::tile_list (cr_render_adaptive_*).  Only pathtrace_kernel_listed
// passes true: read in the kernels that movies and regions run on, the list cost them 0.3 - 0.8 % at unchanged registers
// (profiles/experiments/adaptive_sampling.txt), so it has kernels of its own and every other kernel compiles to what it was.
// COUNT: the body keeps the four work counters and adds them to KernelArgs::counters at its end.  Only pathtrace_kernel_quiet
// passes false: its launches are the renders whose caller asked for no stats (render.hpp launch()).
// VIEWS: a frame of the batch is a view with a camera of its own (KernelArgs::views, cr_render_views_*).  Only
// pathtrace_kernel_views passes true: the camera record becomes a per-lane read from global memory, so every other kernel
// keeps its camera in the kernarg segment and compiles to what it was.
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK = false, bool RELAX = false, bool SCREEN = false, bool REG = true, bool LIST = false, bool COUNT = true,
          bool VIEWS = false>
CR_D void pathtrace_body(const KernelArgs<real>& A) {
    constexpr bool BATCH = RELAX && (ANIM || CAMK);
    constexpr bool REGION = BATCH && REG;
    static_assert(!VIEWS || REGION, "the views' kernels are batch kernels");
    // REGION: the region's words (reg_x0 .. reg_h) are read through the kernarg segment where they are used, also in the
    // kernels that keep the by-value parameter: there they would be four more scalars alive for the whole launch
    const KernelArgs<real>& RG = kernel_args<real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // (RELAX: the waves' slots behind the scene)
#ifdef CR_HOLD_VCC
    unsigned long long vcc_hold;
    asm volatile("s_mov_b64 %0, 0" : "={vcc}"(vcc_hold));
#endif
    const SceneStage<real> S = stage_scene<real, RES, ORD, SCREEN>(A);
    const Entry<real>* lds_entries = S.lds_entries;
    const void* lds_screen = S.lds_screen;
    const Prim<real>* prims = S.prims;
    const Mat<real>* mats = S.mats;
    const Tex<real>* texs = S.texs;
    if constexpr (SCREEN && RES == RES_LDS) {   // links of the staged screening records become LDS addresses (fetch_screen, fetch_screen_ordered)
        using ScreenT = typename ScreenOf<ORD>::type;
        const uint32_t base = screen_lds_base<RES>(smem);
        ScreenT* rec = (ScreenT*)smem;
        for (int32_t i = (int32_t)threadIdx.x; i < A.n_entries; i += (int32_t)blockDim.x) {
            if constexpr (ORD) { for (int k = 0; k < 8; k++) rec[i].skip[k] += base; }
            else rec[i].skip += base;
            if (!(rec[i].hit & kScreenLeaf)) rec[i].hit += base;
        }
        __syncthreads();
    }

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
    // RELAX: this wave's two accumulator slots and the tiles they hold (wave-uniform; kFxNoTile = empty)
    constexpr uint32_t kFxNoTile = 0xffffffffu;
    unsigned long long* fx_slots = nullptr;
    uint32_t fx_tile0 = kFxNoTile, fx_tile1 = kFxNoTile, fx_mru = 0;
    V3<real> thr = mk<real>(1, 1, 1);
    const uint32_t fx_words = 3u << (A.sg_lw + A.sg_lh);   // words per slot
    if constexpr (RELAX) {
        fx_slots = (unsigned long long*)(smem + A.fx_lds_off) + (size_t)(threadIdx.x >> 6) * 2 * fx_words;
        for (uint32_t k = lane; k < 2 * fx_words; k += 64) fx_slots[k] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    // adds a slot's sums to the global ones and empties it (whole wave; `tile` is wave-uniform)
    auto fx_flush = [&](uint32_t slot, uint32_t tile) {
        if constexpr (RELAX) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (tile != kFxNoTile) {
                uint32_t ti, tj;
                tile_xy(A, tile, ti, tj);
                ti <<= A.sg_lw; tj <<= A.sg_lh;
                // BATCH: the tile's first row in fx_acc, where a batch's frames are H rows apart (tiles_y << sg_lh in pix_j)
                if constexpr (BATCH) tj -= batch_frame(A, tj) * ((A.tiles_y << A.sg_lh) - (REGION ? RG.reg_h : (uint32_t)A.cam.H));
                for (uint32_t k = lane; k < fx_words; k += 64) {   // 48 words for the usual 4 x 4 tile: one pass
                    unsigned long long* w = fx_slots + slot * fx_words + k;
                    const unsigned long long v = *w;
                    if (v) {
                        *w = 0ull;
                        const uint32_t px = k / 3u, ch = k - px * 3u;
                        const uint32_t pi = ti + (px & ((1u << A.sg_lw) - 1u)), pj = tj + (px >> A.sg_lw);
                        unsigned long long* g;   // (REGION: fx_acc's rows are the region's)
                        if constexpr (REGION) g = A.fx_acc + ((size_t)pj * (size_t)RG.reg_w + pi) * 3 + ch;
                        else g = A.fx_acc + ((size_t)pj * (size_t)A.cam.W + pi) * 3 + ch;
                        if (v & ~kFxNaN) atomicAdd(g, v & ~kFxNaN);
                        if (v & kFxNaN) atomicOr(g, kFxNaN);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
    };
    const uint32_t total_work = (A.sg_on || RELAX) ? A.sg_total : A.tiles_x * A.tiles_y * 64u;
    const CamConst<real>& cam = A.cam;
    // sample-granular mode: the wave's private slice [wv_next, wv_end) of the work counter (same value in all lanes)
    uint32_t wv_next = 0, wv_end = 0;
    const uint32_t SG_CHUNK = A.sg_chunk;   // items a wave takes per atomic: 1024 for long launches, fewer for short ones (launch())

    int state = ST_NEED_PIXEL;
    uint32_t pix_i = 0, pix_j = 0;
    uint32_t item = 0;   // sample-granular mode: the lane's current work item
    int32_t sample = 0;
    real acc_r = 0, acc_g = 0, acc_b = 0;
    // path state
    V3<real> ro = mk<real>(0, 0, 0), rd = mk<real>(0, 0, 1);
    real rtime = 0;
    uint64_t rng = 0;
    int32_t depth_left = 0, stack_n = 0;
    std::conditional_t<COUNT, uint32_t, NoCount> c_seg{}, c_prim{}, c_tex{};
    std::conditional_t<COUNT, unsigned long long, NoCount> c_node{};
    // walk state, kept across rounds: a lane whose walk is cut short resumes where it stopped
    WalkState<real> ws;
    ws.inv = mk<real>(0, 0, 0); ws.dd = 0; ws.rda = quot_divide<real>(); ws.best_t = 0; ws.best = -1; ws.idx = 0; ws.exact_box = false; ws.pending = -1;
    constexpr bool LAZY = lazy_inv<real, RES, ANIM, ORD, CAMK, SCREEN>();   // walk_begin_screened / walk_round's LAZY_INV
    if constexpr (LAZY) { ws.invf = mk<float>(0, 0, 0); ws.unscreened = false; }
    const int32_t n_entries = A.n_entries;
    // read once, into a scalar register that stays: a load at every walk_begin would wait with the LDS reads around it
    uint32_t exact_tree = tree_walks_exact(A) ? 1u : 0u;
    if constexpr (std::is_same<real, float>::value) {
        exact_tree = (uint32_t)__builtin_amdgcn_readfirstlane((int)exact_tree);
        asm volatile("" : "+s"(exact_tree));
    }

    Diag* dgp = nullptr;
    CR_DIAG_ONLY(Diag dg_store; for (int i = 0; i < DG_N; i++) dg_store.v[i] = 0; dgp = &dg_store;
                 unsigned long long d_t_regen = 0, d_t_trace = 0, d_t_shade = 0;
                 unsigned long long d_t0 = __builtin_readcyclecounter(); const unsigned long long d_begin = d_t0;)
    for (;;) {
        CR_DIAG_ONLY(if (CR_DIAG_LEADER()) dg_store.v[DG_OUTER_WAVE]++; d_t0 = __builtin_readcyclecounter();)
        // ---------------- regeneration: pixels
        uint64_t need = __ballot(state == ST_NEED_PIXEL);
        if (need && (A.sg_on || RELAX)) {
            // One (pixel, sample) per lane.  The wave takes SG_CHUNK consecutive items from the global counter at a
            // time and hands them to its lanes in order, so a wave stays on one tile's samples (coherent rays) and
            // the counter sees one atomic per 1024 samples.
            const uint32_t cnt = (uint32_t)__popcll(need), avail = wv_end - wv_next;
            uint32_t fresh = 0;
            uint32_t my_tile = kFxNoTile;   // the tile of the item this lane takes in this round
            if (cnt > avail) {
                const int leader = __ffsll((unsigned long long)need) - 1;
                if ((int)lane == leader) fresh = atomicAdd(A.work_counter, SG_CHUNK);
                fresh = (uint32_t)__builtin_amdgcn_readlane((int)fresh, leader);   // a scalar: the cursor stays in scalar registers
            }
            if (state == ST_NEED_PIXEL) {
                const uint32_t rank = wave_rank(need);
                // past the end of the counter's range (also when it wrapped): nothing left
                const uint32_t w = rank < avail ? wv_next + rank : fresh + (rank - avail);
                if (w >= total_work) state = ST_DONE;
                else {
                    item = w;
                    const uint32_t group = w >> 6, in = w & 63u;
                    uint32_t tile = fastdiv(group, A.fd_groups);
                    const uint32_t sg = group - tile * A.sg_groups;
                    // LIST: a launch that names its tiles (KernelArgs::tile_list) -- the frame's own tile number from here on
                    if constexpr (REGION && LIST) { const int32_t* const listed = RG.tile_list; if (listed) tile = (uint32_t)listed[tile]; }
                    uint32_t tx, ty;
                    tile_xy(A, tile, tx, ty);
                    my_tile = tile;
                    const uint32_t px = in & ((1u << A.sg_lw) - 1u), py = (in >> A.sg_lw) & ((1u << A.sg_lh) - 1u);
                    const uint32_t ds = in >> (A.sg_lw + A.sg_lh);
                    pix_i = (tx << A.sg_lw) + px;
                    pix_j = (ty << A.sg_lh) + py;
                    // the offset in the shard decides: begin + offset may pass INT32_MAX in the last group's padding, and wraps
                    const uint32_t s_off = sg * (64u >> (A.sg_lw + A.sg_lh)) + ds;
                    sample = (int32_t)((uint32_t)A.sample_begin + s_off);
                    uint32_t row = pix_j;   // BATCH: pix_j counts the rows of a whole batch; the frame's own row decides
                    if constexpr (BATCH) row -= batch_frame(A, pix_j) * (A.tiles_y << A.sg_lh);
                    bool inside;   // (REGION: inside the region, which is the whole frame unless a region was asked for)
                    if constexpr (REGION) inside = pix_i < RG.reg_w && row < RG.reg_h;
                    else inside = pix_i < (uint32_t)cam.W && row < (uint32_t)cam.H;
                    if (inside && s_off < (uint32_t)(A.sample_end - A.sample_begin)) state = ST_NEED_SAMPLE;
                    // else: padding of an edge tile or of the last sample group, ask again next round
                    // REGION: from here on the lane keeps the pixel at the frame's origin (the region's offset added once,
                    // to integers): camera_ray reads it as it is, the sums' addresses take the offset off again -- kept
                    // the other way round, the sums of the offsets were two more registers alive through camera_ray
                    if constexpr (REGION) { pix_i += RG.reg_x0; pix_j += RG.reg_y0; }
                }
            }
            if (cnt > avail) { wv_next = fresh + (cnt - avail); wv_end = fresh + SG_CHUNK; }
            else wv_next += cnt;
            if constexpr (RELAX) {
                // make room for the tiles this round's new items belong to (consecutive items: one or two tiles)
                uint64_t fresh_items = __ballot(state == ST_NEED_SAMPLE) & need;
                while (fresh_items) {
                    const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)my_tile, __ffsll((unsigned long long)fresh_items) - 1);
                    fresh_items &= ~__ballot(my_tile == t);
                    if (t == fx_tile0) fx_mru = 0;
                    else if (t == fx_tile1) fx_mru = 1;
                    else if (fx_mru == 0) { fx_flush(1, fx_tile1); fx_tile1 = t; fx_mru = 1; }
                    else { fx_flush(0, fx_tile0); fx_tile0 = t; fx_mru = 0; }                }
            }
        } else if (need) {
            uint32_t cnt = (uint32_t)__popcll(need);
            uint32_t base = 0;
            int leader = __ffsll((unsigned long long)need) - 1;
            if ((int)lane == leader) base = atomicAdd(A.work_counter, cnt);
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
            if (state == ST_NEED_PIXEL) {
                uint32_t rank = wave_rank(need);
                uint32_t w = base + rank;
                if (w >= total_work) state = ST_DONE;
                else {
                    uint32_t tile = w >> 6, in = w & 63u;
                    uint32_t tx, ty;
                    tile_xy(A, tile, tx, ty);
                    pix_i = tx * 8u + (in & 7u);
                    pix_j = ty * 8u + (in >> 3);
                    if (pix_i < (uint32_t)cam.W && pix_j < (uint32_t)cam.H) {
                        state = ST_NEED_SAMPLE; sample = A.sample_begin; acc_r = acc_g = acc_b = 0;
                    }   // else: padding of an edge tile, ask again next round
                }
            }
        }
        if (__ballot(state != ST_DONE) == 0) break;

        // ---------------- regeneration: camera rays (cast_ray, ray_casting.rs:82-105)
        if (state == ST_NEED_SAMPLE) {
            CR_DIAG_HIT(dgp, DG_REGEN_WAVE, DG_REGEN_LANE);
            if constexpr (BATCH) {   // a frame of a batch: its own row and its own ray times; a region: the frame's own pixel, as one integer
                const uint32_t f = batch_frame(A, REGION ? pix_j - RG.reg_y0 : pix_j);
                if constexpr (VIEWS)   // the lane's view: its camera record, read where camera_ray uses it
                    camera_ray_of<real, ANIM, CAMK>(A, RG.views[f], pix_i, pix_j - f * (A.tiles_y << A.sg_lh), sample, rng, ro, rd, rtime,
                                                    A.n_frames > 1u ? A.frame_times[f] : A.current_time);
                else
                camera_ray<real, ANIM, CAMK>(A, pix_i, pix_j - f * (A.tiles_y << A.sg_lh), sample, rng, ro, rd, rtime,
                                             A.n_frames > 1u ? A.frame_times[f] : A.current_time);
            } else camera_ray<real, ANIM, CAMK>(A, pix_i, pix_j, sample, rng, ro, rd, rtime);
            depth_left = A.max_depth; stack_n = 0;
            if constexpr (RELAX) thr = mk<real>(1, 1, 1);
            state = ST_TRACE;
        }

        CR_DIAG_ONLY({ unsigned long long t = __builtin_readcyclecounter(); d_t_regen += t - d_t0; d_t0 = t; })
        // ---------------- closest hit (Hittables::hit on the BVH root, interval (0.001, inf))
        V3<real> col = mk<real>(0, 0, 0);   // colour returned by the innermost ray_color call
        bool finished = false;
        if (state == ST_TRACE) {
            if (depth_left == 0) finished = true;   // ray_color: depth == 0 -> black
            else {
                c_seg++;
                if constexpr (LAZY) walk_begin_screened<quot_form<real, RES, ANIM, SCREEN>() == 1>(ws, ro, rd);
                else walk_begin<quot_form<real, RES, ANIM, SCREEN>() == 1>(ws, rd, exact_tree != 0u);
                state = n_entries > 0 ? ST_WALK : ST_SHADE;
            }
        }
        // Rounds of the while-while walk (walk_round).  After each round the wave may leave the walk if enough
        // lanes are done: the stragglers keep their WalkState and resume on the next round of the outer loop, so
        // each lane still performs BVHWrapper::hit's exact sequence; only the interleaving with other lanes'
        // shading changes.
        if (__ballot(state == ST_WALK)) {
            for (;;) {
                walk_round<real, RES, ANIM, ORD, SCREEN, true, LAZY, sphere_loop<real, RES, ANIM, ORD, CAMK, SCREEN>()>(A, lds_entries, prims, ro, rd, rtime, ws, state == ST_WALK, A.walk_round_steps, c_node, c_prim, dgp, lds_screen);
                if (state == ST_WALK && ws.idx >= n_entries && ws.pending < 0) state = ST_SHADE;
                const uint64_t walking = __ballot(state == ST_WALK);
                if (!walking || 64u - (uint32_t)__popcll(walking) >= A.walk_exit_lanes) break;
            }
        }
        const bool tracing = (state == ST_SHADE);

        CR_DIAG_ONLY({ unsigned long long t = __builtin_readcyclecounter(); d_t_trace += t - d_t0; d_t0 = t; })
        // ---------------- shade
        if (tracing) {
            finished = shade<real, ANIM, RES == RES_TOP, RELAX>(A, prims, mats, texs, ro, rd, rtime, rng, depth_left, stack_n, ws.best_t, ws.best,
                                         A.n_threads, gtid, c_tex, col, dgp, &thr, CR_SHADE_DD ? &ws.dd : nullptr);
            state = ST_TRACE;   // scattered: a fresh ray to walk (overwritten below when the path finished)
        }

        // ---------------- sample / pixel completion (average_samples, ray_casting.rs:154-173)
        if (RELAX && finished) {
            if constexpr (RELAX) {
                // round(c * 2^S) as an integer: c in [0, 1] (clamped Color), so c * 2^S + 2^52 lies in [2^52, 2^53], where
                // doubles are the integers -- one fused multiply-add rounds once, and the integer is the difference of
                // the bit patterns.  A colour that is not a number sets the pixel's NaN flag instead.
                const bool black = col.x == real(0) && col.y == real(0) && col.z == real(0);   // adds nothing (depth ran out, scatter None)
                if (!black) {
                    uint32_t ri = pix_i, rj = pix_j;   // the pixel among the launch's tiles (REGION: without the region's offset)
                    if constexpr (REGION) { ri -= RG.reg_x0; rj -= RG.reg_y0; }
                    const uint32_t tile = (rj >> A.sg_lh) * A.tiles_x + (ri >> A.sg_lw);
                    const uint32_t px = ((rj & ((1u << A.sg_lh) - 1u)) << A.sg_lw) | (ri & ((1u << A.sg_lw) - 1u));
                    const real cc[3] = {col.x, col.y, col.z};
                    unsigned long long v[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const double x = (double)cc[c];
                        v[c] = (x == x) ? (unsigned long long)(__builtin_bit_cast(long long, __builtin_fma(x, A.fx_scale, 0x1.0p52)) - 0x4330000000000000ll) : kFxNaN;
                    }
                    const bool nan = (v[0] | v[1] | v[2]) >> 63;
                    unsigned long long* dst;
                    bool in_lds = true;
                    if (tile == fx_tile0) dst = fx_slots + px * 3u;
                    else if (tile == fx_tile1) dst = fx_slots + fx_words + px * 3u;
                    else {
                        uint32_t row = rj;   // fx_acc's row
                        if constexpr (BATCH) row -= batch_frame(A, rj) * ((A.tiles_y << A.sg_lh) - (REGION ? RG.reg_h : (uint32_t)cam.H));
                        if constexpr (REGION) dst = A.fx_acc + ((size_t)row * (size_t)RG.reg_w + ri) * 3;
                        else dst = A.fx_acc + ((size_t)row * (size_t)cam.W + ri) * 3;
                        in_lds = false;
                    }
                    if (!nan) {
                        if (in_lds) {
                            auto d = (__attribute__((address_space(3))) unsigned long long*)dst;   // ds_add_u64, not a flat atomic
                            for (int c = 0; c < 3; c++) if (v[c]) (void)__hip_atomic_fetch_add(d + c, v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else {
                            auto d = (__attribute__((address_space(1))) unsigned long long*)dst;
                            for (int c = 0; c < 3; c++) if (v[c]) (void)__hip_atomic_fetch_add(d + c, v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    } else {
                        for (int c = 0; c < 3; c++) {
                            if (v[c] >> 63) atomicOr(dst + c, kFxNaN);
                            else if (v[c]) atomicAdd(dst + c, v[c]);
                        }
                    }
                }
            }
            state = ST_NEED_PIXEL;
        } else if (finished && A.sg_on) {   // the ordered sum happens in sg_finalize_kernel
            real* o = A.sample_buf + (size_t)item * 3;
            o[0] = col.x; o[1] = col.y; o[2] = col.z;
            state = ST_NEED_PIXEL;
        } else if (finished) {
            acc_r += col.x; acc_g += col.y; acc_b += col.z;
            sample++;
            if (sample >= A.sample_end) {
                size_t o = ((size_t)pix_j * (size_t)cam.W + pix_i) * 3;
                if (A.output_sum) { A.out[o] = acc_r; A.out[o + 1] = acc_g; A.out[o + 2] = acc_b; }
                else {
                    real cnt = (real)A.samples_total;
                    A.out[o] = acc_r / cnt; A.out[o + 1] = acc_g / cnt; A.out[o + 2] = acc_b / cnt;
                }
                state = ST_NEED_PIXEL;
            } else state = ST_NEED_SAMPLE;
        }
        CR_DIAG_ONLY({ unsigned long long t = __builtin_readcyclecounter(); d_t_shade += t - d_t0; d_t0 = t; })
    }

    if constexpr (RELAX) { fx_flush(0, fx_tile0); fx_flush(1, fx_tile1); }
    // flush work counters: one atomic per counter per wave
    if constexpr (COUNT) {
        CR_DIAG_ONLY(
            {
                unsigned long long* c = (unsigned long long*)A.counters;
                for (int i = 0; i < DG_N; i++) { unsigned long long w = WaveSum{}(dg_store.v[i]); if (lane == 0) atomicAdd(&c[16 + i], w); }
                if (lane == 0) {
                    atomicAdd(&c[9], d_t_regen); atomicAdd(&c[10], d_t_trace); atomicAdd(&c[11], d_t_shade);
                    atomicAdd(&c[12], __builtin_readcyclecounter() - d_begin);
                }
            })
#ifdef CR_HOLD_VCC
        asm volatile("" :: "{vcc}"(vcc_hold));
#endif
        flush_counters(WaveSum{}, A.counters, lane, c_seg, c_node, c_prim, c_tex);
    }
}
template <typename real, int RES, bool ANIM, bool ORD = false, bool CAMK = false, bool RELAX = false, bool SCREEN = false>
__global__ void __launch_bounds__(MaxBlock<real>::value) pathtrace_kernel(const KernelArgs<real> A) {
    // the LDS-resident f32 kernels have registers to spare and lose 1 % to the reloads: they keep the by-value parameter
    if constexpr (std::is_same<real, double>::value || RES != RES_LDS) pathtrace_body<real, RES, ANIM, ORD, CAMK, RELAX, SCREEN>(kernel_args<real>());
    else pathtrace_body<real, RES, ANIM, ORD, CAMK, RELAX, SCREEN>(A);
}

// The headline's kernel once more -- pathtrace_kernel<double, RES_LDS, false, false, false, true, true>: static f64, relaxed
// sums, screening records of an unordered tree, the whole scene in LDS -- without the work counters: the same paths and the same
// frame, for renders whose caller asked for no stats (render.hpp launch()).  No counter registers, and a vector instruction
// of the screened box step fewer.  A name of its own, so that a profile tells the two apart.  RES_LDS alone:
// the RES_TOP twin measured 0.3 % slower than the counted kernel on 1M spheres, so those scenes keep counting.
template <int RES>
__global__ void __launch_bounds__(MaxBlock<double>::value) pathtrace_kernel_quiet(const KernelArgs<double> A) {
    static_assert(RES == RES_LDS, "the counter-free kernel exists for scenes staged whole in LDS");
    pathtrace_body<double, RES, false, false, false, true, true, true, false, false>(kernel_args<double>());
}

// The relaxed kernels with keys once more, with the active-tile list in their work decode: the passes of cr_render_adaptive_*
// (adaptive.hip).  Kernels of their own, so that the ones movies and regions run on do not pay for the list.
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK, bool SCREEN>
__global__ void __launch_bounds__(MaxBlock<real>::value) pathtrace_kernel_listed(const KernelArgs<real> A) {
    static_assert(ANIM != CAMK, "keyed primitives or camera keys alone, as for pathtrace_kernel");
    if constexpr (std::is_same<real, double>::value || RES != RES_LDS) pathtrace_body<real, RES, ANIM, ORD, CAMK, true, SCREEN, true, true>(kernel_args<real>());
    else pathtrace_body<real, RES, ANIM, ORD, CAMK, true, SCREEN, true, true>(A);
}

// cr_render_views_* (DESIGN.md 6.18): the keyed RELAX kernel whose frames are views, each with its camera record in
// KernelArgs::views.  Kernels of their own (render_views_f32.hip, render_views_f64.hip), for the reason the listed ones are.
template <typename real, int RES, bool ANIM, bool ORD, bool CAMK, bool SCREEN = false>
__global__ void __launch_bounds__(MaxBlock<real>::value) pathtrace_kernel_views(const KernelArgs<real> A) {
    static_assert(ANIM != CAMK, "keyed primitives or camera keys alone, as for pathtrace_kernel");
    if constexpr (std::is_same<real, double>::value || RES != RES_LDS) pathtrace_body<real, RES, ANIM, ORD, CAMK, true, SCREEN, true, false, true, true>(kernel_args<real>());
    else pathtrace_body<real, RES, ANIM, ORD, CAMK, true, SCREEN, true, false, true, true>(A);
}

// The same kernel compiled for 6 waves per SIMD (<= 80 VGPRs, 512-thread groups), for trees far larger than the
// LDS window: there the walk waits on L2 / HBM reads and more resident waves hide more of that latency than the
// extra spills cost (1M spheres +11 %; the LDS-resident book1 and the 8K-wrapper teapot lose 3 % and stay on
// pathtrace_kernel).  RES_TOP only.
constexpr int LatencyBlock = 512;
template <typename real, bool ANIM, bool ORD = false, bool CAMK = false, bool RELAX = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, LatencyBlock), amdgpu_waves_per_eu(6, 6)))
pathtrace_kernel_latency(const KernelArgs<real> A) {
    pathtrace_body<real, RES_TOP, ANIM, ORD, CAMK, RELAX, false, false>(A);
}

// One plane of a screening record (screen.hpp's kernels make the records): the f64 plane rounded to the nearest f32 (the
// band of walk_round allows for either direction).  A finite f64 plane beyond the f32 range becomes an infinite f32 plane,
// an error TH does not cover (an f32 box that reaches to infinity decides hits that Aabb::hit misses): such a plane sets
// *overflow, and the caller then walks the tree without the screen.
CR_D void screen_plane(double b, float& f, int32_t* overflow) {
    f = (float)b;
    if (__builtin_fabsf(f) == __builtin_inff() && __builtin_fabs(b) != __builtin_inf()) *overflow = 1;
}
CR_D void screen_plane(float b, float& f, int32_t*) { f = b; }

// CR_SUM_RELAXED: the fixed-point sums become the frame -- sum * 2^-S, divided by the sample count unless the raw
// sum of the shard is asked for; a set NaN flag gives NaN (the reference would have panicked in Color::new).
template <typename real>
__global__ void __launch_bounds__(256) fx_finalize_kernel(const unsigned long long* acc, real* out, size_t n, double inv_scale, double count,
                                                          int32_t output_sum) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long v = acc[i];
    const unsigned long long m = v & ~kFxNaN;
    // exact u64 -> f64 in two halves (each below 2^53), then one rounding in the add
    double s = ((double)(uint32_t)(m >> 32) * 4294967296.0 + (double)(uint32_t)m) * inv_scale;
    if (!output_sum) s = s / count;
    if (v & kFxNaN) s = __builtin_nan("");
    out[i] = (real)s;
}

// average_samples' running sum (ray_casting.rs:161-165) for the sample-granular mode: the batch's colours are added
// to the pixel's sum in sample order, exactly the order the pixel-owning lane uses; the last batch divides by the
// sample count (`/= count`, :168-170) or hands out the raw sum.
template <typename real>
__global__ void __launch_bounds__(256) sg_finalize_kernel(const KernelArgs<real> A, real* acc, int32_t batch_samples, int32_t first_batch,
                                                          int32_t last_batch) {
    // one thread per pixel, threads numbered tile by tile (the pixels of a tile are consecutive threads), so the
    // reads of a sample group are contiguous across the tile's threads
    const uint32_t tile_px = 1u << (A.sg_lw + A.sg_lh);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t tile = (uint32_t)(t >> (A.sg_lw + A.sg_lh)), in_px = (uint32_t)t & (tile_px - 1u);
    if (tile >= A.tiles_x * A.tiles_y) return;
    uint32_t tx, ty;
    tile_xy(A, tile, tx, ty);
    const uint32_t pi = (tx << A.sg_lw) + (in_px & ((1u << A.sg_lw) - 1u));
    const uint32_t pj = (ty << A.sg_lh) + (in_px >> A.sg_lw);
    if (pi >= (uint32_t)A.cam.W || pj >= (uint32_t)A.cam.H) return;
    const size_t p = (size_t)pj * (size_t)A.cam.W + pi;
    const uint32_t ns = 64u >> (A.sg_lw + A.sg_lh);
    real r = 0, g = 0, b = 0;
    if (!first_batch) { r = acc[3 * p]; g = acc[3 * p + 1]; b = acc[3 * p + 2]; }
    for (int32_t s = 0; s < batch_samples; s++) {
        const uint32_t sg = (uint32_t)s / ns, ds = (uint32_t)s - sg * ns;
        const size_t item = ((size_t)tile * A.sg_groups + sg) * 64u + ((size_t)ds << (A.sg_lw + A.sg_lh)) + in_px;
        const real* c = A.sample_buf + item * 3;
        r += c[0]; g += c[1]; b += c[2];
    }
    if (last_batch) {
        if (A.output_sum) { A.out[3 * p] = r; A.out[3 * p + 1] = g; A.out[3 * p + 2] = b; }
        else {
            real cnt = (real)A.samples_total;
            A.out[3 * p] = r / cnt; A.out[3 * p + 1] = g / cnt; A.out[3 * p + 2] = b / cnt;
        }
    } else { acc[3 * p] = r; acc[3 * p + 1] = g; acc[3 * p + 2] = b; }
}

#endif   // __HIPCC__

}   // namespace cr
