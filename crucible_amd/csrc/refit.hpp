// BVH refit for keyframed primitives -- SURVEY 8(f) rows 1-2, opt-in through CrRenderParams.refit_boxes.
//
// The reference computes a wrapper's box once, from the primitives' construction-time boxes
// (src/objects/bvhwrapper.rs:47-50), and never again: Hittables::update_bb reaches only leaf primitives and its
// result is not read (objects/mod.rs:141, bvhwrapper.rs:102-106 carry the author's TODO).  A primitive that a
// keyframe moves out of its construction-time box is therefore clipped.  With refit_boxes = 0 this library keeps
// those stale boxes (that is the reference's image); with refit_boxes = 1 every wrapper box is re-derived for the
// frame before the render, from the same primitives and the same timeline arithmetic:
//
//   box of a primitive over the frame's ray-time interval [ta, tb] = union of its box at ta, at tb, at every key
//   end t1 inside (ta, tb), and at every key start t0 inside (ta, tb] taken twice -- with the key active (the
//   value from t0 on) and with keys starting exactly at t0 still inactive (the value just before t0).  A keyed
//   channel is piecewise linear in t with jumps only at key starts (timeline/mod.rs:233-263), so these times
//   carry its extremes.  The box at one time is Sphere::new's / Triangle::new's (sphere.rs:29-30,
//   triangle.rs:28-35) on the evaluated position; wrapper box = tight_enclose of its children (bvh.rs:67-73).
//
// A triangle with ScaleX / ScaleY / ScaleZ keys moves along v(t) * x(t) (+ y(t)): a product of two piecewise-linear
// functions, whose extremes need not sit at those times.  For such a primitive the translate part and the scale
// part (the winning scale key and its value) are sampled at those times INDEPENDENTLY and every combination is
// united: between two consecutive sample times both parts are linear, so the vertex is a bilinear function of
// (translate time, scale time) there and its coordinates are bounded by the four corner combinations, all of which
// are among the pairs.
//
// Those arguments hold for the exact values.  The computed ones are rounded sums of rounded products, which can stray past
// the values at the sample times by a few units in the last place of the largest magnitude met -- keys of opposite signs
// on one channel, a centre moving while the radius shrinks.  Every face of a keyed primitive's box therefore moves out by
// timeline_pad, a bound on twice that error.  And the value at a sample time is its right limit: a zero-length LERP key
// evaluated at its own instant gives 0/0, but just after it the key is complete.  Conservative (a superset), never too small.
//
// On a scene without primitive keys this reproduces the construction-time boxes exactly.  A refit never changes the
// topology.  (The test suite's CPU checker applies the same rule to its own tree.)
//
// refit_boxes = CR_REFIT_REBUILD builds another tree for the frame instead, over the primitives' boxes of
// this rule (prim_box_over; motion_boxes_kernel below computes them for the device builder), and fills its wrapper boxes
// with the same kernels: build.hip, build_frame_scene.
#pragma once
#include "pack.hpp"
#include "records.hpp"

namespace cr {

// combine_and_compute (timeline/mod.rs:233-263) with a switch for the one-sided limits at t: before_start = true treats a
// key whose t0 equals t as not yet active (the left limit at a key start); false counts a key whose t1 equals t as complete
// (the right limit: s = 1, which only a zero-length key does not already reach at t1, where it gives 0/0).
template <typename real>
CR_HD void timeline_eval_side(const Key<real>* keys, int n, real t, bool before_start, real& x, real& y, real& z, real& w,
                              int32_t* skind = nullptr) {
    x = real(0) + x; y = real(0) + y; z = real(0) + z;
    int32_t sk = -1;
    for (int i = 0; i < n; i++) {
        Key<real> k = keys[i];
        bool started = before_start ? (k.t0 < t) : (k.t0 <= t);
        bool active = (t > k.t1) || (started && t <= k.t1);
        if (!active) continue;
        real s = (!before_start && t >= k.t1) ? real(1) : clamp01((t - k.t0) / (k.t1 - k.t0));
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

// How far every face of a keyed primitive's box moves out (header comment): B * (4 n + 32) * 2^-p for n keys and precision p,
// B a bound on every magnitude the evaluation meets -- G the largest initial coordinate (and radius), T the sum of the
// translate keys' |a|, V the largest scale value (1, or a scale key's |a| or |b|): B = G + T + V for a sphere (c +- r), and
// (V + 1) (G + T) for a triangle (v x + y).  Each channel is n rounded additions of rounded a * s terms; the bound covers
// twice that error with room to spare.  Not a number (a key that is not): +inf, the box becomes unbounded.  Zero when no key
// moves anything (every key NERP, a LERP translate by 0 or a LERP scale from a value to itself): the computed values are
// then constant between key starts, and the samples take each of them exactly.
template <typename real> CR_HD real timeline_pad(const Prim<real>& p, const Key<real>* keys) {
    const Key<real>* k = keys + p.key_first;
    real g = real(0), tr = real(0), v = real(1);
    bool moving = false;
    const int ng = p.kind() == 0 ? 4 : 9;
    for (int i = 0; i < ng; i++) g = r_fmax(g, r_abs(p.g[i]));
    for (int i = 0; i < p.key_count; i++) {
        if (k[i].channel <= 2) tr = tr + r_abs(k[i].a);
        else v = r_fmax(v, r_fmax(r_abs(k[i].a), r_abs(k[i].b)));
        moving |= k[i].interp && (k[i].channel <= 2 ? k[i].a != real(0) : k[i].a != k[i].b);
    }
    if (!moving) return real(0);
    const real b = p.kind() == 0 ? (g + tr) + v : (v + real(1)) * (g + tr);
    const real eps = sizeof(real) == 8 ? real(0x1.0p-53) : real(0x1.0p-24);
    const real pad = b * ((real)(4 * p.key_count + 32) * eps);
    return pad == pad ? pad : r_inf(real(0));
}

// A sample box with a coordinate that is not a number is not united (a zero-length LERP key evaluated exactly at its
// own start gives 0/0): the rule would otherwise depend on the order of its unions.  Ray times are drawn from a
// continuum, so the instant itself carries no rays.  That holds for sample boxes only: the construction-time box (use_keys =
// false) is taken as it is -- in f32 a sphere whose centre and radius are both infinite has a plane inf - inf, and a fresh
// build keeps it (tree.hpp prim_box), so cr_update_primitives and the device builders keep it too.
template <typename real> CR_HD bool box_is_number(const real blo[3], const real bhi[3]) {
    return blo[0] == blo[0] && blo[1] == blo[1] && blo[2] == blo[2] && bhi[0] == bhi[0] && bhi[1] == bhi[1] && bhi[2] == bhi[2];
}
template <typename real> CR_HD void enclose(real lo[3], real hi[3], const real blo[3], const real bhi[3]) {
    for (int a = 0; a < 3; a++) {   // Interval::tight_enclose, utils.rs:629-633
        lo[a] = lo[a] <= blo[a] ? lo[a] : blo[a];
        hi[a] = hi[a] >= bhi[a] ? hi[a] : bhi[a];
    }
}

// Box of primitive p with its translate part taken at time t and its scale part at time ts, united into lo/hi
// (ts = t, bs = before_start: the box at one time), its faces moved out by pad.  use_keys = false: the construction-time
// box (no keys applied; pad 0 leaves it exact).
template <typename real>
CR_HD void prim_box_at2(const Prim<real>& p, const Key<real>* keys, real t, bool before_start, real ts, bool bs, real lo[3], real hi[3],
                        bool use_keys = true, real pad = real(0)) {
    real blo[3], bhi[3];
    const Key<real>* k = keys + p.key_first;
    const int32_t n_keys = use_keys ? p.key_count : 0;
    real v[3][3];
    for (int j = 0; j < 3; j++) {
        real w = real(1), w2 = real(1), ux = p.g[3 * j], uy = p.g[3 * j + 1], uz = p.g[3 * j + 2];
        int32_t sk;
        v[j][0] = ux; v[j][1] = uy; v[j][2] = uz;
        timeline_eval_side(k, n_keys, t, before_start, v[j][0], v[j][1], v[j][2], w);
        timeline_eval_side(k, n_keys, ts, bs, ux, uy, uz, w2, &sk);
        const V3<real> q = scale_point(sk, w2, v[j][0], v[j][1], v[j][2]);
        v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z;
    }
    for (int a = 0; a < 3; a++) {
        bhi[a] = r_fmax(v[0][a], r_fmax(v[1][a], v[2][a])) + pad;
        blo[a] = r_fmin(v[0][a], r_fmin(v[1][a], v[2][a])) - pad;
    }
    if (!use_keys || box_is_number(blo, bhi)) enclose(lo, hi, blo, bhi);
}

template <typename real>
CR_HD void prim_box_at(const Prim<real>& p, const Key<real>* keys, real t, bool before_start, real lo[3], real hi[3], bool use_keys = true,
                       real pad = real(0)) {
    if (p.kind() != 0) { prim_box_at2(p, keys, t, before_start, t, before_start, lo, hi, use_keys, pad); return; }
    real blo[3], bhi[3];
    const Key<real>* k = keys + p.key_first;
    const int32_t n_keys = use_keys ? p.key_count : 0;
    {   // Sphere::new, sphere.rs:29-30; Aabb::new_from_points, bvh.rs:44-64
        real c[3] = {p.g[0], p.g[1], p.g[2]}, r = p.g[3];
        timeline_eval_side(k, n_keys, t, before_start, c[0], c[1], c[2], r);
        for (int a = 0; a < 3; a++) {
            real l = c[a] + (-r), h = c[a] + r;
            if (l <= h) { blo[a] = l - pad; bhi[a] = h + pad; } else { blo[a] = h - pad; bhi[a] = l + pad; }
        }
    }
    if (!use_keys || box_is_number(blo, bhi)) enclose(lo, hi, blo, bhi);
}

// The sample times of the refit rule, indexed: 0 = ta, 1 = tb, then three per key (its start with the key active,
// its start with the key not yet active, its end).  false: that sample is not part of the rule.
template <typename real>
CR_HD bool refit_sample(const Prim<real>& p, const Key<real>* keys, real ta, real tb, int32_t i, real& t, bool& before_start) {
    before_start = false;
    if (i == 0) { t = ta; return true; }
    if (i == 1) { t = tb; return true; }
    const Key<real> k = keys[p.key_first + (i - 2) / 3];
    const int32_t which = (i - 2) % 3;
    if (which < 2) { t = k.t0; before_start = which == 1; return ta < k.t0 && k.t0 <= tb; }
    t = k.t1;
    return ta < k.t1 && k.t1 < tb;
}

// Box of primitive p over ray times [ta, tb], united into lo/hi (rule in the header comment).  use_keys = false, or no
// keys: the construction-time box, exactly.  Every sample box is grown by timeline_pad before it is united (the same
// bits as growing the union: rounding is monotone).
template <typename real>
CR_HD void prim_box_over(const Prim<real>& p, const Key<real>* keys, real ta, real tb, real lo[3], real hi[3], bool use_keys = true) {
    if (!use_keys || p.key_count == 0) { prim_box_at(p, keys, ta, false, lo, hi, use_keys); return; }
    const real pad = timeline_pad(p, keys);
    prim_box_at(p, keys, ta, false, lo, hi, true, pad);
    bool scaled = false;   // ScaleX / ScaleY / ScaleZ keys: translate and scale parts sampled independently
    for (int i = 0; i < p.key_count; i++) scaled |= keys[p.key_first + i].channel >= 4;
    if (scaled) {
        const int32_t n = 2 + 3 * p.key_count;
        for (int32_t i = 0; i < n; i++) {
            real t1; bool b1;
            if (!refit_sample(p, keys, ta, tb, i, t1, b1)) continue;
            for (int32_t j = 0; j < n; j++) {
                real t2; bool b2;
                if (refit_sample(p, keys, ta, tb, j, t2, b2)) prim_box_at2(p, keys, t1, b1, t2, b2, lo, hi, true, pad);
            }
        }
        return;
    }
    prim_box_at(p, keys, tb, false, lo, hi, true, pad);
    for (int i = 0; i < p.key_count; i++) {
        const Key<real> k = keys[p.key_first + i];
        if (ta < k.t0 && k.t0 <= tb) {
            prim_box_at(p, keys, k.t0, false, lo, hi, true, pad);
            prim_box_at(p, keys, k.t0, true, lo, hi, true, pad);
        }
        if (ta < k.t1 && k.t1 < tb) prim_box_at(p, keys, k.t1, false, lo, hi, true, pad);
    }
}

// The same rule on the host, from the caller's description of the scene: the boxes of n primitives over [ta, tb] -- desc[j]
// names the j-th in `prims`, desc = nullptr takes the first n in order -- as the SAH builders read them (bmin / bmax: [3]).
// What build_frame_scene hands the host builder; motion_boxes_kernel below writes the same bits for the device builder.
template <typename real>
void motion_boxes(const std::vector<CrPrimitive>& prims, const int32_t* desc, int32_t n, const std::vector<CrKeyframe>& scene_keys, real ta, real tb,
                  std::vector<real>* bmin, std::vector<real>* bmax) {
    std::vector<Key<real>> keys(scene_keys.size() + 1);
    memset(keys.data(), 0, keys.size() * sizeof(Key<real>));
    for (size_t i = 0; i < scene_keys.size(); i++) key_to_real(scene_keys[i], keys[i]);
    for (int a = 0; a < 3; a++) { bmin[a].resize(n); bmax[a].resize(n); }
    for (int32_t j = 0; j < n; j++) {
        const Prim<real> q = pack_prim<real>(prims[(size_t)(desc ? desc[j] : j)]);
        real lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
        prim_box_over(q, keys.data(), ta, tb, lo, hi, true);
        for (int a = 0; a < 3; a++) { bmin[a][j] = lo[a]; bmax[a][j] = hi[a]; }
    }
}

#if defined(__HIPCC__)
// One level of the tree, deepest level first (entries are stored level by level, children after parents):
// leaves take their primitives' boxes, inner wrappers the union of their two children, already refitted.
// use_keys = 0 gives the construction-time boxes (how the LBVH builder fills in its boxes).
template <typename real, bool ORD>
__global__ void refit_level_kernel(typename EntryOf<real, ORD>::type* entries, int32_t begin, int32_t end, const Prim<real>* prims,
                                   const Key<real>* keys, real ta, real tb, int32_t use_keys, const int32_t* leaf_runs) {
    const int32_t i = begin + (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= end) return;
    const int32_t leaf = entries[i].leaf;
    real lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
    if (leaf >= 0) {
        int32_t first = leaf >> 1, count = (leaf & 1) + 1;
        if (leaf & kLeafRun) { first = leaf_runs[2 * (leaf & kLeafRunIndex)]; count = leaf_runs[2 * (leaf & kLeafRunIndex) + 1]; }
        if ((leaf & kLeafRun) && (leaf & kLeafPseudo)) count = 0;   // tested without a box in the reference: the box stays empty
        for (int32_t k = 0; k < count; k++) prim_box_over(prims[first + k], keys, ta, tb, lo, hi, use_keys != 0);
    } else {
        const int32_t li = ORD ? ordered_left(leaf) : -leaf;   // siblings are adjacent in the level-order array
        for (int32_t c = li; c <= li + 1; c++) {
            const int32_t cl = entries[c].leaf;
            if (cl >= 0 && (cl & kLeafRun) && (cl & kLeafPseudo)) {
                // a primitive / list beside a BVHWrapper element: its own record keeps the empty box (the reference tests it
                // without one), but the wrapper above it spans it
                const int32_t first = leaf_runs[2 * (cl & kLeafRunIndex)], count = leaf_runs[2 * (cl & kLeafRunIndex) + 1];
                real clo[3], chi[3];
                for (int a = 0; a < 3; a++) { clo[a] = r_inf(real(0)); chi[a] = -r_inf(real(0)); }
                for (int32_t k = 0; k < count; k++) prim_box_over(prims[first + k], keys, ta, tb, clo, chi, use_keys != 0);
                enclose(lo, hi, clo, chi);
                continue;
            }
            const real* cb = entries[c].b;
            const real clo[3] = {cb[0], cb[2], cb[4]}, chi[3] = {cb[1], cb[3], cb[5]};
            enclose(lo, hi, clo, chi);
        }
    }
    real* b = entries[i].b;
    b[0] = lo[0]; b[1] = hi[0]; b[2] = lo[1]; b[3] = hi[1]; b[4] = lo[2]; b[5] = hi[2];
}

// CR_REFIT_REBUILD: the input of the device SAH builder for one frame.  One thread per record of the base
// tree's `prims` (leaf order, read coalesced); its box over the ray times [ta, tb] -- prim_box_over in `real`, the bits a
// refit gives a one-primitive leaf -- goes, widened to f64 (exact), to the position the builders see that primitive at:
// input_of[i], six doubles lo xyz, hi xyz as build_sah_device takes them.  The keyed loop's trip count is per primitive (a
// scaled triangle: quadratic in its keys), so a wave runs as long as its longest timeline; records are not regrouped by key
// count -- the pass runs once per frame build and unkeyed primitives leave after one box.
template <typename real>
__global__ void motion_boxes_kernel(const Prim<real>* prims, const int32_t* input_of, int32_t n, const Key<real>* keys, real ta, real tb, double* box6) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int32_t j = input_of[i];
    if (j < 0 || j >= n) return;   // (a permutation of 0 .. n-1: never taken)
    real lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
    prim_box_over(prims[i], keys, ta, tb, lo, hi, true);
    double* o = box6 + (size_t)j * 6;
    for (int a = 0; a < 3; a++) { o[a] = (double)lo[a]; o[3 + a] = (double)hi[a]; }
}

// The frame tree's primitive records in its own leaf order, gathered from the base tree's: out[i] = base[src[i]].
template <typename real>
__global__ void gather_prims_kernel(const Prim<real>* base, const int32_t* src, int32_t n, Prim<real>* out) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int32_t s = src[i];
    if (s < 0 || s >= n) return;
    out[i] = base[s];
}
#endif

}   // namespace cr
