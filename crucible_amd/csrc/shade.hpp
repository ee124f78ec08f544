// shade.hpp -- device only: what happens at a hit and where a path begins.  Image look-up, the software
// atan2 / asin / acos, the device samplers, camera rays, the record loads, the checker texture, and shade (Materials::scatter
// and the sky).  The reference citations are pathtrace.hpp's.
#pragma once
#include "intersect.hpp"

#if defined(__HIPCC__)

namespace cr {

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

}   // namespace cr

#endif   // __HIPCC__
