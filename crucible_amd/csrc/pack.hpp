// Host-side packing of the C-ABI descriptors (include/crucible_hip.h) into the device records of records.hpp: primitives,
// materials, textures, keyframes, images and the camera constants.  build.hip, scene.hip and render.hip upload what these functions make, and
// tests/shade_check.hip packs its inputs with the same functions, so the device checks see the library's own records
// (Schlick's r0, 1/scatter_prob, 1/radius, the texel words) rather than a copy of the packing.
#pragma once
#include "../../include/crucible_hip.h"
#include "records.hpp"
#include "scene_checks.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cr {

template <typename real> void key_to_real(const CrKeyframe& k, Key<real>& o) {
    o.t0 = (real)k.t0; o.t1 = (real)k.t1; o.a = (real)k.a; o.b = (real)k.b; o.channel = k.channel; o.interp = k.interp;
}

template <typename real> Prim<real> pack_prim(const CrPrimitive& p) {
    Prim<real> q;
    memset(&q, 0, sizeof q);
    for (int k = 0; k < 9; k++) q.g[k] = (real)p.v[k];
    if (p.kind == CR_PRIM_SPHERE) q.g[4] = real(1) / q.g[3];    // 1/radius, used for the hit normal of static spheres
    q.kind_mat = (p.kind & 1) | (p.material << 1);
    q.key_first = p.key_first; q.key_count = p.key_count;
    return q;
}

// live_texture_remap, the device texture table's re-indexing, reads descriptors alone: scene_checks.hpp

template <typename real> Mat<real> pack_mat(const CrMaterial& m, const CrTexture* textures, const int32_t* tex_remap) {
    Mat<real> o;
    memset(&o, 0, sizeof o);
    o.kind = m.kind; o.param = (real)m.param; o.tex = -1;
    for (int k = 0; k < 3; k++) o.albedo[k] = (real)m.albedo[k];
    if (m.kind == CR_MAT_LAMBERTIAN) {
        const CrTexture& t = textures[m.texture];
        if (t.kind == CR_TEX_SOLID) for (int k = 0; k < 3; k++) o.albedo[k] = (real)t.color[k];
        else o.tex = tex_remap[m.texture];
        o.aux = real(1) / r_abs(o.param);                       // Color / f64: (1.0 / rhs.abs()) * c
    } else if (m.kind == CR_MAT_DIELECTRIC) {
        auto r0 = [](real ri) { real q = (real(1) - ri) / (real(1) + ri); return q * q; };   // dielectric.rs:21-23
        o.albedo[0] = real(1) / o.param;                        // ri for a front-face hit (dielectric.rs:33-37)
        o.albedo[1] = r0(o.albedo[0]);
        o.albedo[2] = r0(o.param);
    }
    return o;
}

template <typename real> Tex<real> pack_tex(const CrTexture& t, const int32_t* tex_remap) {
    Tex<real> o;
    memset(&o, 0, sizeof o);
    o.kind = t.kind; o.image = t.image; o.inv_scale = (real)t.inv_scale;
    o.even = t.kind == CR_TEX_CHECKER ? tex_remap[t.even] : -1;
    o.odd = t.kind == CR_TEX_CHECKER ? tex_remap[t.odd] : -1;
    for (int k = 0; k < 3; k++) o.color[k] = (real)t.color[k];
    return o;
}

// The device's material and texture tables of a description: what build_dev_scene uploads and cr_update_materials repacks
template <typename real>
void pack_side_tables(const std::vector<CrMaterial>& materials, const std::vector<CrTexture>& textures, std::vector<Mat<real>>& mats, std::vector<Tex<real>>& texs) {
    const std::vector<int32_t> tex_remap = live_texture_remap(materials.data(), materials.size(), textures.data(), textures.size());
    mats.resize(materials.size());
    for (size_t i = 0; i < mats.size(); i++) mats[i] = pack_mat<real>(materials[i], textures.data(), tex_remap.data());
    texs.clear();
    for (size_t i = 0; i < textures.size(); i++)
        if (tex_remap[i] >= 0) texs.push_back(pack_tex<real>(textures[i], tex_remap.data()));
}

// Images: RGB8 -> RGBA8 words, one flat texel array.  false when the texels do not fit 32-bit offsets.
inline bool pack_images(const CrImage* images, int32_t n_images, std::vector<ImageRef>& refs, std::vector<uint32_t>& texels) {
    refs.resize((size_t)n_images);
    size_t total = 0;
    for (int i = 0; i < n_images; i++) {
        refs[i].w = images[i].width; refs[i].h = images[i].height; refs[i].offset = (uint32_t)total; refs[i].pad = 0;
        total += (size_t)images[i].width * images[i].height;
    }
    if (total >= ((size_t)1 << 32)) return false;
    texels.assign(total ? total : 1, 0u);
    for (int i = 0; i < n_images; i++) {
        const uint8_t* src = images[i].rgb8;
        size_t n = (size_t)refs[i].w * refs[i].h;
        uint32_t* dst = texels.data() + refs[i].offset;
        for (size_t k = 0; k < n; k++) dst[k] = (uint32_t)src[3 * k] | ((uint32_t)src[3 * k + 1] << 8) | ((uint32_t)src[3 * k + 2] << 16);
    }
    return true;
}

// The camera constants of a render: Radians::new_from_degrees (utils.rs:51-55), fix_viewport (rendering_compute.rs:5-11)
// and defocus_radius (:71-73) in f64, rounded once; the camera's keys go first the look_from keys, then the look_at keys.
template <typename real> void pack_camera(const CrCameraDesc* cd, CamConst<real>& c) {
    const double PI64 = 3.14159265358979323846264338327950288;
    c.W = cd->image_width; c.H = cd->image_height;
    double vfov = cd->vfov_degrees * PI64 / 180.0;
    double hh = std::tan(vfov / 2.0);
    double vh = 2.0 * hh * cd->focus_dist;
    double vw = vh * ((double)cd->image_width / (double)cd->image_height);
    double da = cd->defocus_angle_degrees * PI64 / 180.0;
    c.viewport_height = (real)vh; c.viewport_width = (real)vw; c.focus_dist = (real)cd->focus_dist;
    c.defocus_on = !(da <= 0.0);
    c.defocus_radius = (real)(cd->focus_dist * std::tan(da / 2.0));
    c.from = mk<real>((real)cd->look_from[0], (real)cd->look_from[1], (real)cd->look_from[2]);
    c.at = mk<real>((real)cd->look_at[0], (real)cd->look_at[1], (real)cd->look_at[2]);
    c.vup = mk<real>((real)cd->vup[0], (real)cd->vup[1], (real)cd->vup[2]);
    int nk = cd->from_key_count + cd->at_key_count;
    c.animated = nk > 0;
    c.from_key_first = 0; c.from_key_count = cd->from_key_count;
    c.at_key_first = cd->from_key_count; c.at_key_count = cd->at_key_count;
}

// The static camera's per-sample vectors: the same expression tree the kernel would evaluate per sample.
template <typename real> void pack_camera_frame(CamConst<real>& c) {
    V3<real> from = mk<real>(real(0) + c.from.x, real(0) + c.from.y, real(0) + c.from.z);
    V3<real> at = mk<real>(real(0) + c.at.x, real(0) + c.at.y, real(0) + c.at.z);
    from = scale(real(1), from); at = scale(real(1), at);   // build_other_scaler(1.0): s*x
    CamFrame<real> f = camera_frame(c, from, at);
    if (!c.animated) c.from = f.from;
    c.p00 = f.p00; c.pdu = f.pdu; c.pdv = f.pdv; c.ddu = f.ddu; c.ddv = f.ddv;
}

// cr_render_views_*: the records of n cameras that share one key table -- view k's look_from keys, then its look_at keys,
// behind those of the views before it, so its *_key_first count from the table's start.  Each record is otherwise what
// pack_camera and pack_camera_frame make of the camera alone.  Returns the keys of all views together.
template <typename real> int64_t pack_views(const CrCameraDesc* cams, int32_t n, CamConst<real>* table) {
    int64_t first = 0;
    for (int32_t k = 0; k < n; k++) {
        CamConst<real>& c = table[k];
        pack_camera(&cams[k], c);
        // (a table longer than the key slot is refused by the caller: the offsets only need to stay defined up to there)
        c.from_key_first = (int32_t)std::min<int64_t>(first, INT32_MAX);
        c.at_key_first = (int32_t)std::min<int64_t>(first + cams[k].from_key_count, INT32_MAX);
        first += (int64_t)cams[k].from_key_count + cams[k].at_key_count;
        pack_camera_frame(c);
    }
    return first;
}
// ... and the table itself: dst receives the keys in that order
template <typename real> void pack_view_keys(const CrCameraDesc* cams, int32_t n, Key<real>* dst) {
    for (int32_t k = 0; k < n; k++) {
        for (int i = 0; i < cams[k].from_key_count; i++) key_to_real(cams[k].from_keys[i], *dst++);
        for (int i = 0; i < cams[k].at_key_count; i++) key_to_real(cams[k].at_keys[i], *dst++);
    }
}

// The frame's ray times [current_time, current_time + shutter_length] in `real` (ray_casting.rs:77-79).
template <typename real> void frame_times(const CrRenderParams* p, real& current_time, real& shutter_length) {
    current_time = (real)p->frame * (real(1) / (real)p->frame_rate);
    shutter_length = ((real)p->shutter_angle / real(360)) * (real(1) / (real)p->frame_rate);
}

}   // namespace cr
