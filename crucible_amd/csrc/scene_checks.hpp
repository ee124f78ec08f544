// scene_checks.hpp -- the checks on a scene description that read descriptor arrays alone and answer a code and a message:
// textures, materials, the sky, a primitive's material index.  cr_upload_scene runs them in its own order; cr_update_materials,
// cr_update_image and cr_set_sky (scene.hip) run them on the description their edit would leave, after their own
// argument checks, which are here as well; and live_texture_remap, which decides from the descriptors what the device texture
// table holds.  Free of the HIP runtime: tests/scene_checks_check.cpp compiles it with g++.
#pragma once
#include "../../include/crucible_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace cr {

struct SceneCheck {
    int32_t code;        // CR_OK, or the refusal's status
    const char* msg;     // its message; nullptr with CR_OK
    bool ok() const { return code == CR_OK; }
};
inline SceneCheck check_ok() { return SceneCheck{CR_OK, nullptr}; }
inline SceneCheck check_fail(int32_t code, const char* msg) { return SceneCheck{code, msg}; }

inline bool check_finite(double x) { return x == x && x != HUGE_VAL && x != -HUGE_VAL; }

// Every texture, then the nesting depth of the checkers
inline SceneCheck check_textures(const CrTexture* textures, int32_t n_textures, int32_t n_images) {
    for (int i = 0; i < n_textures; i++) {
        const CrTexture& t = textures[i];
        if (t.kind < CR_TEX_SOLID || t.kind > CR_TEX_IMAGE) return check_fail(CR_ERR_INVALID_ARG, "unknown texture kind");
        // children before parents keeps the texture graph acyclic (Arc<Textures> cannot cycle either)
        if (t.kind == CR_TEX_CHECKER && (t.even < 0 || t.even >= i || t.odd < 0 || t.odd >= i))
            return check_fail(CR_ERR_INVALID_ARG, "checker sub-textures must have smaller indices");
        if (t.kind == CR_TEX_IMAGE && (t.image < 0 || t.image >= n_images)) return check_fail(CR_ERR_INVALID_ARG, "texture image index out of range");
        if (t.kind == CR_TEX_SOLID) for (int k = 0; k < 3; k++) if (!(t.color[k] >= 0.0 && t.color[k] <= 1.0))
            return check_fail(CR_ERR_INVALID_ARG, "colour component outside [0,1]");   // Color::new, utils.rs:345-350
    }
    // the device resolves a checker chain iteratively with a bound of 32 levels (pathtrace.hpp, shade)
    std::vector<int32_t> depth((size_t)std::max(0, n_textures), 0);
    for (int i = 0; i < n_textures; i++) {
        const CrTexture& t = textures[i];
        if (t.kind != CR_TEX_CHECKER) continue;
        depth[i] = 1 + std::max(depth[t.even], depth[t.odd]);
        if (depth[i] > CR_MAX_CHECKER_DEPTH) return check_fail(CR_ERR_UNSUPPORTED, "checker textures nested deeper than CR_MAX_CHECKER_DEPTH (32)");
    }
    return check_ok();
}

inline SceneCheck check_materials(const CrMaterial* materials, int32_t n_materials, int32_t n_textures) {
    for (int i = 0; i < n_materials; i++) {
        const CrMaterial& m = materials[i];
        if (m.kind < CR_MAT_LAMBERTIAN || m.kind > CR_MAT_DIELECTRIC) return check_fail(CR_ERR_INVALID_ARG, "unknown material kind");
        if (m.kind == CR_MAT_LAMBERTIAN && (m.texture < 0 || m.texture >= n_textures)) return check_fail(CR_ERR_INVALID_ARG, "material texture index out of range");
        if (m.kind == CR_MAT_METAL) {
            if (!(m.param <= 1.0)) return check_fail(CR_ERR_INVALID_ARG, "A metal cannot have a fuzz factor above 1.0");   // metal.rs:21
            if (!(m.param >= 0.0)) return check_fail(CR_ERR_INVALID_ARG, "A metal cannot have a fuzz factor below 0.0");   // metal.rs:22
            for (int k = 0; k < 3; k++) if (!(m.albedo[k] >= 0.0 && m.albedo[k] <= 1.0)) return check_fail(CR_ERR_INVALID_ARG, "colour component outside [0,1]");
        }
        if (!check_finite(m.param)) return check_fail(CR_ERR_INVALID_ARG, "material parameter is not finite");
    }
    return check_ok();
}

// A sphere's or triangle's material index against the table it names
inline SceneCheck check_prim_material(int32_t material, int32_t n_materials) {
    if (material < 0 || material >= n_materials) return check_fail(CR_ERR_INVALID_ARG, "primitive material index out of range");
    return check_ok();
}

inline SceneCheck check_sky_kind(int32_t sky_kind) {
    if (sky_kind != CR_SKY_DEFAULT && sky_kind != CR_SKY_SPHERICAL) return check_fail(CR_ERR_INVALID_ARG, "unknown sky kind");
    return check_ok();
}
inline SceneCheck check_sky_image(int32_t sky_kind, int32_t sky_image, int32_t n_images) {
    if (sky_kind == CR_SKY_SPHERICAL && (sky_image < 0 || sky_image >= n_images)) return check_fail(CR_ERR_INVALID_ARG, "sky image index out of range");
    return check_ok();
}

// Device texture table: only textures a non-solid lambertian can reach (a solid top-level texture is folded into its
// material), re-indexed densely; children keep smaller indices.  Returns the new index of every texture, or -1.
inline std::vector<int32_t> live_texture_remap(const CrMaterial* materials, size_t n_materials, const CrTexture* textures, size_t n_textures) {
    std::vector<int32_t> tex_remap(n_textures, -1);
    std::vector<char> live(n_textures, 0);
    for (size_t i = 0; i < n_materials; i++) {
        const CrMaterial& m = materials[i];
        if (m.kind == CR_MAT_LAMBERTIAN && textures[m.texture].kind != CR_TEX_SOLID) live[m.texture] = 1;
    }
    for (size_t i = n_textures; i-- > 0;)   // parents have larger indices than children
        if (live[i] && textures[i].kind == CR_TEX_CHECKER) { live[textures[i].even] = 1; live[textures[i].odd] = 1; }
    int32_t next = 0;
    for (size_t i = 0; i < live.size(); i++) if (live[i]) tex_remap[i] = next++;
    return tex_remap;
}

// ---------------------------------------------------------------- cr_update_materials
// The shape of the call's arguments: what can be said before the handle's scene is looked at
inline SceneCheck check_materials_args(const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                                       const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    if (n_materials < 0 || n_textures < 0 || n_assign < 0) return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: negative count");
    // a null table says "stays as it is": a count beside it contradicts that
    if ((!materials && n_materials != 0) || (!textures && n_textures != 0))
        return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: a null table with a count that is not zero");
    if (n_assign > 0 && (!prim_index || !prim_material)) return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: null assignment arrays");
    return check_ok();
}

// The call against the uploaded description (prims; the tables that stay: kept_*): the assignment's own refusals, then the
// checks of the description the edit would leave, in cr_upload_scene's order -- textures, materials, primitives.
inline SceneCheck check_materials_update(const CrPrimitive* prims, int64_t n_prims, const CrMaterial* kept_materials, int32_t n_kept_materials,
                                         const CrTexture* kept_textures, int32_t n_kept_textures, int32_t n_images,
                                         const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                                         const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    for (int32_t k = 0; k < n_assign; k++)
        if (prim_index[k] < 0 || prim_index[k] >= n_prims) return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: primitive index out of range");
    // where assignment k lands; -1: the primitive keeps its material
    std::vector<int32_t> assigned;
    if (n_assign > 0) {
        assigned.assign((size_t)n_prims, -1);
        for (int32_t k = 0; k < n_assign; k++) {
            int32_t& slot = assigned[(size_t)prim_index[k]];
            if (slot >= 0) return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: a primitive is named twice");
            slot = k;
        }
        for (int32_t k = 0; k < n_assign; k++) {
            const CrPrimitive& p = prims[prim_index[k]];
            if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) return check_fail(CR_ERR_INVALID_ARG, "cr_update_materials: a list element has no material to assign");
        }
    }
    const CrTexture* tex = textures ? textures : kept_textures;
    const int32_t n_tex = textures ? n_textures : n_kept_textures;
    const CrMaterial* mat = materials ? materials : kept_materials;
    const int32_t n_mat = materials ? n_materials : n_kept_materials;
    if (textures) { const SceneCheck c = check_textures(tex, n_tex, n_images); if (!c.ok()) return c; }
    if (materials || textures) { const SceneCheck c = check_materials(mat, n_mat, n_tex); if (!c.ok()) return c; }
    if (materials || n_assign > 0)
        for (int64_t i = 0; i < n_prims; i++) {
            const CrPrimitive& p = prims[i];
            if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) continue;
            const int32_t m = (!assigned.empty() && assigned[(size_t)i] >= 0) ? prim_material[assigned[(size_t)i]] : p.material;
            const SceneCheck c = check_prim_material(m, n_mat);
            if (!c.ok()) return c;
        }
    return check_ok();
}

// ---------------------------------------------------------------- cr_update_image
// The rectangle (x0, y0, width, height) of image `image`, one of n_images whose sizes are image_w / image_h as uploaded
inline SceneCheck check_image_update(int32_t image, int32_t n_images, const int32_t* image_w, const int32_t* image_h,
                                     int32_t x0, int32_t y0, int32_t width, int32_t height, const void* rgb8) {
    if (!rgb8) return check_fail(CR_ERR_INVALID_ARG, "cr_update_image: null texels");
    if (width < 1 || height < 1) return check_fail(CR_ERR_INVALID_ARG, "cr_update_image: width or height below 1");
    if (image < 0 || image >= n_images) return check_fail(CR_ERR_INVALID_ARG, "cr_update_image: image index out of range");
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + (int64_t)width > (int64_t)image_w[image] || (int64_t)y0 + (int64_t)height > (int64_t)image_h[image])
        return check_fail(CR_ERR_INVALID_ARG, "cr_update_image: the rectangle leaves the image");
    return check_ok();
}

}   // namespace cr
