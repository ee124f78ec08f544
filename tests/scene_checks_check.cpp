// scene_checks_check -- crucible_amd/csrc/scene_checks.hpp under a plain C++ compiler (tests/test_scene_checks_host.py builds it
// with g++, plain and with -fsanitize=undefined,address, and holds its lines to the contract of cr_update_materials,
// cr_update_image and cr_set_sky in include/crucible_hip.h).  Takes no input.  Prints one line per case,
//   NAME|CODE|MESSAGE            a check's answer (MESSAGE empty with CR_OK)
//   NAME|remap|I0 I1 ...|N       live_texture_remap's new indices and the size of the device texture table
#include "scene_checks.hpp"

#include <climits>
#include <cstdio>
#include <vector>

using namespace cr;

static void say(const char* name, const SceneCheck& c) { printf("%s|%d|%s\n", name, c.code, c.msg ? c.msg : ""); }

static CrTexture solid(double r, double g, double b) { CrTexture t{}; t.kind = CR_TEX_SOLID; t.even = t.odd = t.image = -1; t.color[0] = r; t.color[1] = g; t.color[2] = b; return t; }
static CrTexture checker(int even, int odd) { CrTexture t{}; t.kind = CR_TEX_CHECKER; t.even = even; t.odd = odd; t.image = -1; t.inv_scale = 2.0; return t; }
static CrTexture image(int i) { CrTexture t{}; t.kind = CR_TEX_IMAGE; t.even = t.odd = -1; t.image = i; return t; }
static CrMaterial lambertian(int tex) { CrMaterial m{}; m.kind = CR_MAT_LAMBERTIAN; m.texture = tex; m.param = 1.0; return m; }
static CrMaterial metal(double fuzz, double a) { CrMaterial m{}; m.kind = CR_MAT_METAL; m.texture = -1; m.albedo[0] = m.albedo[1] = m.albedo[2] = a; m.param = fuzz; return m; }
static CrMaterial dielectric(double ri) { CrMaterial m{}; m.kind = CR_MAT_DIELECTRIC; m.texture = -1; m.param = ri; return m; }
static CrPrimitive prim(int kind, int material) { CrPrimitive p{}; p.kind = kind; p.material = material; p.v[3] = 1.0; return p; }

// a chain of `levels` checkers over two solids: texture 2 + k has children (1 + k, 0)
static std::vector<CrTexture> chain(int levels) {
    std::vector<CrTexture> t{solid(0, 0, 0), solid(1, 1, 1)};
    for (int k = 0; k < levels; k++) t.push_back(checker(1 + k, 0));
    return t;
}

static void remap(const char* name, const std::vector<CrMaterial>& m, const std::vector<CrTexture>& t) {
    const std::vector<int32_t> r = live_texture_remap(m.data(), m.size(), t.data(), t.size());
    printf("%s|remap|", name);
    int n = 0;
    for (size_t i = 0; i < r.size(); i++) { printf(i ? " %d" : "%d", r[i]); n += r[i] >= 0; }
    printf("|%d\n", n);
}

int main() {
    const double nan = std::nan("");
    // ---- textures
    { std::vector<CrTexture> t{solid(0, 0, 0)}; t[0].kind = 3; say("tex_kind", check_textures(t.data(), 1, 0)); }
    { std::vector<CrTexture> t{checker(0, 0)}; say("checker_self", check_textures(t.data(), 1, 0)); }
    { std::vector<CrTexture> t{solid(0, 0, 0), checker(0, 2), solid(1, 1, 1)}; say("checker_forward", check_textures(t.data(), 3, 0)); }
    { std::vector<CrTexture> t{image(2)}; say("tex_image", check_textures(t.data(), 1, 2)); say("tex_image_ok", check_textures((t[0] = image(1), t.data()), 1, 2)); }
    { std::vector<CrTexture> t{solid(0, 1.5, 0)}; say("tex_colour", check_textures(t.data(), 1, 0)); t[0] = solid(0, nan, 0); say("tex_colour_nan", check_textures(t.data(), 1, 0)); }
    { std::vector<CrTexture> t = chain(CR_MAX_CHECKER_DEPTH); say("depth_at_limit", check_textures(t.data(), (int32_t)t.size(), 0)); }
    { std::vector<CrTexture> t = chain(CR_MAX_CHECKER_DEPTH + 1); say("depth_over", check_textures(t.data(), (int32_t)t.size(), 0)); }
    { std::vector<CrTexture> t{solid(2, 0, 0), image(0)}; say("two_tex_faults_first_wins", check_textures(t.data(), 2, 0)); }   // the first texture's fault
    say("tex_empty", check_textures(nullptr, 0, 0));
    // ---- materials
    { CrMaterial m = lambertian(0); m.kind = 3; say("mat_kind", check_materials(&m, 1, 1)); m.kind = -1; say("mat_kind_negative", check_materials(&m, 1, 1)); }
    { CrMaterial m = lambertian(1); say("mat_texture", check_materials(&m, 1, 1)); m.texture = -1; say("mat_texture_negative", check_materials(&m, 1, 1)); m.texture = 0; say("mat_texture_ok", check_materials(&m, 1, 1)); }
    { CrMaterial m = metal(1.5, 0.5); say("fuzz_above", check_materials(&m, 1, 0)); m = metal(-0.5, 0.5); say("fuzz_below", check_materials(&m, 1, 0)); m = metal(nan, 0.5); say("fuzz_nan", check_materials(&m, 1, 0)); }
    { CrMaterial m = metal(0.5, 1.5); say("metal_albedo", check_materials(&m, 1, 0)); }
    { CrMaterial m = dielectric(nan); say("param_nan", check_materials(&m, 1, 0)); m = dielectric(HUGE_VAL); say("param_inf", check_materials(&m, 1, 0)); m = lambertian(0); m.param = -HUGE_VAL; say("param_neg_inf", check_materials(&m, 1, 1)); }
    { std::vector<CrMaterial> m{dielectric(nan), lambertian(9)}; say("two_mat_faults_first_wins", check_materials(m.data(), 2, 1)); }
    // ---- a primitive's material, the sky
    say("prim_material_at_count", check_prim_material(3, 3));
    say("prim_material_last", check_prim_material(2, 3));
    say("prim_material_negative", check_prim_material(-1, 3));
    say("prim_material_int_max", check_prim_material(INT_MAX, INT_MAX));
    say("prim_material_int_min", check_prim_material(INT_MIN, INT_MAX));
    say("sky_kind", check_sky_kind(2));
    say("sky_kind_negative", check_sky_kind(-1));
    say("sky_default", check_sky_image(CR_SKY_DEFAULT, -1, 0));
    say("sky_image_at_count", check_sky_image(CR_SKY_SPHERICAL, 2, 2));
    say("sky_image_negative", check_sky_image(CR_SKY_SPHERICAL, -1, 2));
    say("sky_image_int_max", check_sky_image(CR_SKY_SPHERICAL, INT_MAX, INT_MAX));
    say("sky_image_ok", check_sky_image(CR_SKY_SPHERICAL, 1, 2));

    // ---- cr_update_materials: the shape of the arguments
    const CrMaterial one_m = metal(0.0, 0.5);
    const CrTexture one_t = solid(0, 0, 0);
    const int32_t some[2] = {0, 1};
    say("args_negative_materials", check_materials_args(&one_m, -1, nullptr, 0, nullptr, nullptr, 0));
    say("args_negative_textures", check_materials_args(nullptr, 0, &one_t, INT_MIN, nullptr, nullptr, 0));
    say("args_negative_assign", check_materials_args(nullptr, 0, nullptr, 0, some, some, -1));
    say("args_null_materials_with_count", check_materials_args(nullptr, 1, nullptr, 0, nullptr, nullptr, 0));
    say("args_null_textures_with_count", check_materials_args(nullptr, 0, nullptr, INT_MAX, nullptr, nullptr, 0));
    say("args_null_index", check_materials_args(nullptr, 0, nullptr, 0, nullptr, some, 2));
    say("args_null_material", check_materials_args(nullptr, 0, nullptr, 0, some, nullptr, INT_MAX));
    say("args_nothing", check_materials_args(nullptr, 0, nullptr, 0, nullptr, nullptr, 0));
    say("args_empty_tables", check_materials_args(&one_m, 0, &one_t, 0, nullptr, nullptr, 0));
    say("args_negative_before_null", check_materials_args(nullptr, -1, nullptr, 0, nullptr, nullptr, 2));          // two faults: the count's sign first
    say("args_contradiction_before_null_arrays", check_materials_args(nullptr, 1, nullptr, 0, nullptr, nullptr, 2));   // then the table, then the arrays

    // ---- cr_update_materials against a scene: prims 0..3 spheres / triangle of materials 0, 2, 1, 2; prim 4 a list; prim 5 a BVH element
    std::vector<CrPrimitive> P{prim(CR_PRIM_SPHERE, 0), prim(CR_PRIM_SPHERE, 2), prim(CR_PRIM_TRIANGLE, 1), prim(CR_PRIM_SPHERE, 2), prim(CR_PRIM_LIST, 77), prim(CR_PRIM_BVH, -5)};
    std::vector<CrMaterial> M{lambertian(0), metal(0.1, 0.5), dielectric(1.5)};
    std::vector<CrTexture> T{solid(0.5, 0.5, 0.5), image(0)};
    auto upd = [&](const std::vector<CrMaterial>* m, const std::vector<CrTexture>* t, const std::vector<int32_t>& idx, const std::vector<int32_t>& mat) {
        // an empty table is a table: a pointer that is not null beside a count of 0
        return check_materials_update(P.data(), (int64_t)P.size(), M.data(), (int32_t)M.size(), T.data(), (int32_t)T.size(), 1,
                                      m ? (m->empty() ? &one_m : m->data()) : nullptr, m ? (int32_t)m->size() : 0,
                                      t ? (t->empty() ? &one_t : t->data()) : nullptr, t ? (int32_t)t->size() : 0,
                                      idx.data(), mat.data(), (int32_t)idx.size());
    };
    say("upd_nothing", upd(nullptr, nullptr, {}, {}));
    say("upd_index_negative", upd(nullptr, nullptr, {0, -1}, {0, 0}));
    say("upd_index_at_count", upd(nullptr, nullptr, {6}, {0}));
    say("upd_index_int_max", upd(nullptr, nullptr, {INT_MAX}, {0}));
    say("upd_index_int_min", upd(nullptr, nullptr, {INT_MIN}, {0}));
    say("upd_twice", upd(nullptr, nullptr, {1, 3, 1}, {0, 0, 0}));
    say("upd_list", upd(nullptr, nullptr, {4}, {0}));
    say("upd_bvh", upd(nullptr, nullptr, {0, 5}, {0, 0}));
    say("upd_assign_ok", upd(nullptr, nullptr, {0, 1, 2, 3}, {2, 1, 0, 0}));
    say("upd_assign_at_count", upd(nullptr, nullptr, {0}, {3}));
    say("upd_assign_negative", upd(nullptr, nullptr, {0}, {-1}));
    say("upd_assign_int_max", upd(nullptr, nullptr, {0}, {INT_MAX}));
    say("upd_assign_int_min", upd(nullptr, nullptr, {0}, {INT_MIN}));
    { std::vector<CrMaterial> m{M[0], M[1], M[2]}; say("upd_shrink_to_largest_used_plus_one", upd(&m, nullptr, {}, {})); }
    { std::vector<CrMaterial> m{M[0], M[1]}; say("upd_shrink_below_used", upd(&m, nullptr, {}, {}));
      say("upd_shrink_one_still_uses_it", upd(&m, nullptr, {1}, {0}));
      say("upd_shrink_with_reassign", upd(&m, nullptr, {1, 3}, {0, 1})); }
    { std::vector<CrMaterial> m; say("upd_empty_table_under_primitives", upd(&m, nullptr, {}, {})); }
    { std::vector<CrMaterial> m{M[0], M[1], M[2], lambertian(1), lambertian(2)}; say("upd_new_materials_against_kept_textures", upd(&m, nullptr, {}, {}));
      std::vector<CrTexture> t{T[0], T[1], checker(0, 1)}; say("upd_both_tables_grow", upd(&m, &t, {3}, {4})); }
    { std::vector<CrTexture> t; say("upd_new_textures_against_kept_materials", upd(nullptr, &t, {}, {}));
      std::vector<CrMaterial> m{metal(0, 0.5), metal(0, 0.5), metal(0, 0.5)}; say("upd_no_textures_no_lambertian", upd(&m, &t, {}, {})); }
    { std::vector<CrTexture> t{T[0], image(1)}; say("upd_texture_image_against_n_images", upd(nullptr, &t, {}, {})); }
    { std::vector<CrTexture> t = chain(CR_MAX_CHECKER_DEPTH + 1); say("upd_depth_over", upd(nullptr, &t, {}, {})); }
    // two faults at once: the call's own refusals, then textures, materials, primitives -- cr_upload_scene's order
    say("order_range_before_twice", upd(nullptr, nullptr, {1, 1, 9}, {0, 0, 0}));
    say("order_range_before_list", upd(nullptr, nullptr, {4, 9}, {0, 0}));
    say("order_twice_before_list", upd(nullptr, nullptr, {4, 1, 1}, {0, 0, 0}));
    { std::vector<CrTexture> t{solid(3, 0, 0)}; say("order_twice_before_texture", upd(nullptr, &t, {1, 1}, {0, 0}));
      std::vector<CrMaterial> m{metal(2.0, 0.5)}; say("order_texture_before_material", upd(&m, &t, {}, {}));
      say("order_list_before_texture", upd(nullptr, &t, {4}, {0})); }
    { std::vector<CrMaterial> m{metal(2.0, 0.5)}; say("order_material_before_primitive", upd(&m, nullptr, {}, {})); }

    // ---- cr_update_image: images 0 (5 x 3) and 1 (64 x 32)
    const int32_t W[2] = {5, 64}, H[2] = {3, 32};
    const uint8_t px[3] = {1, 2, 3};
    auto img = [&](int32_t i, int32_t x0, int32_t y0, int32_t w, int32_t h, const void* p) { return check_image_update(i, 2, W, H, x0, y0, w, h, p); };
    say("img_whole", img(0, 0, 0, 5, 3, px));
    say("img_corner", img(0, 4, 2, 1, 1, px));
    say("img_null", img(0, 0, 0, 1, 1, nullptr));
    say("img_width_zero", img(0, 0, 0, 0, 1, px));
    say("img_height_negative", img(0, 0, 0, 1, -1, px));
    say("img_height_int_min", img(0, 0, 0, 1, INT_MIN, px));
    say("img_index_negative", img(-1, 0, 0, 1, 1, px));
    say("img_index_at_count", img(2, 0, 0, 1, 1, px));
    say("img_index_int_max", img(INT_MAX, 0, 0, 1, 1, px));
    say("img_x_one_over", img(0, 1, 0, 5, 3, px));
    say("img_y_one_over", img(1, 0, 1, 64, 32, px));
    say("img_x0_negative", img(1, -1, 0, 2, 1, px));
    say("img_y0_int_min", img(1, 0, INT_MIN, 1, 1, px));
    say("img_x_sum_overflows", img(1, INT_MAX, 0, INT_MAX, 1, px));       // x0 + width = 2^32 - 2: 64 bits hold it
    say("img_x_sum_wraps_to_small", img(1, 2, 0, INT_MAX, 1, px));        // in 32 bits 2 + INT_MAX is negative: "inside"
    say("img_y_sum_overflows", img(1, 0, INT_MAX, 1, INT_MAX, px));
    say("order_img_null_before_size", img(9, 0, 0, 0, 0, nullptr));
    say("order_img_size_before_index", img(9, 0, 0, 0, 1, px));
    say("order_img_index_before_rect", img(9, -1, 0, 1, 1, px));

    // ---- live_texture_remap where the device texture table changes size: 0, 1 solids; 2 checker(0, 1); 3 image; 4 checker(2, 3)
    std::vector<CrTexture> R{solid(0.1, 0.1, 0.1), solid(0.9, 0.9, 0.9), checker(0, 1), image(0), checker(2, 3)};
    remap("remap_all_solid", {lambertian(0), metal(0, 0.5), lambertian(1)}, R);                 // every top-level texture folded into its material
    remap("remap_dead_checker_becomes_live", {lambertian(2), metal(0, 0.5), lambertian(1)}, R); // a Lambertian switched from solid 0 to checker 2
    remap("remap_checker_back_to_solid", {lambertian(0), metal(0, 0.5), lambertian(1)}, R);
    remap("remap_image_alone", {lambertian(3)}, R);
    remap("remap_image_behind_a_checker_level", {lambertian(4)}, R);
    remap("remap_metal_names_no_texture", {metal(0, 0.5)}, R);
    remap("remap_no_textures", {metal(0, 0.5)}, {});
    return 0;
}
