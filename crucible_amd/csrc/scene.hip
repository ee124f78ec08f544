// scene.hip -- the scene on the handle: cr_upload_scene validates and deep-copies the description; the device steps
// that upload, refit and update share (wrapper boxes bottom-up, refit.hpp; the f32 screening records);
// cr_update_primitives (update.hpp); and cr_update_materials, cr_update_image, cr_set_sky,
// which run the descriptor checks of scene_checks.hpp that cr_upload_scene runs.
#include "handle.hpp"
#include "refit.hpp"
#include "screen.hpp"
#include "pack.hpp"
#include "scene_checks.hpp"
#include "update.hpp"

#include <chrono>

namespace cr {

// Boxes of every wrapper of `entries` (a device copy of the tree), bottom-up by level: for the ray times [ta, tb]
// of a frame (use_keys) or the construction-time boxes (!use_keys).
template <typename real>
int32_t run_box_kernels(CrHandle* h, DevScene<real>& ds, void* entries, real ta, real tb, bool use_keys) {
    for (size_t l = ds.level_begin.size() - 1; l-- > 0;) {
        const int32_t begin = ds.level_begin[l], end = ds.level_begin[l + 1];
        if (end <= begin) continue;
        const dim3 grid((unsigned)((end - begin + 255) / 256)), block(256);
        if (ds.ordered) hipLaunchKernelGGL((refit_level_kernel<real, true>), grid, block, 0, h->stream, (EntryO<real>*)entries, begin, end,
                                           (const Prim<real>*)ds.prims.p, (const Key<real>*)ds.keys.p, ta, tb, use_keys ? 1 : 0, (const int32_t*)ds.leaf_runs.p);
        else hipLaunchKernelGGL((refit_level_kernel<real, false>), grid, block, 0, h->stream, (Entry<real>*)entries, begin, end,
                                (const Prim<real>*)ds.prims.p, (const Key<real>*)ds.keys.p, ta, tb, use_keys ? 1 : 0, (const int32_t*)ds.leaf_runs.p);
    }
    HIP_TRY(h, hipGetLastError());
    return CR_OK;
}

// The f32 screening records of a (possibly refitted) f64 wrapper array, in the layout of the tree (ScreenEntry / ScreenEntryO).
// *usable = false when a finite f64 plane lies beyond the f32 range (screen_from_entries_kernel): the walk must not screen
// on these records.  Synchronises the stream.
int32_t make_screen(CrHandle* h, DevScene<double>& ds, const void* entries, DevBuf& out, bool* usable) {
    const size_t rec = ds.ordered ? sizeof(ScreenEntryO) : sizeof(ScreenEntry);
    HIP_TRY(h, out.ensure((size_t)ds.n_entries * rec, ds.ordered ? entry_pad<ScreenEntryO>() : entry_pad<ScreenEntry>()));
    HIP_TRY(h, ds.screen_overflow.ensure(sizeof(int32_t)));
    HIP_TRY(h, hipMemsetAsync(ds.screen_overflow.p, 0, sizeof(int32_t), h->stream));
    const dim3 grid((unsigned)((ds.n_entries + 255) / 256));
    int32_t* flag = (int32_t*)ds.screen_overflow.p;
    if (ds.ordered) hipLaunchKernelGGL(screen_from_ordered_entries_kernel, grid, dim3(256), 0, h->stream, (const EntryO<double>*)entries, (ScreenEntryO*)out.p, ds.n_entries, flag);
    else hipLaunchKernelGGL(screen_from_entries_kernel<double>, grid, dim3(256), 0, h->stream, (const Entry<double>*)entries, (ScreenEntry*)out.p, ds.n_entries, flag);
    HIP_TRY(h, hipGetLastError());
    int32_t overflow = 0;
    HIP_TRY(h, hipMemcpyAsync(&overflow, flag, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *usable = overflow == 0;
    return CR_OK;
}
// f32 scenes: the same boxes in ScreenEntry's link layout (the walk's inner loop reads that one), unordered trees only
int32_t make_screen(CrHandle* h, DevScene<float>& ds, const void* entries, DevBuf& out, bool* usable) {
    *usable = true;
    if (ds.ordered) { out.release(); return CR_OK; }
    HIP_TRY(h, out.ensure((size_t)ds.n_entries * sizeof(ScreenEntry), entry_pad<ScreenEntry>()));
    hipLaunchKernelGGL(screen_from_entries_kernel<float>, dim3((unsigned)((ds.n_entries + 255) / 256)), dim3(256), 0, h->stream, (const Entry<float>*)entries, (ScreenEntry*)out.p, ds.n_entries, (int32_t*)nullptr);
    HIP_TRY(h, hipGetLastError());
    return CR_OK;
}

// ---------------------------------------------------------------- cr_update_primitives (update.hpp)
// Everything that can refuse the call, before anything changes.
int32_t validate_update(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, int32_t flags) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (n < 0) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: negative count");
    if (n > 0 && !v) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: null values");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_update_primitives before cr_upload_scene");
    if (flags != CR_UPDATE_REFIT && flags != CR_UPDATE_REBUILD) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: unknown flags");
    const int64_t n_desc = (int64_t)h->prims.size();
    if (prim_index) {
        for (int32_t k = 0; k < n; k++)
            if (prim_index[k] < 0 || prim_index[k] >= n_desc) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: primitive index out of range");
        std::vector<int32_t> sorted(prim_index, prim_index + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: a primitive is named twice");
    } else if (n > n_desc) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: primitive index out of range");
    auto finite = [](double x) { return x == x && x != HUGE_VAL && x != -HUGE_VAL; };
    for (int32_t k = 0; k < n; k++) {
        const CrPrimitive& p = h->prims[(size_t)(prim_index ? prim_index[k] : k)];
        if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) return fail(h, CR_ERR_INVALID_ARG, "cr_update_primitives: a list element has no coordinates to update");
        const double* row = v + (size_t)k * 9;
        const int nv = p.kind == CR_PRIM_SPHERE ? 4 : 9;
        for (int j = 0; j < nv; j++) if (!finite(row[j])) return fail(h, CR_ERR_INVALID_ARG, "primitive coordinate is not finite");
        if (p.kind == CR_PRIM_SPHERE && !(row[3] >= 0.0)) return fail(h, CR_ERR_INVALID_ARG, "Cannot make a sphere with negative radius");   // sphere.rs:26
    }
    // the construction-time box of a HitList / BVHWrapper element is not the union of its objects' boxes: a refit would not
    // reproduce it
    if (h->has_list_elements) return fail(h, CR_ERR_UNSUPPORTED, "cr_update_primitives: the scene holds a HitList or BVHWrapper element");
    return CR_OK;
}

// CR_UPDATE_REFIT on one built precision: the staged rows into the primitive records, then the construction-time boxes of
// every wrapper bottom-up, the screening records, and the host's copy of the tree.  The topology stays.
template <typename real>
static int32_t refit_updated(CrHandle* h, const int32_t* d_index, const double* d_rows, int32_t n) {
    DevScene<real>& ds = dev_scene<real>(h);
    if (!ds.built || ds.n_prims == 0) return CR_OK;
    if (!ds.desc_pos_valid) return fail(h, CR_ERR_UNSUPPORTED, "cr_update_primitives: the scene holds a HitList or BVHWrapper element");
    hipLaunchKernelGGL((update_prims_kernel<real>), dim3((unsigned)((n + kUpdateBlock - 1) / kUpdateBlock)), dim3(kUpdateBlock), 0, h->stream,
                       (Prim<real>*)ds.prims.p, ds.n_prims, (const int32_t*)ds.desc_pos.p, (int32_t)h->prims.size(), d_index, d_rows, n);
    HIP_TRY(h, hipGetLastError());
    if (ds.n_entries == 0) return CR_OK;
    int32_t rc = run_box_kernels<real>(h, ds, ds.entries.p, real(0), real(0), false);
    if (rc != CR_OK) return rc;
    rc = make_screen(h, ds, ds.entries.p, ds.screen, &ds.screen_usable);
    if (rc != CR_OK) return rc;
    if (ds.host_entries.size() != (size_t)ds.n_entries) return CR_OK;   // nothing to export (a scene with a BVHWrapper element; not reached)
    if (!ds.ordered) {   // the device records are the host's, box for box and link for link
        HIP_TRY(h, hipMemcpyAsync(ds.host_entries.data(), ds.entries.p, (size_t)ds.n_entries * sizeof(Entry<real>), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {             // EntryO records: only their boxes go into the host's Entry records
        std::vector<EntryO<real>> eo((size_t)ds.n_entries);
        HIP_TRY(h, hipMemcpyAsync(eo.data(), ds.entries.p, eo.size() * sizeof(EntryO<real>), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < eo.size(); i++) for (int k = 0; k < 6; k++) ds.host_entries[i].b[k] = eo[i].b[k];
    }
    ds.nan_planes = has_nan_plane(ds.host_entries);
    return CR_OK;
}

// After validate_update: the edit itself.
int32_t apply_update(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, int32_t flags) {
    if (n == 0) return CR_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drop_frame_trees(h);   // CR_REFIT_REBUILD's trees were built over the primitives as they were
    const bool refit = flags == CR_UPDATE_REFIT && (h->s32.built || h->s64.built);
    if (refit) {   // one staged buffer: the rows, then the indices; the stream orders the copy after earlier renders
        const size_t row_bytes = (size_t)n * 9 * sizeof(double), idx_bytes = prim_index ? (size_t)n * sizeof(int32_t) : 0;
        HIP_TRY(h, h->update_stage.ensure(row_bytes + idx_bytes));
        HIP_TRY(h, hipMemcpyAsync(h->update_stage.p, v, row_bytes, hipMemcpyHostToDevice, h->stream));
        if (prim_index) HIP_TRY(h, hipMemcpyAsync((char*)h->update_stage.p + row_bytes, prim_index, idx_bytes, hipMemcpyHostToDevice, h->stream));
    } else HIP_TRY(h, hipStreamSynchronize(h->stream));   // a rebuild frees and refills what an earlier render may still read
    for (int32_t k = 0; k < n; k++) {   // the host copy: what a rebuild, a precision not built yet and a hidden primitive see
        CrPrimitive& p = h->prims[(size_t)(prim_index ? prim_index[k] : k)];
        const int nv = p.kind == CR_PRIM_SPHERE ? 4 : 9;
        for (int j = 0; j < nv; j++) p.v[j] = v[(size_t)k * 9 + j];
    }
    if (flags == CR_UPDATE_REBUILD) { h->s32.built = false; h->s64.built = false; return CR_OK; }
    if (!refit) return CR_OK;
    const double* d_rows = (const double*)h->update_stage.p;
    const int32_t* d_index = prim_index ? (const int32_t*)((const char*)h->update_stage.p + (size_t)n * 9 * sizeof(double)) : nullptr;
    int32_t rc = refit_updated<float>(h, d_index, d_rows, n);
    if (rc == CR_OK) rc = refit_updated<double>(h, d_index, d_rows, n);
    hipError_t e = hipStreamSynchronize(h->stream);   // the caller's arrays and the staged buffer are free from here on
    if (e != hipSuccess && rc == CR_OK) { h->error = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = CR_ERR_HIP; }
    return rc;
}

// ---------------------------------------------------------------- cr_update_materials, cr_update_image, cr_set_sky
// Everything that can refuse cr_update_materials, before anything changes: the call's own refusals, then cr_upload_scene's
// checks of the description the edit would leave (scene_checks.hpp).
int32_t validate_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                           const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    if (!h) return CR_ERR_INVALID_ARG;
    SceneCheck c = check_materials_args(materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
    if (!c.ok()) return fail(h, c.code, c.msg);
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_update_materials before cr_upload_scene");
    c = check_materials_update(h->prims.data(), (int64_t)h->prims.size(), h->materials.data(), (int32_t)h->materials.size(), h->textures.data(),
                               (int32_t)h->textures.size(), h->n_images, materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
    return c.ok() ? CR_OK : fail(h, c.code, c.msg);
}

// The device's material and texture tables of one precision from the host copy, where that precision holds side tables at
// all (else its next build packs them): the bytes an upload makes, n_mats / n_texs / lds_bytes with them, and the frame
// tree's aliases.  A buffer that must grow is exchanged after the stream has drained; the copies are ordered on the stream.
template <typename real>
static int32_t repack_side_tables(CrHandle* h) {
    DevScene<real>& ds = dev_scene<real>(h);
    if (!ds.side_tables) return CR_OK;
    std::vector<Mat<real>> mats;
    std::vector<Tex<real>> texs;
    pack_side_tables<real>(h->materials, h->textures, mats, texs);
    const size_t mat_bytes = mats.size() * sizeof(Mat<real>), tex_bytes = texs.size() * sizeof(Tex<real>);
    // a buffer goes when its table outgrows it, or shrinks below half of it (a table that grew once does not hold its
    // largest size for the handle's life; an edit of a few records exchanges nothing)
    auto misfit = [](const DevBuf& b, size_t need) { return need > b.bytes || 2 * need < b.bytes; };
    const size_t mat_need = mat_bytes ? mat_bytes : 16, tex_need = tex_bytes ? tex_bytes : 16;
    if (misfit(ds.mats, mat_need) || misfit(ds.texs, tex_need)) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier render may still read the buffer that goes
        hipError_t e = hipSuccess;
        if (misfit(ds.mats, mat_need)) { ds.mats.release(); e = ds.mats.ensure(mat_need); }
        if (e == hipSuccess && misfit(ds.texs, tex_need)) { ds.texs.release(); e = ds.texs.ensure(tex_need); }
        if (e != hipSuccess) {   // out of memory: the next use builds again and uploads the tables from the host copy
            ds.side_tables = false; ds.built = false;
            return fail(h, CR_ERR_HIP, std::string("cr_update_materials: ") + hipGetErrorString(e));
        }
    }
    if (mat_bytes) HIP_TRY(h, hipMemcpyAsync(ds.mats.p, mats.data(), mat_bytes, hipMemcpyHostToDevice, h->stream));
    if (tex_bytes) HIP_TRY(h, hipMemcpyAsync(ds.texs.p, texs.data(), tex_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // `mats` and `texs` are this function's
    ds.n_mats = (int32_t)mats.size(); ds.n_texs = (int32_t)texs.size();
    ds.lds_bytes = scene_lds_bytes(ds);
    DevScene<real>& fs = frame_scene<real>(h);
    if (fs.built) { alias_side_tables(fs, ds); fs.lds_bytes = scene_lds_bytes(fs); }
    return CR_OK;
}

// The staged assignments into the primitive records of one built precision.  Without desc_pos (a scene with a HitList or
// BVHWrapper element) the tree rebuilds at next use from the edited host copy instead; the side tables stay.
template <typename real>
static int32_t assign_updated(CrHandle* h, const int32_t* d_index, const int32_t* d_material, int32_t n) {
    DevScene<real>& ds = dev_scene<real>(h);
    if (!ds.built) return CR_OK;
    if (!ds.desc_pos_valid) { ds.built = false; return CR_OK; }
    if (ds.n_prims == 0) return CR_OK;
    hipLaunchKernelGGL((assign_materials_kernel<real>), dim3((unsigned)((n + kUpdateBlock - 1) / kUpdateBlock)), dim3(kUpdateBlock), 0, h->stream,
                       (Prim<real>*)ds.prims.p, ds.n_prims, (const int32_t*)ds.desc_pos.p, (int32_t)h->prims.size(), d_index, d_material, n);
    HIP_TRY(h, hipGetLastError());
    return CR_OK;
}

// After validate_materials: the edit itself.
int32_t apply_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                        const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    if (!materials && !textures && n_assign == 0) return CR_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int32_t rc = CR_OK;
    if (materials || textures) {   // the host copy first: the tables are packed from it
        if (materials) h->materials.assign(materials, materials + n_materials);
        if (textures) h->textures.assign(textures, textures + n_textures);
        rc = repack_side_tables<float>(h);
        if (rc == CR_OK) rc = repack_side_tables<double>(h);
        if (rc != CR_OK) return rc;
    }
    if (n_assign == 0) return CR_OK;
    drop_frame_trees(h);   // CR_REFIT_REBUILD's primitive records are gathered copies
    const bool on_device = (h->s32.built && h->s32.desc_pos_valid) || (h->s64.built && h->s64.desc_pos_valid);
    const size_t idx_bytes = (size_t)n_assign * sizeof(int32_t);
    if (on_device) {   // one staged buffer: the indices, then the materials; the stream orders the copy after earlier renders
        HIP_TRY(h, h->update_stage.ensure(2 * idx_bytes));
        HIP_TRY(h, hipMemcpyAsync(h->update_stage.p, prim_index, idx_bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync((char*)h->update_stage.p + idx_bytes, prim_material, idx_bytes, hipMemcpyHostToDevice, h->stream));
    } else HIP_TRY(h, hipStreamSynchronize(h->stream));   // a rebuild frees and refills what an earlier render may still read
    for (int32_t k = 0; k < n_assign; k++) h->prims[(size_t)prim_index[k]].material = prim_material[k];   // what a rebuild, a precision not built yet and a hidden primitive see
    const int32_t* d_index = (const int32_t*)h->update_stage.p;
    const int32_t* d_material = (const int32_t*)((const char*)h->update_stage.p + idx_bytes);
    rc = assign_updated<float>(h, d_index, d_material, n_assign);
    if (rc == CR_OK) rc = assign_updated<double>(h, d_index, d_material, n_assign);
    hipError_t e = hipStreamSynchronize(h->stream);   // the caller's arrays and the staged buffer are free from here on
    if (e != hipSuccess && rc == CR_OK) { h->error = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = CR_ERR_HIP; }
    return rc;
}

int32_t validate_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_update_image before cr_upload_scene");
    const SceneCheck c = check_image_update(image, h->n_images, h->image_w.data(), h->image_h.data(), x0, y0, width, height, rgb8);
    return c.ok() ? CR_OK : fail(h, c.code, c.msg);
}

// The rectangle's bytes into update_stage on the stream, then pack_texels_kernel writes their words where pack_images put them
int32_t apply_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)width * (size_t)height;
    HIP_TRY(h, h->update_stage.ensure(3 * n));
    HIP_TRY(h, hipMemcpyAsync(h->update_stage.p, rgb8, 3 * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pack_texels_kernel, dim3((unsigned)((n + kUpdateBlock - 1) / kUpdateBlock)), dim3(kUpdateBlock), 0, h->stream,
                       (uint32_t*)h->texels.p, h->n_texels, h->image_offset[(size_t)image], h->image_w[(size_t)image], x0, y0, width, height,
                       (const uint8_t*)h->update_stage.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the caller's array and the staged buffer are free from here on
    return CR_OK;
}

int32_t validate_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_set_sky before cr_upload_scene");
    SceneCheck c = check_sky_kind(sky_kind);
    if (c.ok()) c = check_sky_image(sky_kind, sky_image, h->n_images);
    return c.ok() ? CR_OK : fail(h, c.code, c.msg);
}
// render_typed copies the two fields into a launch's KernelArgs: a render launched earlier keeps the sky it was launched with
void apply_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image) { h->sky_kind = sky_kind; h->sky_image = sky_image; }

template int32_t run_box_kernels<float>(CrHandle*, DevScene<float>&, void*, float, float, bool);
template int32_t run_box_kernels<double>(CrHandle*, DevScene<double>&, void*, double, double, bool);

}   // namespace cr

using namespace cr;

extern "C" {

int32_t cr_upload_scene(CrHandle* h, const CrSceneDesc* s) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!s) return fail(h, CR_ERR_INVALID_ARG, "scene is null");
    if (s->n_prims < 0 || s->n_materials < 0 || s->n_textures < 0 || s->n_images < 0 || s->n_keys < 0)
        return fail(h, CR_ERR_INVALID_ARG, "negative count");
    if (s->n_prims >= (1 << 29)) return fail(h, CR_ERR_INVALID_ARG, "too many primitives");
    if ((s->n_prims > 0 && !s->prims) || (s->n_materials > 0 && !s->materials) || (s->n_textures > 0 && !s->textures) ||
        (s->n_images > 0 && !s->images) || (s->n_keys > 0 && !s->keys))
        return fail(h, CR_ERR_INVALID_ARG, "a descriptor array is null although its count is not zero");
    auto finite = [](double x) { return check_finite(x); };
    auto refuse = [&](const SceneCheck& c) { return fail(h, c.code, c.msg); };   // scene_checks.hpp: the checks cr_update_materials and cr_set_sky share
    { const SceneCheck c = check_textures(s->textures, s->n_textures, s->n_images); if (!c.ok()) return refuse(c); }
    { const SceneCheck c = check_materials(s->materials, s->n_materials, s->n_textures); if (!c.ok()) return refuse(c); }
    for (int i = 0; i < s->n_keys; i++) {
        const CrKeyframe& k = s->keys[i];
        if (k.channel < CR_KEY_TX || k.channel > CR_KEY_SCALE_Z || (k.interp != CR_KEY_NERP && k.interp != CR_KEY_LERP))
            return fail(h, CR_ERR_INVALID_ARG, "bad keyframe");
    }
    {   // lists (CR_PRIM_LIST): whole-number ranges of flagged spheres/triangles, every flagged primitive in exactly one
        std::vector<char> owned((size_t)std::max(0, s->n_prims), 0);
        for (int i = 0; i < s->n_prims; i++) {
            const CrPrimitive& p = s->prims[i];
            if (p.kind != CR_PRIM_LIST && p.kind != CR_PRIM_BVH) continue;
            if (p.flags & (CR_PRIM_MEMBER | CR_PRIM_HIDDEN)) return fail(h, CR_ERR_INVALID_ARG, "a list is a scene element: it cannot be hidden or be an object of a list");
            if (p.kind == CR_PRIM_BVH && (p.flags & CR_LIST_EMPTY_BOX)) return fail(h, CR_ERR_INVALID_ARG, "CR_LIST_EMPTY_BOX applies to lists");
            const double first = p.v[0], count = p.v[1];
            if (!(first >= 0.0 && count >= 0.0 && first == std::floor(first) && count == std::floor(count) && first + count <= (double)s->n_prims))
                return fail(h, CR_ERR_INVALID_ARG, "list object range out of bounds");
            for (int64_t k = (int64_t)first; k < (int64_t)(first + count); k++) {
                const CrPrimitive& m = s->prims[k];
                if ((m.kind != CR_PRIM_SPHERE && m.kind != CR_PRIM_TRIANGLE) || !(m.flags & CR_PRIM_MEMBER))
                    return fail(h, CR_ERR_INVALID_ARG, "a list's objects must be spheres or triangles flagged CR_PRIM_MEMBER");
                if (owned[(size_t)k]) return fail(h, CR_ERR_INVALID_ARG, "a primitive is an object of two lists");
                owned[(size_t)k] = 1;
            }
        }
        for (int i = 0; i < s->n_prims; i++)
            if ((s->prims[i].flags & CR_PRIM_MEMBER) && !owned[(size_t)i]) return fail(h, CR_ERR_INVALID_ARG, "a primitive flagged CR_PRIM_MEMBER belongs to no list");
    }
    for (int i = 0; i < s->n_prims; i++) {
        const CrPrimitive& p = s->prims[i];
        if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) continue;
        if (p.kind != CR_PRIM_SPHERE && p.kind != CR_PRIM_TRIANGLE) return fail(h, CR_ERR_INVALID_ARG, "unknown primitive kind");
        { const SceneCheck c = check_prim_material(p.material, s->n_materials); if (!c.ok()) return refuse(c); }
        if (p.key_count < 0 || p.key_first < 0 || p.key_first + p.key_count > s->n_keys) return fail(h, CR_ERR_INVALID_ARG, "primitive keyframe range out of bounds");
        for (int k = 0; k < p.key_count; k++) {   // the Scene API type-checks scale keys (scene_animator.rs:38-183)
            const int32_t ch = s->keys[p.key_first + k].channel;
            if (p.kind == CR_PRIM_SPHERE && ch > CR_KEY_RADIUS) return fail(h, CR_ERR_INVALID_ARG, "ScaleX/ScaleY/ScaleZ cannot apply to Spheres");
            if (p.kind == CR_PRIM_TRIANGLE && ch == CR_KEY_RADIUS) return fail(h, CR_ERR_INVALID_ARG, "ScaleR can only be applied to Spheres");
        }
        int nv = p.kind == CR_PRIM_SPHERE ? 4 : 9;
        for (int k = 0; k < nv; k++) if (!finite(p.v[k])) return fail(h, CR_ERR_INVALID_ARG, "primitive coordinate is not finite");
        if (p.kind == CR_PRIM_SPHERE && !(p.v[3] >= 0.0)) return fail(h, CR_ERR_INVALID_ARG, "Cannot make a sphere with negative radius");   // sphere.rs:26
    }
    { const SceneCheck c = check_sky_kind(s->sky_kind); if (!c.ok()) return refuse(c); }
    const int32_t bvh_base = s->bvh_mode & 0xFF, bvh_flags = s->bvh_mode & ~0xFF;
    if (s->bvh_mode < 0 || bvh_base > CR_BVH_LBVH || (bvh_flags & ~CR_BVH_BUILD_DEVICE)) return fail(h, CR_ERR_INVALID_ARG, "unknown bvh_mode");
    if ((bvh_flags & CR_BVH_BUILD_DEVICE) && bvh_base == CR_BVH_REFERENCE)
        return fail(h, CR_ERR_UNSUPPORTED, "CR_BVH_BUILD_DEVICE: the reference tree's stable sort has no device form (use it with CR_BVH_SAH, CR_BVH_SAH_ORDERED or CR_BVH_LBVH)");
    { const SceneCheck c = check_sky_image(s->sky_kind, s->sky_image, s->n_images); if (!c.ok()) return refuse(c); }
    for (int i = 0; i < s->n_images; i++)
        if (s->images[i].width < 1 || s->images[i].height < 1 || !s->images[i].rgb8) return fail(h, CR_ERR_INVALID_ARG, "bad image");

    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto t_begin = std::chrono::steady_clock::now();
    h->prims.assign(s->prims, s->prims + s->n_prims);
    h->materials.assign(s->materials, s->materials + s->n_materials);
    h->textures.assign(s->textures, s->textures + s->n_textures);
    h->keys.assign(s->keys, s->keys + s->n_keys);
    h->sky_kind = s->sky_kind; h->sky_image = s->sky_image; h->bvh_mode = bvh_base; h->bvh_device = (bvh_flags & CR_BVH_BUILD_DEVICE) != 0;
    if (!h->bvh_device) h->sah_work.release();
    h->s32.built = false; h->s64.built = false;
    h->s32.side_tables = false; h->s64.side_tables = false;
    drop_frame_trees(h);
    h->has_list_elements = false;
    for (const CrPrimitive& p : h->prims) h->has_list_elements |= p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH;
    // images: RGB8 -> RGBA8 words, one flat texel array (pack.hpp)
    std::vector<ImageRef> refs;
    std::vector<uint32_t> texels;
    if (!pack_images(s->images, s->n_images, refs, texels)) return fail(h, CR_ERR_INVALID_ARG, "too many texels");
    HIP_TRY(h, h->images.ensure(refs.size() * sizeof(ImageRef) + 16));
    HIP_TRY(h, h->texels.ensure(texels.size() * 4));
    if (!refs.empty()) HIP_TRY(h, hipMemcpy(h->images.p, refs.data(), refs.size() * sizeof(ImageRef), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->texels.p, texels.data(), texels.size() * 4, hipMemcpyHostToDevice));
    h->n_images = s->n_images;
    h->image_w.resize(refs.size()); h->image_h.resize(refs.size()); h->image_offset.resize(refs.size());
    for (size_t i = 0; i < refs.size(); i++) { h->image_w[i] = refs[i].w; h->image_h[i] = refs[i].h; h->image_offset[i] = refs[i].offset; }
    h->n_texels = texels.size();
    h->has_scene = true;
    h->upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return CR_OK;
}

int32_t cr_update_primitives(CrHandle* h, const int32_t* prim_index, const double* v, int32_t n, int32_t flags) {
    int32_t rc = validate_update(h, prim_index, v, n, flags);
    if (rc != CR_OK) return rc;
    return apply_update(h, prim_index, v, n, flags);
}

int32_t cr_update_materials(CrHandle* h, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                            const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    int32_t rc = validate_materials(h, materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
    if (rc != CR_OK) return rc;
    return apply_materials(h, materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
}

int32_t cr_update_image(CrHandle* h, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8) {
    int32_t rc = validate_image(h, image, x0, y0, width, height, rgb8);
    if (rc != CR_OK) return rc;
    return apply_image(h, image, x0, y0, width, height, rgb8);
}

int32_t cr_set_sky(CrHandle* h, int32_t sky_kind, int32_t sky_image) {
    int32_t rc = validate_sky(h, sky_kind, sky_image);
    if (rc != CR_OK) return rc;
    apply_sky(h, sky_kind, sky_image);
    return CR_OK;
}

}   // extern "C"
