// build.hip -- from the handle's host copy of the scene to a precision's device copy, as stages (build_dev_scene): the host
// side of every stage -- the objects and their boxes, the tree builders, the leaf layout -- is tree.hpp, which knows nothing
// of the device; this unit runs the device side of the LBVH and SAH builds, uploads what the stages made and has the boxes
// filled in.  cr_export_bvh hands the tree back, cr_build_info what the build did.  Also the second tree of refit_boxes =
// CR_REFIT_REBUILD (build_frame_scene, select_tree; cr_export_render_bvh, cr_frame_build_info).  Includes hipcub (as
// sah_device.hip does, the driver of the device-side SAH build this unit calls under CR_BVH_BUILD_DEVICE).
#include "handle.hpp"
#include "tree.hpp"
#include "refit.hpp"
#include <hipcub/hipcub.hpp>

#include <chrono>

namespace cr {

// CR_BVH_LBVH (lbvh.hpp): keys, sort and topology on the device; the node graph is then numbered into the
// level-order wrapper array (tree.hpp lbvh_number; boxes are filled in later by run_box_kernels).  `order` receives the primitives' sorted order.
template <typename real>
int32_t build_lbvh(CrHandle* h, const std::vector<Prim<real>>& src, const std::vector<real>* bmin, const std::vector<real>* bmax,
                   std::vector<int32_t>& order, std::vector<Entry<real>>& entries, std::vector<int32_t>& level_begin) {
    const int32_t n = (int32_t)src.size();
    entries.clear();
    level_begin.assign(1, 0);
    if (n == 0) return CR_OK;
    const LbvhBounds bnd = lbvh_bounds(bmin, bmax, n);
    DevBuf d_src, d_keys, d_keys2, d_idx, d_idx2, d_tmp, d_children;
#define LBVH_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(h, CR_ERR_HIP, hipGetErrorString(e_)); } while (0)
    LBVH_TRY(d_src.ensure((size_t)n * sizeof(Prim<real>)));
    LBVH_TRY(hipMemcpyAsync(d_src.p, src.data(), (size_t)n * sizeof(Prim<real>), hipMemcpyHostToDevice, h->stream));
    LBVH_TRY(d_keys.ensure((size_t)n * 8)); LBVH_TRY(d_keys2.ensure((size_t)n * 8));
    LBVH_TRY(d_idx.ensure((size_t)n * 4)); LBVH_TRY(d_idx2.ensure((size_t)n * 4));
    LBVH_TRY(d_children.ensure((size_t)std::max(1, n - 1) * 8));
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL((lbvh_key_kernel<real>), grid, block, 0, h->stream, (const Prim<real>*)d_src.p, n, bnd, (uint64_t*)d_keys.p, (int32_t*)d_idx.p);
    LBVH_TRY(hipGetLastError());
    size_t tmp_bytes = 0;
    LBVH_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint64_t*)d_keys.p, (uint64_t*)d_keys2.p, (const int32_t*)d_idx.p,
                                                (int32_t*)d_idx2.p, n, 0, 63, h->stream));
    LBVH_TRY(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    LBVH_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, (const uint64_t*)d_keys.p, (uint64_t*)d_keys2.p, (const int32_t*)d_idx.p,
                                                (int32_t*)d_idx2.p, n, 0, 63, h->stream));
    if (n >= 2) {
        hipLaunchKernelGGL(lbvh_topology_kernel, dim3((unsigned)((n - 1 + 255) / 256)), block, 0, h->stream, (const uint64_t*)d_keys2.p, n, (int32_t*)d_children.p);
        LBVH_TRY(hipGetLastError());
    }
    order.resize(n);
    std::vector<int32_t> children((size_t)2 * std::max(1, n - 1));
    LBVH_TRY(hipMemcpyAsync(order.data(), d_idx2.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (n >= 2) LBVH_TRY(hipMemcpyAsync(children.data(), d_children.p, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost, h->stream));
    LBVH_TRY(hipStreamSynchronize(h->stream));
#undef LBVH_TRY
    if (!lbvh_number(children, n, entries, level_begin)) return fail(h, CR_ERR_HIP, "LBVH: malformed topology from the device");
    return CR_OK;
}

// The CR_BVH_SAH / CR_BVH_SAH_ORDERED tree over n >= 1 primitive boxes: the pre-order wrappers re-laid
// level by level, the split axes and the primitive order.  on_device: the node graph and the order come from the device
// builder (sah_device.hpp), never the host's -- from bmin / bmax, or, resident, from the boxes h->sah_work.box already
// holds (bmin / bmax are then not read); the wrapper boxes are left for run_box_kernels.  Otherwise the host SahBuilder.
template <typename real>
int32_t sah_tree(CrHandle* h, const std::vector<real>* bmin, const std::vector<real>* bmax, int32_t n, bool on_device, bool resident,
                 std::vector<int32_t>& order, std::vector<Entry<real>>& entries, std::vector<int8_t>& axis, std::vector<int32_t>& level_begin,
                 SahDeviceStats& dev_stats) {
    if (!on_device) { sah_host_tree(bmin, bmax, n, order, entries, axis, level_begin); return CR_OK; }
    std::vector<SahNodeRec> graph;
    int32_t rc;
    if (resident) rc = build_sah_device_resident(h, n, graph, order, dev_stats);
    else {
        std::vector<double> box6((size_t)n * 6);
        for (int32_t i = 0; i < n; i++) for (int a = 0; a < 3; a++) { box6[(size_t)i * 6 + a] = (double)bmin[a][i]; box6[(size_t)i * 6 + 3 + a] = (double)bmax[a][i]; }
        rc = build_sah_device(h, box6.data(), n, graph, order, dev_stats);
    }
    if (rc != CR_OK) return rc;
    sah_graph_tree(graph, entries, axis, level_begin);
    return CR_OK;
}

static hipError_t upload(DevBuf& d, const void* src_p, size_t bytes, size_t front_pad = 0) {
    hipError_t e = d.ensure(bytes ? bytes : 16, front_pad);
    if (e != hipSuccess) return e;
    if (bytes) return hipMemcpy(d.p, src_p, bytes, hipMemcpyHostToDevice);
    return hipSuccess;
}

// The wrapper array onto the device in the layout of the mode: `entries` with the links of `dev_entries` (the same records,
// or those that name primitive runs), or under CR_BVH_SAH_ORDERED the EntryO records with their per-octant links.
template <typename real>
int32_t upload_entries(CrHandle* h, DevScene<real>& ds, const std::vector<Entry<real>>& entries, const std::vector<Entry<real>>& dev_entries,
                       const std::vector<int8_t>& axis) {
    ds.entry_bytes = ds.ordered ? sizeof(EntryO<real>) : sizeof(Entry<real>);
    if (ds.ordered) {
        const std::vector<EntryO<real>> eo = ordered_entries(entries, axis);
        HIP_TRY(h, upload(ds.entries, eo.data(), eo.size() * sizeof(EntryO<real>), entry_pad<EntryO<real>>()));
    } else
    HIP_TRY(h, upload(ds.entries, dev_entries.data(), dev_entries.size() * sizeof(Entry<real>), entry_pad<Entry<real>>()));
    return CR_OK;
}

// After the uploads: where the builder left the wrapper boxes to the device (device_boxes), run_box_kernels fills them --
// the construction-time boxes, or with use_keys the boxes over the ray times [ta, tb] -- and the host's records take them
// back; then the f32 screening records of an f64 scene / the link-layout records of an f32 scene (pathtrace.hpp walk_round).
template <typename real>
int32_t finish_boxes(CrHandle* h, DevScene<real>& ds, std::vector<Entry<real>>& entries, bool device_boxes, real ta, real tb, bool use_keys) {
    if (device_boxes && ds.n_entries > 0) {
        int32_t rc = run_box_kernels<real>(h, ds, ds.entries.p, ta, tb, use_keys);
        if (rc != CR_OK) return rc;
        if (!ds.ordered) {
            HIP_TRY(h, hipMemcpyAsync(entries.data(), ds.entries.p, entries.size() * sizeof(Entry<real>), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        } else {   // EntryO records: only their boxes go into the host's Entry records
            std::vector<EntryO<real>> eo(entries.size());
            HIP_TRY(h, hipMemcpyAsync(eo.data(), ds.entries.p, eo.size() * sizeof(EntryO<real>), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < eo.size(); i++) for (int k = 0; k < 6; k++) entries[i].b[k] = eo[i].b[k];
        }
    }
    ds.nan_planes = has_nan_plane(entries);
    if (ds.n_entries > 0) {
        int32_t rc = make_screen(h, ds, ds.entries.p, ds.screen, &ds.screen_usable);
        if (rc != CR_OK) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else ds.screen.release();
    return CR_OK;
}

// What a build did (cr_build_info, cr_frame_build_info); total_ms runs from t_begin to now
static CrBuildInfo build_info(int32_t bvh_mode, bool on_device, int32_t n_wrappers, const SahDeviceStats& dev_stats, double tree_ms,
                              std::chrono::steady_clock::time_point t_begin) {
    CrBuildInfo info = CrBuildInfo();
    info.bvh_mode = bvh_mode;
    info.built_on_device = on_device ? 1 : 0;
    info.n_wrappers = n_wrappers;
    info.device_rounds = dev_stats.rounds; info.large_nodes = dev_stats.large_nodes;
    info.small_subtrees = dev_stats.small_subtrees; info.small_threshold = dev_stats.small_threshold;
    info.tree_ms = tree_ms;
    info.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return info;
}

// Stage 2 of build_dev_scene: the topology, by the mode's builder.  device_boxes: the wrapper boxes are left to the device.
template <typename real>
int32_t build_topology(CrHandle* h, SceneBoxes<real>& in, std::vector<int8_t>& axis, std::vector<int32_t>& level_begin, Spliced<real>& spliced,
                       bool& device_boxes, SahDeviceStats& dev_stats) {
    const int32_t n = (int32_t)in.objs.size();
    Builder<real>& b = in.b;
    device_boxes = false;
    if (h->bvh_mode == CR_BVH_LBVH) {
        device_boxes = true;
        return build_lbvh<real>(h, in.src, b.bmin, b.bmax, b.order, b.entries, level_begin);
    }
    // the device SAH builder; fewer than 3 primitives are one leaf, written on the host
    device_boxes = h->bvh_device && (h->bvh_mode == CR_BVH_SAH || h->bvh_mode == CR_BVH_SAH_ORDERED) && n >= 3;
    if (device_boxes) return sah_tree<real>(h, b.bmin, b.bmax, n, true, false, b.order, b.entries, axis, level_begin, dev_stats);
    host_topology(h->prims, h->bvh_mode, in, axis, level_begin, spliced);
    return CR_OK;
}

// Stages 4 and 5: the side tables, then everything onto the device, and what the kernels need to know about it
template <typename real>
int32_t upload_scene(CrHandle* h, DevScene<real>& ds, const SceneBoxes<real>& in, const LeafLayout<real>& lay, const std::vector<int8_t>& axis, bool spliced) {
    const Builder<real>& b = in.b;
    // Device texture table, materials, textures and keyframes (pack.hpp)
    std::vector<Mat<real>> mats;
    std::vector<Tex<real>> texs;
    pack_side_tables<real>(h->materials, h->textures, mats, texs);
    std::vector<Key<real>> keys(h->keys.size());
    if (!keys.empty()) memset(keys.data(), 0, keys.size() * sizeof(Key<real>));
    for (size_t i = 0; i < h->keys.size(); i++) key_to_real(h->keys[i], keys[i]);
    { int32_t rc = upload_entries<real>(h, ds, b.entries, lay.own_entries ? lay.dev_entries : b.entries, axis); if (rc != CR_OK) return rc; }
    HIP_TRY(h, upload(ds.leaf_runs, lay.leaf_runs.data(), lay.leaf_runs.size() * sizeof(int32_t)));
    ds.has_leaf_runs = !lay.leaf_runs.empty();
    ds.has_lists = in.any_lists;
    HIP_TRY(h, upload(ds.prims, lay.leaf_prims.data(), lay.leaf_prims.size() * sizeof(Prim<real>)));
    if (!ds.side_tables) {   // a rebuild after cr_update_primitives: these still hold the uploaded scene's
        HIP_TRY(h, upload(ds.mats, mats.data(), mats.size() * sizeof(Mat<real>)));
        HIP_TRY(h, upload(ds.texs, texs.data(), texs.size() * sizeof(Tex<real>)));
        HIP_TRY(h, upload(ds.keys, keys.data(), keys.size() * sizeof(Key<real>)));
        ds.side_tables = true;
    }
    ds.desc_pos_valid = !in.any_lists && !spliced && !h->has_list_elements;
    if (ds.desc_pos_valid) {   // every object is one primitive: record i of leaf_prims is objs[b.order[i]]
        std::vector<int32_t> pos(h->prims.size(), -1);
        for (size_t i = 0; i < in.objs.size(); i++) pos[(size_t)in.objs[b.order[i]].desc] = (int32_t)i;
        HIP_TRY(h, upload(ds.desc_pos, pos.data(), pos.size() * sizeof(int32_t)));
    }
    ds.n_entries = (int32_t)b.entries.size(); ds.n_prims = (int32_t)lay.leaf_prims.size(); ds.n_mats = (int32_t)mats.size(); ds.n_texs = (int32_t)texs.size();
    ds.n_scene_keys = (int32_t)h->keys.size();
    ds.lds_bytes = scene_lds_bytes(ds);
    ds.animated = in.kinds.any_keys; ds.has_triangles = in.kinds.has_triangles; ds.has_spheres = in.kinds.has_spheres;
    return CR_OK;
}

template <typename real> int32_t build_dev_scene(CrHandle* h) {
    DevScene<real>& ds = dev_scene<real>(h);
    if (ds.built) return CR_OK;
    auto t_begin = std::chrono::steady_clock::now();
    const bool timing = getenv("CRUCIBLE_BUILD_TIMING") != nullptr;
    auto lap = [&](const char* what) { if (timing) fprintf(stderr, "[build] %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); };
    int32_t rc;
    // 1. objects and boxes
    SceneBoxes<real> in;
    scene_boxes(h->prims, h->bvh_mode == CR_BVH_REFERENCE, in);
    ds.ordered = h->bvh_mode == CR_BVH_SAH_ORDERED;
    lap("primitive records and boxes");
    // 2. topology, by the mode's builder
    const auto t_tree = std::chrono::steady_clock::now();
    std::vector<int8_t> axis;
    Spliced<real> spliced;
    bool device_boxes;
    SahDeviceStats dev_stats;
    rc = build_topology<real>(h, in, axis, ds.level_begin, spliced, device_boxes, dev_stats);
    if (rc != CR_OK) return rc;
    lap("tree");
    const double tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tree).count();
    // 3. leaf layout
    LeafLayout<real> lay;
    if (!layout_leaves(h->prims, in, spliced, lay)) return fail(h, CR_ERR_INVALID_ARG, "too many primitives");
    // 4. side tables, 5. uploads
    rc = upload_scene<real>(h, ds, in, lay, axis, spliced.on);
    if (rc != CR_OK) return rc;
    // 6. boxes and screen -- device builders: the construction-time primitive boxes, bottom-up, on the device; then the screening records
    rc = finish_boxes<real>(h, ds, in.b.entries, device_boxes, real(0), real(0), false);
    if (rc != CR_OK) return rc;
    lap("uploads and boxes");
    // 7. bookkeeping
    ds.leaf_desc = leaf_descs(in);
    ds.in_desc.resize(in.objs.size());
    for (size_t i = 0; i < in.objs.size(); i++) ds.in_desc[i] = in.objs[i].desc;
    ds.host_entries.swap(in.b.entries);
    ds.host_axis.swap(axis);
    ds.base_order.swap(in.b.order);
    frame_scene<real>(h).frame_valid = false;   // built from the tree this one replaces
    frame_scene<real>(h).info = CrBuildInfo();
    ds.last_walk = kWalkNone;
    ds.has_bvh_elements = spliced.on;
    ds.built = true;
    ds.info = build_info(h->bvh_mode, device_boxes, ds.n_entries, dev_stats, tree_ms, t_begin);
    h->upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return CR_OK;
}

// cr_export_bvh: the tree of tree.hpp's export_walk; what cannot be exported, and an array too small, are errors here.
template <typename real>
int32_t export_tree(CrHandle* h, const DevScene<real>& ds, const std::vector<Entry<real>>& E, const char* what, double* boxes, int32_t* children,
                    int32_t* split_axis, int32_t capacity, int32_t* n_out) {
    if (ds.has_bvh_elements) return fail(h, CR_ERR_UNSUPPORTED, std::string(what) + ": the scene holds a BVHWrapper element (CR_BVH_REFERENCE): its records are not two-children wrappers");
    *n_out = (int32_t)E.size();
    if (!boxes || !children || capacity < (int32_t)E.size()) return E.empty() || (!boxes && !children) ? CR_OK : fail(h, CR_ERR_INVALID_ARG, std::string(what) + ": capacity too small");
    if (!E.empty()) export_walk(E, ds.host_axis, ds.leaf_desc, ds.ordered, boxes, children, split_axis);
    return CR_OK;
}

template <typename real>
int32_t export_bvh(CrHandle* h, double* boxes, int32_t* children, int32_t* split_axis, int32_t capacity, int32_t* n_out) {
    int32_t rc = build_dev_scene<real>(h);
    if (rc != CR_OK) return rc;
    const DevScene<real>& ds = dev_scene<real>(h);
    return export_tree<real>(h, ds, ds.host_entries, "cr_export_bvh", boxes, children, split_axis, capacity, n_out);
}

// ---------------------------------------------------------------- CR_REFIT_REBUILD: the tree of one frame
// A second tree beside the base tree of a SAH mode: section 6.1's binned SAH over the visible primitives' motion boxes
// for the ray times [ta, tb] (prim_box_over, the box a refit gives a one-primitive leaf), with the wrapper boxes a refit
// derives for that topology.  The primitives, their order and the builders are build_dev_scene's; the records are gathered
// on the device from the base tree's, and materials, textures and keys are the base tree's own buffers.  Kept on the handle
// and reused while the interval stays the same.
template <typename real> int32_t build_frame_scene(CrHandle* h, real ta, real tb) {
    DevScene<real>& base = dev_scene<real>(h);
    DevScene<real>& fs = frame_scene<real>(h);
    if (fs.frame_valid && fs.frame_ta == ta && fs.frame_tb == tb) return CR_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    const int32_t n = base.n_prims;
    if (base.has_lists || base.has_bvh_elements || base.in_desc.size() != (size_t)n || base.base_order.size() != (size_t)n || n < 1)
        return fail(h, CR_ERR_UNSUPPORTED, "CR_REFIT_REBUILD: the base tree is not a SAH tree over single primitives");
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier render may still walk the frame tree this build overwrites
    fs.frame_valid = false; fs.built = false;
    fs.info = CrBuildInfo();
    alias_side_tables(fs, base);   // the side tables are the base tree's
    fs.ordered = base.ordered; fs.animated = base.animated; fs.has_triangles = base.has_triangles; fs.has_spheres = base.has_spheres;
    fs.has_leaf_runs = false; fs.has_lists = false; fs.has_bvh_elements = false; fs.desc_pos_valid = false;
    const bool on_device = h->bvh_device && n >= 3;   // fewer are one leaf, written on the host (as in build_dev_scene)
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    HIP_TRY(h, fs.frame_map.ensure((size_t)n * 2 * sizeof(int32_t)));
    int32_t* d_input_of = (int32_t*)fs.frame_map.p;
    int32_t* d_src = d_input_of + n;
    std::vector<real> bmin[3], bmax[3];
    const auto t_tree = std::chrono::steady_clock::now();
    if (on_device) {   // the motion boxes straight into the builder's input: no host pass over the primitives
        HIP_TRY(h, h->sah_work.box.ensure((size_t)n * 48));
        HIP_TRY(h, hipMemcpyAsync(d_input_of, base.base_order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL((motion_boxes_kernel<real>), grid, block, 0, h->stream, (const Prim<real>*)base.prims.p, (const int32_t*)d_input_of, n,
                           (const Key<real>*)base.keys.p, ta, tb, (double*)h->sah_work.box.p);
        HIP_TRY(h, hipGetLastError());
    } else motion_boxes<real>(h->prims, base.in_desc.data(), n, h->keys, ta, tb, bmin, bmax);   // the same rule on the host (CR_HD), from the handle's copy of the scene
    std::vector<int32_t> order((size_t)n);
    for (int32_t i = 0; i < n; i++) order[i] = i;
    std::vector<Entry<real>> entries;
    std::vector<int8_t> axis;
    SahDeviceStats dev_stats;
    int32_t rc = sah_tree<real>(h, bmin, bmax, n, on_device, true, order, entries, axis, fs.level_begin, dev_stats);
    if (rc != CR_OK) return rc;
    const double tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tree).count();
    // the records in the frame tree's leaf order: position i holds builder input order[i], which the base tree keeps at inv[order[i]]
    std::vector<int32_t> inv((size_t)n), src((size_t)n);
    for (int32_t i = 0; i < n; i++) inv[(size_t)base.base_order[i]] = i;
    for (int32_t i = 0; i < n; i++) src[i] = inv[(size_t)order[i]];
    HIP_TRY(h, hipMemcpyAsync(d_src, src.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, fs.prims.ensure((size_t)n * sizeof(Prim<real>)));
    hipLaunchKernelGGL((gather_prims_kernel<real>), grid, block, 0, h->stream, (const Prim<real>*)base.prims.p, (const int32_t*)d_src, n, (Prim<real>*)fs.prims.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // `src` and the base order were read from host vectors
    rc = upload_entries<real>(h, fs, entries, entries, axis);
    if (rc != CR_OK) return rc;
    fs.n_entries = (int32_t)entries.size(); fs.n_prims = n;
    fs.lds_bytes = scene_lds_bytes(fs);
    // the boxes a refit gives this topology for [ta, tb], on the device for either builder; then the screening records
    rc = finish_boxes<real>(h, fs, entries, true, ta, tb, true);
    if (rc != CR_OK) return rc;
    fs.host_entries.swap(entries);
    fs.host_axis.swap(axis);
    fs.leaf_desc.resize(n);
    for (int32_t i = 0; i < n; i++) fs.leaf_desc[i] = base.in_desc[(size_t)order[i]];
    fs.built = true;
    fs.frame_valid = true; fs.frame_ta = ta; fs.frame_tb = tb;
    fs.info = build_info(h->bvh_mode, on_device, fs.n_entries, dev_stats, tree_ms, t_begin);
    return CR_OK;
}

template <typename real> int32_t select_tree(CrHandle* h, const CrRenderParams* p, bool batch, DevScene<real>** walk, bool* refit) {
    const bool rebuild = p->refit_boxes == CR_REFIT_REBUILD;
    if (rebuild && h->bvh_mode != CR_BVH_SAH && h->bvh_mode != CR_BVH_SAH_ORDERED)
        return fail(h, CR_ERR_UNSUPPORTED, "CR_REFIT_REBUILD builds the binned-SAH tree of the frame: it needs a scene uploaded with CR_BVH_SAH or CR_BVH_SAH_ORDERED");
    int32_t rc = build_dev_scene<real>(h);
    if (rc != CR_OK) return rc;
    DevScene<real>& ds = dev_scene<real>(h);
    *walk = &ds;
    // without primitive keys the boxes would not change -- unless a HitList element's box is not its objects' union
    *refit = p->refit_boxes && (ds.animated || ds.has_lists) && ds.n_entries > 0;
    if (!rebuild || !*refit || batch) return CR_OK;   // (a batch with a refit of either kind is refused by its caller)
    real ta, shutter;
    frame_times(p, ta, shutter);
    rc = build_frame_scene<real>(h, ta, ta + shutter);
    if (rc != CR_OK) return rc;
    *walk = &frame_scene<real>(h);
    *refit = false;   // its boxes are this frame's already
    return CR_OK;
}

// cr_export_render_bvh: the tree the last render or guide pass of this precision walked, with the boxes it walked
template <typename real>
int32_t export_render_bvh(CrHandle* h, double* boxes, int32_t* children, int32_t* split_axis, int32_t capacity, int32_t* n_out) {
    DevScene<real>& ds = dev_scene<real>(h);
    const char* what = "cr_export_render_bvh";
    if (!ds.built || ds.last_walk == kWalkNone) return fail(h, CR_ERR_NO_SCENE, "cr_export_render_bvh before a render of this precision");
    if (ds.last_walk == kWalkFrame) {
        const DevScene<real>& fs = frame_scene<real>(h);
        if (!fs.frame_valid) return fail(h, CR_ERR_NO_SCENE, "cr_export_render_bvh before a render of this precision");
        return export_tree<real>(h, fs, fs.host_entries, what, boxes, children, split_axis, capacity, n_out);
    }
    if (ds.last_walk == kWalkBase || !boxes || !children || capacity < ds.n_entries || ds.host_entries.size() != (size_t)ds.n_entries)
        return export_tree<real>(h, ds, ds.host_entries, what, boxes, children, split_axis, capacity, n_out);
    // the base topology with the refitted boxes, which live on the device (entries_refit) until the next refit overwrites them
    std::vector<Entry<real>> E = ds.host_entries;
    const size_t rec = ds.entry_bytes;
    std::vector<char> raw((size_t)ds.n_entries * rec);
    HIP_TRY(h, hipMemcpyAsync(raw.data(), ds.entries_refit.p, raw.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < E.size(); i++) memcpy(E[i].b, raw.data() + i * rec, 6 * sizeof(real));   // Entry and EntryO both begin with the box
    return export_tree<real>(h, ds, E, what, boxes, children, split_axis, capacity, n_out);
}

template int32_t build_dev_scene<float>(CrHandle*);
template int32_t build_dev_scene<double>(CrHandle*);
template int32_t select_tree<float>(CrHandle*, const CrRenderParams*, bool, DevScene<float>**, bool*);
template int32_t select_tree<double>(CrHandle*, const CrRenderParams*, bool, DevScene<double>**, bool*);

}   // namespace cr

using namespace cr;

extern "C" int32_t cr_build_info(CrHandle* h, int32_t real_type, CrBuildInfo* out) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!out) return fail(h, CR_ERR_INVALID_ARG, "cr_build_info: null out");
    if (real_type != CR_REAL_F32 && real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_build_info before cr_upload_scene");
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t rc = real_type == CR_REAL_F64 ? build_dev_scene<double>(h) : build_dev_scene<float>(h);
    if (rc != CR_OK) return rc;
    *out = real_type == CR_REAL_F64 ? h->s64.info : h->s32.info;
    return CR_OK;
}

extern "C" int32_t cr_frame_build_info(CrHandle* h, int32_t real_type, CrBuildInfo* out) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!out) return fail(h, CR_ERR_INVALID_ARG, "cr_frame_build_info: null out");
    if (real_type != CR_REAL_F32 && real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_frame_build_info before cr_upload_scene");
    *out = real_type == CR_REAL_F64 ? h->f64.info : h->f32.info;   // all zero while no frame tree exists
    return CR_OK;
}

extern "C" int32_t cr_export_render_bvh(CrHandle* h, int32_t real_type, double* boxes, int32_t* children, int32_t* split_axis, int32_t capacity,
                             int32_t* n_wrappers) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!n_wrappers) return fail(h, CR_ERR_INVALID_ARG, "cr_export_render_bvh: null n_wrappers");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_export_render_bvh before cr_upload_scene");
    if (real_type != CR_REAL_F32 && real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    HIP_TRY(h, hipSetDevice(h->device));
    return real_type == CR_REAL_F64 ? export_render_bvh<double>(h, boxes, children, split_axis, capacity, n_wrappers)
                                    : export_render_bvh<float>(h, boxes, children, split_axis, capacity, n_wrappers);
}

extern "C" int32_t cr_export_bvh(CrHandle* h, int32_t real_type, double* boxes, int32_t* children, int32_t* split_axis, int32_t capacity,
                      int32_t* n_wrappers) {
    if (!h) return CR_ERR_INVALID_ARG;
    if (!n_wrappers) return fail(h, CR_ERR_INVALID_ARG, "cr_export_bvh: null n_wrappers");
    if (!h->has_scene) return fail(h, CR_ERR_NO_SCENE, "cr_export_bvh before cr_upload_scene");
    if (real_type != CR_REAL_F32 && real_type != CR_REAL_F64) return fail(h, CR_ERR_INVALID_ARG, "unknown real_type");
    HIP_TRY(h, hipSetDevice(h->device));
    return real_type == CR_REAL_F64 ? export_bvh<double>(h, boxes, children, split_axis, capacity, n_wrappers)
                                    : export_bvh<float>(h, boxes, children, split_axis, capacity, n_wrappers);
}
