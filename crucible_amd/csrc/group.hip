// group.hip -- cr_group_*: several devices behind one call (group.hpp has the RCCL table, the kernels and CrGroup).
#include "handle.hpp"

using namespace cr;

#include "group.hpp"

extern "C" {

int32_t cr_group_shard(int32_t samples, int32_t member, int32_t n_members, int32_t* begin, int32_t* count) {
    if (samples < 0 || n_members < 1 || member < 0 || member >= n_members || !begin || !count) return CR_ERR_INVALID_ARG;
    const int64_t b = (int64_t)member * samples / n_members, e = (int64_t)(member + 1) * samples / n_members;
    *begin = (int32_t)b; *count = (int32_t)(e - b);
    return CR_OK;
}

int32_t cr_group_create(const int32_t* device_ids, int32_t n_devices, CrGroup** out) {
    if (!out) return gfail(nullptr, CR_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!device_ids || n_devices < 1) return gfail(nullptr, CR_ERR_INVALID_ARG, "device list is empty");
    // CRUCIBLE_GROUP_SAME_DEVICE=1 (tests on a one-GPU box): the members may share a device; their sums are then added
    // by a plain kernel instead of RCCL, which refuses two ranks on one device.  Everything else is the real path.
    const bool same_device = getenv("CRUCIBLE_GROUP_SAME_DEVICE") != nullptr;
    for (int i = 0; i < n_devices; i++) for (int j = 0; j < i; j++)
        if (device_ids[i] == device_ids[j] && !same_device) return gfail(nullptr, CR_ERR_INVALID_ARG, "a device appears twice in the list");
    DeviceGuard guard;
    CrGroup* g = new CrGroup();
    g->same_device_sum = same_device && n_devices > 1;
    g->world = n_devices; g->first = 0;
    g->members.assign((size_t)n_devices, nullptr);
    g->partial.resize((size_t)n_devices);
    g->flags.resize((size_t)n_devices);
    g->status.resize((size_t)n_devices);
    for (int i = 0; i < n_devices; i++) {
        int32_t rc = cr_create(device_ids[i], &g->members[(size_t)i]);
        if (rc != CR_OK) { g_group_create_error = cr_last_error(nullptr); group_free(g); return rc; }
    }
    const bool force = getenv("CRUCIBLE_GROUP_FORCE_RCCL") != nullptr;   // tests: exercise the collective on one device
    if ((n_devices > 1 || force) && !g->same_device_sum) {
        RcclApi& api = rccl_api();
        if (!api.lib) { g_group_create_error = api.error; group_free(g); return CR_ERR_UNSUPPORTED; }
        g->comms.assign((size_t)n_devices, nullptr);
        ncclResult_t r = api.CommInitAll(g->comms.data(), n_devices, device_ids);
        if (r != ncclSuccess) { g_group_create_error = std::string("ncclCommInitAll: ") + api.GetErrorString(r); g->comms.clear(); group_free(g); return CR_ERR_HIP; }
    }
    (void)hipSetDevice(g->members[0]->device);
    if (g->ev0.create() != hipSuccess || g->ev1.create() != hipSuccess) { g_group_create_error = "hipEventCreate failed"; group_free(g); return CR_ERR_HIP; }
    *out = g;
    return CR_OK;
}

int32_t cr_group_unique_id(uint8_t id[CR_GROUP_ID_BYTES]) {
    static_assert(CR_GROUP_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id) return gfail(nullptr, CR_ERR_INVALID_ARG, "id is null");
    RcclApi& api = rccl_api();
    if (!api.lib) return gfail(nullptr, CR_ERR_UNSUPPORTED, api.error);
    ncclUniqueId u;
    ncclResult_t r = api.GetUniqueId(&u);
    if (r != ncclSuccess) return gfail(nullptr, CR_ERR_HIP, std::string("ncclGetUniqueId: ") + api.GetErrorString(r));
    memcpy(id, u.internal, CR_GROUP_ID_BYTES);
    return CR_OK;
}

int32_t cr_group_create_rank(int32_t device_id, int32_t rank, int32_t world_size, const uint8_t id[CR_GROUP_ID_BYTES], CrGroup** out) {
    if (!out) return gfail(nullptr, CR_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (world_size < 1 || rank < 0 || rank >= world_size) return gfail(nullptr, CR_ERR_INVALID_ARG, "rank outside [0, world_size)");
    if (world_size > 1 && !id) return gfail(nullptr, CR_ERR_INVALID_ARG, "id is null");
    DeviceGuard guard;
    CrGroup* g = new CrGroup();
    g->world = world_size; g->first = rank;
    g->members.assign(1, nullptr);
    g->partial.resize(1);
    g->flags.resize(1);
    g->status.resize(1);
    int32_t rc = cr_create(device_id, &g->members[0]);
    if (rc != CR_OK) { g_group_create_error = cr_last_error(nullptr); group_free(g); return rc; }
    const bool force = getenv("CRUCIBLE_GROUP_FORCE_RCCL") != nullptr && id;
    if (world_size > 1 || force) {
        RcclApi& api = rccl_api();
        if (!api.lib) { g_group_create_error = api.error; group_free(g); return CR_ERR_UNSUPPORTED; }
        ncclUniqueId u;
        memcpy(u.internal, id, CR_GROUP_ID_BYTES);
        g->comms.assign(1, nullptr);
        (void)hipSetDevice(device_id);
        ncclResult_t r = api.CommInitRank(&g->comms[0], world_size, u, rank);
        if (r != ncclSuccess) { g_group_create_error = std::string("ncclCommInitRank: ") + api.GetErrorString(r); g->comms.clear(); group_free(g); return CR_ERR_HIP; }
    }
    (void)hipSetDevice(device_id);
    if (g->ev0.create() != hipSuccess || g->ev1.create() != hipSuccess) { g_group_create_error = "hipEventCreate failed"; group_free(g); return CR_ERR_HIP; }
    *out = g;
    return CR_OK;
}

void cr_group_destroy(CrGroup* g) { DeviceGuard guard; group_free(g); }
int32_t cr_group_local_size(CrGroup* g) { return g ? (int32_t)g->members.size() : 0; }
int32_t cr_group_size(CrGroup* g) { return g ? g->world : 0; }
int32_t cr_group_rank(CrGroup* g) { return g ? g->first : -1; }
CrHandle* cr_group_handle(CrGroup* g, int32_t i) { return (g && i >= 0 && i < (int32_t)g->members.size()) ? g->members[(size_t)i] : nullptr; }
const char* cr_group_last_error(CrGroup* g) { return g ? g->error.c_str() : g_group_create_error.c_str(); }

int32_t cr_group_upload_scene(CrGroup* g, const CrSceneDesc* scene) {
    if (!g) return CR_ERR_INVALID_ARG;
    DeviceGuard guard;
    for (CrHandle* h : g->members) {
        int32_t rc = cr_upload_scene(h, scene);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    return CR_OK;
}

int32_t cr_group_update_primitives(CrGroup* g, const int32_t* prim_index, const double* v, int32_t n, int32_t flags) {
    if (!g) return CR_ERR_INVALID_ARG;
    DeviceGuard guard;
    for (CrHandle* h : g->members) {   // every member is validated before any is changed
        int32_t rc = validate_update(h, prim_index, v, n, flags);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    for (CrHandle* h : g->members) {
        int32_t rc = apply_update(h, prim_index, v, n, flags);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    return CR_OK;
}

int32_t cr_group_update_materials(CrGroup* g, const CrMaterial* materials, int32_t n_materials, const CrTexture* textures, int32_t n_textures,
                                  const int32_t* prim_index, const int32_t* prim_material, int32_t n_assign) {
    if (!g) return CR_ERR_INVALID_ARG;
    DeviceGuard guard;
    for (CrHandle* h : g->members) {   // every member is validated before any is changed
        int32_t rc = validate_materials(h, materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    for (CrHandle* h : g->members) {
        int32_t rc = apply_materials(h, materials, n_materials, textures, n_textures, prim_index, prim_material, n_assign);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    return CR_OK;
}

int32_t cr_group_update_image(CrGroup* g, int32_t image, int32_t x0, int32_t y0, int32_t width, int32_t height, const uint8_t* rgb8) {
    if (!g) return CR_ERR_INVALID_ARG;
    DeviceGuard guard;
    for (CrHandle* h : g->members) {
        int32_t rc = validate_image(h, image, x0, y0, width, height, rgb8);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    for (CrHandle* h : g->members) {
        int32_t rc = apply_image(h, image, x0, y0, width, height, rgb8);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    return CR_OK;
}

int32_t cr_group_set_sky(CrGroup* g, int32_t sky_kind, int32_t sky_image) {
    if (!g) return CR_ERR_INVALID_ARG;
    for (CrHandle* h : g->members) {
        int32_t rc = validate_sky(h, sky_kind, sky_image);
        if (rc != CR_OK) return gfail(g, rc, h->error);
    }
    for (CrHandle* h : g->members) apply_sky(h, sky_kind, sky_image);
    return CR_OK;
}

// Failure handling.  Nothing is launched before every local member's arguments have been validated and its buffers exist,
// so bad arguments fail the same way on every rank.  A member that fails later (its render, an allocation) does NOT leave:
// with a collective, every member first takes part in a 4-byte ncclAllReduce(min) of "my render is fine" on the render's own
// stream, and only a unanimous 1 goes on to the ncclReduce -- otherwise every rank returns an error (its own, or
// CR_ERR_PEER) and the communicator is still consistent.  Only a failing collective call itself poisons the group
// (its communicators are aborted; every later call answers CR_ERR_PEER): peers inside that collective cannot be told.
// pre_rc / pre_msg: a failure this rank met before the call (cr_group_render_host's root-side buffer); it takes part
// in the agreement like a failed render, so the other ranks are not left waiting.
static int32_t group_render_impl(CrGroup* g, const CrCameraDesc* cam, const CrRenderParams* params, void* d_out, CrGroupStats* stats,
                                 int32_t pre_rc, const char* pre_msg) {
    if (!g) return CR_ERR_INVALID_ARG;
    if (g->poisoned) return gfail(g, CR_ERR_PEER, "an earlier collective of this group failed: destroy it and create a new one");
    if (!cam || !params) return gfail(g, CR_ERR_INVALID_ARG, "null camera or params");   // the same on every rank
    const bool root_here = g->first == 0;
    DeviceGuard guard;   // the caller's current device is the caller's again on every way out
    const bool collective = !g->comms.empty();
    const bool summed = g->world > 1 || collective;
    const int local = (int)g->members.size();
    std::vector<CrRenderParams> ps((size_t)local, *params);
    // 0. arguments and buffers, before anything is launched
    int32_t local_rc = CR_OK;
    std::string local_err;
    auto note = [&](int32_t rc, const std::string& msg) { if (local_rc == CR_OK && rc != CR_OK) { local_rc = rc; local_err = msg; } };
    if (pre_rc != CR_OK) note(pre_rc, pre_msg ? pre_msg : "");
    if (root_here && !d_out) note(CR_ERR_INVALID_ARG, "the root member needs an output buffer");
    for (int i = 0; i < local; i++) {
        CrHandle* h = g->members[(size_t)i];
        int32_t rc = validate_render(h, cam, params);
        if (rc != CR_OK) { note(rc, h->error); continue; }
        if (cr_group_shard(params->samples, g->first + i, g->world, &ps[(size_t)i].sample_begin, &ps[(size_t)i].sample_count) != CR_OK) note(CR_ERR_INVALID_ARG, "samples must be >= 0");
    }
    // relaxed sums reduce exactly: the members export fixed-point words at the frame's scale, the group adds integers
    // and the root finalizes them as cr_render_device does -- the frame of any member count is the one-device frame
    const bool exact = summed && resolve_sum_order(g->members[0], params) == CR_SUM_RELAXED;
    for (CrRenderParams& p : ps) p.output_sum = exact ? CR_OUTPUT_FIXED_SUM : (summed ? 1 : 0);   // one member, no collective: exactly cr_render_device
    const size_t n = local_rc == CR_OK ? (size_t)cam->image_width * (size_t)cam->image_height * 3 : 0;
    const bool f64 = params->real_type == CR_REAL_F64;
    const size_t bytes = n * (exact ? sizeof(unsigned long long) : (f64 ? sizeof(double) : sizeof(float)));
    if (summed) for (int i = 0; i < local && local_rc == CR_OK; i++) {
        CrHandle* h = g->members[(size_t)i];
        if (hipSetDevice(h->device) != hipSuccess || g->partial[(size_t)i].ensure(bytes) != hipSuccess ||
            (collective && exact && g->flags[(size_t)i].ensure(n) != hipSuccess) ||
            (collective && g->status[(size_t)i].ensure(kStatusWords * sizeof(int32_t)) != hipSuccess)) { (void)hipGetLastError(); note(CR_ERR_HIP, "cannot allocate a member's buffer of per-pixel sums"); }
    }
    // 1. every local member renders its shard, asynchronously on its own stream
    const char* fail_member = getenv("CRUCIBLE_GROUP_FAIL_MEMBER");   // tests: this member's render reports a failure after it was launched
    for (int i = 0; i < local && local_rc == CR_OK; i++) {
        CrHandle* h = g->members[(size_t)i];
        h->keep_counters = stats != nullptr;   // member_stats reads them once the stream is idle (a render without stats keeps none)
        int32_t rc = cr_render_device(h, cam, &ps[(size_t)i], summed ? g->partial[(size_t)i].p : d_out, nullptr);
        h->keep_counters = false;
        if (rc == CR_OK && fail_member && atoi(fail_member) == g->first + i) rc = fail(h, CR_ERR_HIP, "render failure injected by CRUCIBLE_GROUP_FAIL_MEMBER");
        if (rc != CR_OK) note(rc, h->error);
    }
    // a collective call that fails leaves peers behind inside it: nothing more can be agreed on through these communicators
    auto poison = [&](const std::string& what) {
        g->poisoned = true;
        RcclApi& api = rccl_api();
        for (size_t i = 0; i < g->comms.size(); i++) if (g->comms[i]) { (void)hipSetDevice(g->members[i]->device); if (api.CommAbort) (void)api.CommAbort(g->comms[i]); g->comms[i] = nullptr; }
        for (CrHandle* h : g->members) { (void)hipSetDevice(h->device); (void)hipStreamSynchronize(h->stream); }
        return gfail(g, CR_ERR_HIP, what);
    };
    // 2. do all members of the whole group stand?  (min over "1 = fine")  And do they all reduce the same kind of sums?
    //    (min over exact and over -exact: equal kinds iff the two minima are opposite)
    bool all_fine = local_rc == CR_OK, same_kind = true;
    if (collective) {
        RcclApi& api = rccl_api();
        const int32_t mine[kStatusWords] = {local_rc == CR_OK ? 1 : 0, exact ? 1 : 0, exact ? -1 : 0};
        bool ok = true;
        for (int i = 0; i < local && ok; i++) {
            CrHandle* h = g->members[(size_t)i];
            ok = hipSetDevice(h->device) == hipSuccess && g->status[(size_t)i].ensure(sizeof mine) == hipSuccess &&
                 hipMemcpyAsync(g->status[(size_t)i].p, mine, sizeof mine, hipMemcpyHostToDevice, h->stream) == hipSuccess;
        }
        if (!ok) return poison("cannot stage the group's status word");
        ncclResult_t r = api.GroupStart();
        for (int i = 0; i < local && r == ncclSuccess; i++) {
            CrHandle* h = g->members[(size_t)i];
            (void)hipSetDevice(h->device);
            r = api.AllReduce(g->status[(size_t)i].p, g->status[(size_t)i].p, kStatusWords, ncclInt32, ncclMin, g->comms[(size_t)i], h->stream);
        }
        if (r == ncclSuccess) r = api.GroupEnd(); else (void)api.GroupEnd();
        if (r != ncclSuccess) return poison(std::string("ncclAllReduce of the status word: ") + api.GetErrorString(r));
        int32_t agreed = 1;
        for (int i = 0; i < local; i++) {
            CrHandle* h = g->members[(size_t)i];
            int32_t v[kStatusWords] = {0, 0, 0};
            if (hipSetDevice(h->device) != hipSuccess || hipMemcpyAsync(v, g->status[(size_t)i].p, sizeof v, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess) return poison("cannot read the group's status word");
            agreed = std::min(agreed, v[0]);
            same_kind = same_kind && v[1] == -v[2];
        }
        all_fine = agreed == 1 && same_kind;
    }
    if (!all_fine) {   // every rank is here: wait for what was launched and report
        for (CrHandle* h : g->members) { (void)hipSetDevice(h->device); (void)hipStreamSynchronize(h->stream); }
        if (local_rc != CR_OK) return gfail(g, local_rc, local_err);
        if (!same_kind) return gfail(g, CR_ERR_INVALID_ARG, "the ranks of the group resolve different summation orders (sum_order, CRUCIBLE_SUM_ORDER); nothing was reduced");
        return gfail(g, CR_ERR_PEER, "another member of the group failed its render; nothing was reduced");
    }
    // 3. one reduce of the sums to the root, then the divide there
    if (summed) {
        CrHandle* root = g->members[0];
        if (root_here) { GHIP_TRY(g, hipSetDevice(root->device)); GHIP_TRY(g, hipEventRecord(g->ev0, root->stream)); }
        if (g->same_device_sum) {   // every member is on the root's device: wait for their renders, then add in member order
            for (int i = 1; i < local; i++) GHIP_TRY(g, hipStreamSynchronize(g->members[(size_t)i]->stream));
            const unsigned grid = (unsigned)((n + 255) / 256);
            for (int i = 1; i < local; i++) {
                if (exact) hipLaunchKernelGGL(group_fx_add_kernel, dim3(grid), dim3(256), 0, root->stream, (unsigned long long*)g->partial[0].p, (const unsigned long long*)g->partial[(size_t)i].p, n);
                else if (f64) hipLaunchKernelGGL((group_add_kernel<double>), dim3(grid), dim3(256), 0, root->stream, (double*)g->partial[0].p, (const double*)g->partial[(size_t)i].p, n);
                else hipLaunchKernelGGL((group_add_kernel<float>), dim3(grid), dim3(256), 0, root->stream, (float*)g->partial[0].p, (const float*)g->partial[(size_t)i].p, n);
            }
            GHIP_TRY(g, hipGetLastError());
        }
        if (collective) {
            RcclApi& api = rccl_api();
            if (exact) for (int i = 0; i < local; i++) {   // on each member's stream, behind its render
                CrHandle* h = g->members[(size_t)i];
                GHIP_TRY(g, hipSetDevice(h->device));
                hipLaunchKernelGGL(group_fx_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                                   (unsigned long long*)g->partial[(size_t)i].p, (uint8_t*)g->flags[(size_t)i].p, n);
                GHIP_TRY(g, hipGetLastError());
            }
            const ncclDataType_t dt = exact ? ncclUint64 : (f64 ? ncclDouble : ncclFloat);
            ncclResult_t r = api.GroupStart();
            for (int i = 0; i < local && r == ncclSuccess; i++) {
                CrHandle* h = g->members[(size_t)i];
                (void)hipSetDevice(h->device);
                void* buf = g->partial[(size_t)i].p;   // in place on the root
                r = api.Reduce(buf, buf, n, dt, ncclSum, 0, g->comms[(size_t)i], h->stream);
                if (exact && r == ncclSuccess) r = api.Reduce(g->flags[(size_t)i].p, g->flags[(size_t)i].p, n, ncclUint8, ncclMax, 0, g->comms[(size_t)i], h->stream);
            }
            if (r == ncclSuccess) r = api.GroupEnd(); else (void)api.GroupEnd();
            if (r != ncclSuccess) return poison(std::string("ncclReduce: ") + api.GetErrorString(r));
        }
        if (root_here) {
            GHIP_TRY(g, hipSetDevice(root->device));
            const unsigned grid = (unsigned)((n + 255) / 256);
            if (exact) {
                unsigned long long* sums = (unsigned long long*)g->partial[0].p;
                if (collective) hipLaunchKernelGGL(group_fx_merge_kernel, dim3(grid), dim3(256), 0, root->stream, sums, (const uint8_t*)g->flags[0].p, n);
                GHIP_TRY(g, hipGetLastError());
                if (fixed_sums_to_rgb(root, sums, n, params->samples, f64, d_out) != CR_OK) return gfail(g, CR_ERR_HIP, root->error);
            } else if (f64) hipLaunchKernelGGL((group_mean_kernel<double>), dim3(grid), dim3(256), 0, root->stream, (const double*)g->partial[0].p, (double*)d_out, n, (double)params->samples);
            else hipLaunchKernelGGL((group_mean_kernel<float>), dim3(grid), dim3(256), 0, root->stream, (const float*)g->partial[0].p, (float*)d_out, n, (float)params->samples);
            GHIP_TRY(g, hipGetLastError());
            GHIP_TRY(g, hipEventRecord(g->ev1, root->stream));
        }
    }
    // 4. wait for every local stream; a queue-pipeline wave that gave up leaves an incomplete image behind
    for (CrHandle* h : g->members) { GHIP_TRY(g, hipSetDevice(h->device)); GHIP_TRY(g, hipStreamSynchronize(h->stream)); }
    for (CrHandle* h : g->members) { int32_t rc = check_queue_abort(h); if (rc != CR_OK) return gfail(g, rc, h->error); }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->members = g->world; stats->used_rccl = collective ? 1 : 0;
        const int64_t npix = (int64_t)cam->image_width * cam->image_height;
        for (int i = 0; i < local; i++) {
            CrStats s;
            int32_t rc = member_stats(g->members[(size_t)i], npix * ps[(size_t)i].sample_count, &s);
            if (rc != CR_OK) return gfail(g, rc, g->members[(size_t)i]->error);
            stats->render.samples += s.samples; stats->render.segments += s.segments; stats->render.node_tests += s.node_tests;
            stats->render.prim_tests += s.prim_tests; stats->render.texel_fetches += s.texel_fetches;
            stats->render.kernel_ms = std::max(stats->render.kernel_ms, s.kernel_ms);
            stats->render.upload_ms = std::max(stats->render.upload_ms, s.upload_ms);
        }
        if (root_here && summed) {
            float ms = 0;
            GHIP_TRY(g, hipSetDevice(g->members[0]->device));
            GHIP_TRY(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
            stats->reduce_ms = ms;
        }
    }
    return CR_OK;
}

int32_t cr_group_render(CrGroup* g, const CrCameraDesc* cam, const CrRenderParams* params, void* d_out, CrGroupStats* stats) {
    return group_render_impl(g, cam, params, d_out, stats, CR_OK, nullptr);
}

int32_t cr_group_render_host(CrGroup* g, const CrCameraDesc* cam, const CrRenderParams* params, void* h_out, CrGroupStats* stats) {
    if (!g) return CR_ERR_INVALID_ARG;
    if (!cam || !params) return gfail(g, CR_ERR_INVALID_ARG, "null camera or params");
    DeviceGuard guard;
    const bool root_here = g->first == 0;
    CrHandle* root = g->members[0];
    const bool sized = cam->image_width >= 1 && cam->image_height >= 1;
    const size_t n = sized ? (size_t)cam->image_width * (size_t)cam->image_height * 3 : 0;
    const size_t bytes = n * real_size(params->real_type);
    void* d_out = nullptr;
    // what only the root can get wrong goes into the agreement step, so the other ranks are not left in the collective
    int32_t pre_rc = CR_OK;
    const char* pre_msg = nullptr;
    if (root_here && !h_out) { pre_rc = CR_ERR_INVALID_ARG; pre_msg = "the root member needs an output buffer"; }
    else if (root_here && sized) {
        if (hipSetDevice(root->device) != hipSuccess || root->out_buf.ensure(bytes) != hipSuccess) { (void)hipGetLastError(); pre_rc = CR_ERR_HIP; pre_msg = "cannot allocate the root's output buffer"; }
        d_out = root->out_buf.p;
    }
    CrGroupStats local;
    int32_t rc = group_render_impl(g, cam, params, d_out, stats ? stats : &local, pre_rc, pre_msg);
    if (rc != CR_OK || !root_here) return rc;
    GHIP_TRY(g, hipSetDevice(root->device));
    GHIP_TRY(g, hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, root->stream));
    GHIP_TRY(g, hipStreamSynchronize(root->stream));
    const uint64_t bad = bad_pixels(h_out, params->real_type, n / 3);   // Color::new asserts 0 <= c <= 1 on every mean (ray_casting.rs:172)
    if (stats) stats->render.nan_pixels = bad;
    if (bad) return gfail(g, CR_ERR_NAN, "a pixel mean is NaN or outside [0,1] (the reference panics in Color::new)");
    return CR_OK;
}

}   // extern "C"
