// aov_kernel.hpp -- the guide pass's first-hit kernels for gfx950 and their launch: made of the megakernel's parts
// (pathtrace.hpp: camera_ray, walk_begin / walk_round, CR_CHECKER_LEAF, image_lookup, shade's sky) around a much
// smaller body -- a primary ray per work item, its closest hit, four values, no path state.  Included by aov_f32.hip
// and aov_f64.hip, each of which instantiates aov_ladder for its precision, and by aov_counts_f32.hip and aov_counts_f64.hip,
// which instantiate aov_counts_ladder (the kernels at a count plane), so no kernel is emitted twice.  Which
// kernel runs -- the scene's residency, screening records or wrappers -- is residency.hpp's rule, the render's own; how
// a pass is cut into units and launches is launch_plan.hpp's, and aov_launch keeps the HIP calls.
#pragma once
#include "aov.hpp"
#include "pathtrace.hpp"

#include <type_traits>

namespace cr {

#if defined(__HIPCC__)

// rint(x * 2^S) as a signed word (x * 2^S is exact: a power of two scales); false for a value that is not finite or
// whose word would not leave room for a sum
CR_D bool aov_word(double x, double scale, long long& v) {
    const double y = __builtin_rint(x * scale);
    if (!(__builtin_fabs(y) < 0x1.0p62)) return false;
    v = (long long)y;
    return true;
}

// BATCH: the kernels of cr_render_aov_frames_* -- the units of G.n_frames frames in one launch, frame after frame.  A unit
// lies in one frame, so all that depends on the frame (its first ray time, its accumulators and flags) is wave-uniform;
// pixels, tiles and the RNG key stay the frame's own.  The single-frame kernels do not carry the arithmetic.
// The BATCH kernels also render a region (cr_render_aov_region_*, as a batch of one frame): their tiles are anchored at
// (k.reg_x0, k.reg_y0), the accumulators and flags hold k.reg_w x k.reg_h pixels per frame, and camera_ray alone sees the
// frame's own pixel.  A whole frame is the region (0, 0, W, H).
// COUNTS (with BATCH only): the kernels of cr_render_aov_counts_* -- pixel p takes the samples [0, n_p), n_p its clamped
// value of the plane G.counts (aov_counts.hpp has the rules).  A unit reads its tile's sixteen counts, the wave forms
// their maximum as a scalar, and the group loop ends where that maximum ends: whole rounds disappear, not only lanes.
// VIEWS (with BATCH only): the kernels of cr_render_aov_views_* -- frame f of the batch is a view whose camera record is
// A.views[f] (KernelArgs::views), wave-uniform like everything else of the frame.
template <typename real, int RES, bool ANIM, bool ORD, bool SCREEN, bool BATCH, bool COUNTS = false, bool VIEWS = false>
CR_D void aov_body(const AovArgs<real>& G) {
    static_assert(BATCH || !COUNTS, "the COUNTS kernels are BATCH kernels");
    static_assert(BATCH || !VIEWS, "the VIEWS kernels are BATCH kernels");
    const KernelArgs<real>& A = G.k;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // (the waves' slots behind the scene)
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
    const CamConst<real>& cam = A.cam;
    const int32_t n_entries = A.n_entries;
    // this wave's slot: the words of one tile, emptied by every flush
    unsigned long long* slot = (unsigned long long*)(smem + G.acc_lds_off) + (size_t)(threadIdx.x >> 6) * kAovSlotWords;
    for (uint32_t k = lane; k < kAovSlotWords; k += 64) slot[k] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    auto slot_word = [&](uint32_t k) { return (__attribute__((address_space(3))) unsigned long long*)(slot + k); };

    uint32_t c_seg = 0, c_prim = 0, c_tex = 0;
    unsigned long long c_node = 0;
    const bool want_albedo = (G.layers & CR_AOV_ALBEDO) != 0, want_normal = (G.layers & CR_AOV_NORMAL) != 0;
    const bool want_depth = (G.layers & CR_AOV_DEPTH) != 0, want_cover = (G.layers & CR_AOV_COVERAGE) != 0;
    const double fxs = A.fx_scale;

    for (;;) {
        uint32_t wu = 0;
        if (lane == 0) wu = atomicAdd(A.work_counter, 1u);
        wu = (uint32_t)__builtin_amdgcn_readfirstlane((int)wu);
        if (wu >= G.n_units) break;
        const uint32_t unit_tile = wu / G.unit_chunks, chunk = wu - unit_tile * G.unit_chunks;
        // BATCH: the unit's frame and what goes with it, from wu alone (scalar registers); `tile` is the frame's own
        const uint32_t frame = BATCH ? unit_tile / G.frame_tiles : 0u;
        const uint32_t tile = BATCH ? unit_tile - frame * G.frame_tiles : unit_tile;
        const size_t frame_pix = BATCH ? (size_t)frame * ((size_t)A.reg_w * (size_t)A.reg_h) : 0;   // the frame's first pixel in the batch's planes
        const real frame_time = BATCH ? G.frame_times[frame] : real(0);
        const uint32_t g0 = chunk * G.unit_groups, g1 = g0 + G.unit_groups < G.groups ? g0 + G.unit_groups : G.groups;
        const uint32_t px = lane & 15u;
        uint32_t tile_x, tile_y;   // (scalars, like the tile)
        tile_xy(A, tile, tile_x, tile_y);
        const uint32_t pix_i = (tile_x << 2) + (px & 3u), pix_j = (tile_y << 2) + (px >> 2);
        // BATCH: inside the region, and the frame's own pixel for camera_ray (one integer each)
        const bool in_image = BATCH ? pix_i < A.reg_w && pix_j < A.reg_h : pix_i < (uint32_t)cam.W && pix_j < (uint32_t)cam.H;
        const uint32_t cam_i = BATCH ? A.reg_x0 + pix_i : pix_i, cam_j = BATCH ? A.reg_y0 + pix_j : pix_j;
        // COUNTS: the pixel's count (sixteen addresses per tile, inside the region only) and the tile's largest, a scalar
        uint32_t n_p = 0, g_end = g1;
        if constexpr (COUNTS) {
            if (in_image) n_p = aov_count_clamp(G.counts[frame_pix + ((size_t)pix_j * (size_t)A.reg_w + pix_i)], A.sample_end - A.sample_begin);
            uint32_t tile_max = n_p;   // (n_p depends on lane & 15 alone -- a round's four sample rows hold the same pixels --, so four steps cover the tile)
            for (int off = 8; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)tile_max, off); tile_max = o > tile_max ? o : tile_max; }
            tile_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_max);
            g_end = aov_count_group_end(g1, tile_max);
            if (g0 >= g_end) continue;   // nothing of this tile in the unit's range: neither the slot nor the accumulators are touched
        }
        for (uint32_t g = g0; g < g_end; g++) {
            const uint32_t s_off = g * 4u + (lane >> 4);   // begin + offset may pass INT32_MAX in the last group's padding: the offset decides
            const int32_t sample = (int32_t)((uint32_t)A.sample_begin + s_off);
            // else: padding of an edge tile or of the last group (COUNTS: n_p is 0 outside the image, one per-lane bound)
            const bool active = COUNTS ? s_off < n_p : in_image && s_off < (uint32_t)(A.sample_end - A.sample_begin);
            V3<real> ro = mk<real>(0, 0, 0), rd = mk<real>(0, 0, 1);
            real rtime = 0;
            uint64_t rng = 0;
            WalkState<real> ws;
            ws.inv = mk<real>(0, 0, 0); ws.dd = 0; ws.best_t = 0; ws.best = -1; ws.idx = n_entries; ws.exact_box = false; ws.oct = 0; ws.pending = -1;
            bool walking = false;
            if (active) {   // cast_ray's primary ray (the keyed camera is a per-launch, wave-uniform branch of camera_ray)
                if constexpr (VIEWS) camera_ray_of<real, true>(A, A.views[frame], cam_i, cam_j, sample, rng, ro, rd, rtime, frame_time);
                else if constexpr (BATCH) camera_ray<real, true>(A, cam_i, cam_j, sample, rng, ro, rd, rtime, frame_time);
                else camera_ray<real, true>(A, pix_i, pix_j, sample, rng, ro, rd, rtime);
                c_seg++;
                walk_begin(ws, rd, tree_walks_exact(A));
                walking = n_entries > 0;
            }
            // Hittables::hit on (0.001, inf): rounds of the walk until every lane has its closest hit
            while (__ballot(walking)) {
                walk_round<real, RES, ANIM, ORD, SCREEN>(A, lds_entries, prims, ro, rd, rtime, ws, walking, A.walk_round_steps, c_node, c_prim, nullptr, lds_screen);
                if (walking && ws.idx >= n_entries && ws.pending < 0) walking = false;
            }
            if (active) {
            V3<real> alb = mk<real>(0, 0, 0), n = mk<real>(0, 0, 0);
            real depth = r_inf(real(0));
            const bool hit = ws.best >= 0;
            if (hit) {
                const Prim<real>& p = prims[ws.best];
                const V3<real> loc = add(ro, scale(ws.best_t, rd));   // Ray::at
                if (want_depth) depth = r_sqrt(len2(sub(loc, ro)));
                if (want_albedo || want_normal) {
                    auto mat_at = [&](int32_t i) { return RES == RES_TOP ? load_rec(mats + i, A.lds_side != 0) : mats[i]; };
                    auto tex_at = [&](int32_t i) { return RES == RES_TOP ? load_rec(texs + i, A.lds_side != 0) : texs[i]; };
                    const Mat<real> m = mat_at(p.mat());
                    bool need_uv = false;
                    int32_t leaf_tex = -1;
                    if (want_albedo && m.kind == 0 && m.tex >= 0) {   // only image textures read u,v
                        int ti = m.tex;
                        Tex<real> tx = tex_at(ti);
                        CR_CHECKER_LEAF(tex_at, ti, tx, loc)
                        need_uv = tx.kind == 2;
                        leaf_tex = ti;
                    }
                    // the HitRecord's normal and u, v, as shade() forms them
                    real tu = 0, tv = 0;
                    if (p.kind() == 0) {
                        real g0s = p.g[0], g1s = p.g[1], g2s = p.g[2], g3s = p.g[3];
                        if (ANIM && p.key_count) {
                            timeline_eval(A.keys + p.key_first, p.key_count, rtime, g0s, g1s, g2s, g3s);
                            n = divs(sub(loc, mk<real>(g0s, g1s, g2s)), g3s);   // sphere.rs:97
                        } else n = scale(p.g[4], sub(loc, mk<real>(g0s, g1s, g2s)));   // p.g[4] = 1/radius
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
                    }
                    if (!(dot(rd, n) < real(0))) n = neg(n);            // HitRecord::new
                    if (want_albedo) {
                        if (m.kind == 0) {                              // Lambertian: tex.value(u, v, position)
                            if (m.tex < 0) alb = mk<real>(m.albedo[0], m.albedo[1], m.albedo[2]);
                            else {
                                const Tex<real> lt = tex_at(leaf_tex);
                                if (need_uv) alb = image_lookup(A.images, A.texels, lt.image, tu, tv, c_tex);
                                else alb = mk<real>(lt.color[0], lt.color[1], lt.color[2]);
                            }
                        } else if (m.kind == 1) alb = mk<real>(m.albedo[0], m.albedo[1], m.albedo[2]);
                        else alb = mk<real>(1, 1, 1);
                    }
                }
            } else if (want_albedo) {   // the sky ray_color returns for this ray: shade()'s miss branch with a unit throughput
                int32_t depth_left = 1, stack_n = 0;
                V3<real> thr = mk<real>(1, 1, 1);
                (void)shade<real, false, RES == RES_TOP, true>(A, prims, mats, texs, ro, rd, rtime, rng, depth_left, stack_n, ws.best_t, -1, 0u, 0u, c_tex, alb,
                                                               nullptr, &thr);
            }
            const real half = real(0.5);
            const real vals[7] = {alb.x, alb.y, alb.z, half * n.x + half, half * n.y + half, half * n.z + half, hit ? real(1) : real(0)};
            const bool want[7] = {want_albedo, want_albedo, want_albedo, want_normal, want_normal, want_normal, want_cover};
            uint32_t bad = 0;
#pragma unroll
            for (uint32_t c = 0; c < 7; c++) {
                if (!want[c]) continue;
                long long v = 0;
                if (!aov_word((double)vals[c], fxs, v)) bad |= 1u << c;
                else if (v) (void)__hip_atomic_fetch_add(slot_word(px * kAovWords + c), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (bad) atomicOr(G.flags + (BATCH ? frame_pix + ((size_t)pix_j * (size_t)A.reg_w + pix_i) : ((size_t)pix_j * (size_t)cam.W + pix_i)), bad);
            if (want_depth && hit) {
                unsigned long long bits, inf_bits;
                if constexpr (std::is_same<real, double>::value) { bits = __builtin_bit_cast(unsigned long long, depth); inf_bits = 0x7ff0000000000000ull; }
                else { bits = (unsigned long long)__builtin_bit_cast(uint32_t, depth); inf_bits = 0x7f800000ull; }
                if (bits < inf_bits)   // (a NaN's pattern lies above +inf's: the minimum over bit patterns never picks it)
                    (void)__hip_atomic_fetch_max(slot_word(px * kAovWords + kAovDepth), ~bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            }   // active
        }
        // the unit's words into the global accumulators
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t k = lane; k < kAovSlotWords; k += 64) {
            const unsigned long long v = slot[k];
            if (v) {   // (only pixels inside the image ever add)
                slot[k] = 0ull;
                const uint32_t q = k / kAovWords, ch = k - q * kAovWords;
                const uint32_t pi = (tile_x << 2) + (q & 3u), pj = (tile_y << 2) + (q >> 2);
                const size_t row_w = BATCH ? (size_t)A.reg_w : (size_t)cam.W;   // the accumulators' rows: the region's
                auto g = (__attribute__((address_space(1))) unsigned long long*)(G.acc + (BATCH ? frame_pix * kAovWords : 0) + ((size_t)pj * row_w + pi) * kAovWords + ch);
                if (ch == kAovDepth) (void)__hip_atomic_fetch_max(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else (void)__hip_atomic_fetch_add(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }

    flush_counters(WaveSum{}, A.counters, lane, c_seg, c_node, c_prim, c_tex);
}

// (the arguments are read through the kernarg segment where they are used, as pathtrace_kernel reads its own)
template <typename real, int RES, bool ANIM, bool ORD, bool SCREEN, bool BATCH = false>
__global__ void __launch_bounds__(MaxBlock<real>::value) aov_kernel(const AovArgs<real> G) {
    aov_body<real, RES, ANIM, ORD, SCREEN, BATCH>(*(const AovArgs<real>*)(const __attribute__((address_space(4))) AovArgs<real>*)__builtin_amdgcn_kernarg_segment_ptr());
}

// The kernels at a count plane (aov_counts_f32.hip, aov_counts_f64.hip): kernels of their own, so that the names of
// aov_kernel's instantiations stay what they were
template <typename real, int RES, bool ANIM, bool ORD, bool SCREEN>
__global__ void __launch_bounds__(MaxBlock<real>::value) aov_counts_kernel(const AovArgs<real> G) {
    aov_body<real, RES, ANIM, ORD, SCREEN, true, true>(*(const AovArgs<real>*)(const __attribute__((address_space(4))) AovArgs<real>*)__builtin_amdgcn_kernarg_segment_ptr());
}

// The kernels of several cameras in one launch (aov_views_f32.hip, aov_views_f64.hip): kernels of their own, for the same reason
template <typename real, int RES, bool ANIM, bool ORD, bool SCREEN>
__global__ void __launch_bounds__(MaxBlock<real>::value) aov_views_kernel(const AovArgs<real> G) {
    aov_body<real, RES, ANIM, ORD, SCREEN, true, false, true>(*(const AovArgs<real>*)(const __attribute__((address_space(4))) AovArgs<real>*)__builtin_amdgcn_kernarg_segment_ptr());
}

template <typename real, int RES, bool ANIM, bool ORD, bool SCREEN, bool BATCH, bool COUNTS, bool VIEWS = false>
auto aov_kernel_of() -> void (*)(const AovArgs<real>) {
    static_assert(!VIEWS || (BATCH && !COUNTS), "the VIEWS kernels are BATCH kernels without a count plane");
    if constexpr (VIEWS) return aov_views_kernel<real, RES, ANIM, ORD, SCREEN>;
    else if constexpr (COUNTS) return aov_counts_kernel<real, RES, ANIM, ORD, SCREEN>;
    else return aov_kernel<real, RES, ANIM, ORD, SCREEN, BATCH>;
}

#endif   // __HIPCC__

// One launch: persistent workgroups (one LDS copy of the scene each), the waves' slots behind the scene, units handed
// out by the work counter.  How large a unit is, how many a launch holds and on how many blocks it runs is
// launch_plan.hpp's arithmetic (plan_guide_units, plan_grid): a batch (a.n_frames frames, the BATCH
// kernels) is sized as one piece of work, whose frames share one ramp-up and one tail, and a batch with more units than
// the work counter holds runs as consecutive launches of whole frames, each on its own part of the accumulators.
// COUNTS: sized from params->samples all the same -- the host does not see a device plane --, so a unit beyond its tile's
// largest count costs one counter fetch and sixteen loads; each launch's frames read their own part of the plane.
// One body per precision: what the launch depends on in its kernel -- the residency, BATCH and COUNTS -- arrives as
// numbers beside the kernel's address (aov_variant names the kernels), so a unit compiles this once.
template <typename real>
int32_t aov_launch(CrHandle* h, void (*kern)(const AovArgs<real>), int res, bool batch, bool counts_plane, AovArgs<real>& a, size_t scene_lds_bytes, int* res_out) {
    const int max_block = MaxBlock<real>::value;
    const size_t off = res != RES_GLOBAL ? r16(scene_lds_bytes) : 0;
    a.acc_lds_off = (uint32_t)off;
    HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(off + aov_lds_bytes(max_block))));
    int block = 256, per_cu = 1;
    { int32_t rc = pick_block(h, (const void*)kern, max_block, true, off, aov_lds_bytes(64), "guide kernel does not fit on a CU", block, per_cu); if (rc != CR_OK) return rc; }
    const GuidePlan g = plan_guide_units(a.k.tiles_x, a.k.tiles_y, a.groups, batch, a.n_frames, h->n_cus, per_cu, block, h->work_counter_max);
    a.unit_groups = g.unit_groups;
    a.unit_chunks = g.unit_chunks;
    a.frame_tiles = g.frame_tiles;
    const size_t npix = (size_t)a.k.reg_w * (size_t)a.k.reg_h;
    unsigned long long* const acc = a.acc;
    uint32_t* const flags = a.flags;
    const real* const times = a.frame_times;
    const int32_t* const counts = a.counts;
    const CamConst<real>* const views = a.k.views;   // cr_render_aov_views_*: a frame is a view
    for (uint64_t f0 = 0; f0 < g.n_frames; f0 += g.frames_per_launch) {
        const uint64_t fn = g.slice_frames(f0);
        if (batch) {
            a.n_frames = (uint32_t)fn;
            a.frame_times = times + f0;
            a.acc = acc + f0 * npix * kAovWords;
            a.flags = flags + f0 * npix;
            if (counts_plane) a.counts = counts + f0 * npix;
            if (views) a.k.views = views + f0;
        }
        a.n_units = g.units(fn);
        const uint32_t grid = plan_grid(h->n_cus, per_cu, a.n_units, block, 64).blocks;   // a unit is a wave's
        HIP_TRY(h, hipMemsetAsync(h->work_counter.p, 0, 4, h->stream));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), off + aov_lds_bytes(block), h->stream, a);
        HIP_TRY(h, hipGetLastError());
        h->last_block = block; h->last_grid = (int)grid;
    }
    *res_out = res;
    return CR_OK;
}

// keyed primitives and leaves that hold a list walk with the ANIM decode (render.hip); a keyed camera needs no kernel of its own here
// a.n_frames != 0: a batch (cr_render_aov_frames_*), on the BATCH kernels whatever its length
template <typename real, int RES, bool ORD, bool SCREEN, bool COUNTS = false, bool VIEWS = false>
int32_t aov_variant(CrHandle* h, AovArgs<real>& a, size_t lds_bytes, const WalkChoice& w, int* res) {
    auto on = [&](auto batch) {
        constexpr bool BATCH = decltype(batch)::value;
        return aov_launch<real>(h, w.anim ? aov_kernel_of<real, RES, true, ORD, SCREEN, BATCH, COUNTS, VIEWS>() : aov_kernel_of<real, RES, false, ORD, SCREEN, BATCH, COUNTS, VIEWS>(),
                                RES, BATCH, COUNTS, a, lds_bytes, res);
    };
    // (COUNTS: a.n_frames >= 1, a single frame is a batch of one there, and a COUNTS unit instantiates no other kernel.  The
    // BATCH kernels are named first: a unit emits its kernels in the order it first names them, and the code the compiler
    // makes of a kernel depends on that order -- scripts/isa_diff.py shows it)
    if constexpr (COUNTS || VIEWS) return on(std::true_type{});   // (VIEWS: a.n_frames >= 1 as well, and a VIEWS unit instantiates no other kernel)
    else return a.n_frames ? on(std::true_type{}) : on(std::false_type{});
}

// The guide kernels' residency ladder: the rule walk_ladder asks (residency.hpp), so a guide pass stages what the render
// stages; the 6-waves-per-SIMD entry point has no counterpart here, so the query's latency inputs stay at never
template <typename real, bool ORD, bool COUNTS = false, bool VIEWS = false>
int32_t aov_ladder_ord(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res) {
    const Residency r = choose_residency(residency_query<real, ORD>(h, ds, w));
    a.k.lds_entries = r.lds_entries;
    if (r.lds_side) a.k.lds_side = 1;
    if (r.clear_screen) a.k.screen = nullptr;
    return residency_dispatch<!(ORD && std::is_same<real, float>::value), false>(r, [&](auto rs, auto screen, auto) {
        return aov_variant<real, decltype(rs)::value, ORD, decltype(screen)::value, COUNTS, VIEWS>(h, a, r.lds_bytes, w, res);
    });
}

template <typename real>
int32_t aov_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res) {
    return ds.ordered ? aov_ladder_ord<real, true>(h, a, ds, w, res) : aov_ladder_ord<real, false>(h, a, ds, w, res);
}

template <typename real>
int32_t aov_counts_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res) {
    return ds.ordered ? aov_ladder_ord<real, true, true>(h, a, ds, w, res) : aov_ladder_ord<real, false, true>(h, a, ds, w, res);
}

template <typename real>
int32_t aov_views_ladder(CrHandle* h, AovArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, int* res) {
    return ds.ordered ? aov_ladder_ord<real, true, false, true>(h, a, ds, w, res) : aov_ladder_ord<real, false, false, true>(h, a, ds, w, res);
}

}   // namespace cr
