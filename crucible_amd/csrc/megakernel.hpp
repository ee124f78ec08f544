// megakernel.hpp -- device only: the persistent kernel.  The lane states, stage_scene (the scene's LDS copy
// by residency.hpp's layout), kernel_args, pathtrace_body and its entry points pathtrace_kernel, _quiet, _listed, _views and
// _latency, and the two finalize kernels.  Every __global__ function here is a template: a unit emits the ones it names,
// in the order it first names them (render.hpp launch_variant), and no other unit emits any.
#pragma once
#include "shade.hpp"
#include "walk.hpp"
#include "launch_plan.hpp"   // fx_lds_bytes: the LDS of the relaxed sums' slots, and the rest of what sizes a launch

#if defined(__HIPCC__)

namespace cr {

// Diagnostic build: per-wave phase clocks go to counters[9..12] (regeneration, walk, shade, total).
#ifdef CR_DIAG
#define CR_DIAG_ONLY(...) __VA_ARGS__
#else
#define CR_DIAG_ONLY(...)
#endif

// TRACE: has a ray whose walk has not begun; WALK: walking (state kept across rounds of the outer loop);
// SHADE: closest hit known.
enum : int { ST_NEED_PIXEL = 0, ST_NEED_SAMPLE = 1, ST_TRACE = 2, ST_DONE = 3, ST_WALK = 4, ST_SHADE = 5 };

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
    // HEAD: the headline's kernels, the ones the switches of the work around the box step apply to (walk.hpp);
    // OFFS: their position is WalkOffset's LDS address, from walk_start (the first record) to walk_end (walk finished)
    constexpr bool HEAD = walk_offset<real, RES, ANIM, ORD, CAMK, RELAX, SCREEN>();
    constexpr bool OFFS = HEAD && CR_WALK_OFFSET != 0;
    std::conditional_t<OFFS, WalkOffset, WalkState<real>> ws;
    uint32_t walk_start = 0u, walk_end = 0u;
    if constexpr (OFFS) {
        walk_start = screen_lds_base<RES>(lds_screen); walk_end = walk_start + ((uint32_t)A.n_entries << 5);
        ws.dd = 0; ws.rda = quot_divide<real>(); ws.best_t = 0; ws.best = -1; ws.off = walk_start; ws.pending = -1;
    } else {
    ws.inv = mk<real>(0, 0, 0); ws.dd = 0; ws.rda = quot_divide<real>(); ws.best_t = 0; ws.best = -1; ws.idx = 0; ws.exact_box = false; ws.pending = -1;
    }
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
                if constexpr (OFFS) walk_begin_screened<quot_form<real, RES, ANIM, SCREEN>() == 1>(ws, ro, rd, walk_start);
                else if constexpr (LAZY) walk_begin_screened<quot_form<real, RES, ANIM, SCREEN>() == 1>(ws, ro, rd);
                else walk_begin<quot_form<real, RES, ANIM, SCREEN>() == 1>(ws, rd, exact_tree != 0u);
                state = n_entries > 0 ? ST_WALK : ST_SHADE;
            }
        }
        // Rounds of the while-while walk (walk_round).  After each round the wave may leave the walk if enough
        // lanes are done: the stragglers keep their WalkState and resume on the next round of the outer loop, so
        // each lane still performs BVHWrapper::hit's exact sequence; only the interleaving with other lanes'
        // shading changes.
        // The headline's kernels under either switch (walk.hpp): CR_WALK_PRIO -- the rounds run at wave priority 1, everything
        // else at 0; s_setprio ignores EXEC, so both stand under the scalar branch on the ballot, which the whole wave takes or
        // skips.  CR_WALK_OFFSET -- "walk finished" is one unsigned compare of the address with walk_end.  With both switches
        // off, and in every other kernel, the loop below is compiled: one loop with `if constexpr` around the three spots
        // did not compile those kernels to the code they had, so the loop stands twice.
        if constexpr (HEAD && (CR_WALK_OFFSET != 0 || CR_WALK_PRIO != 0)) {
            if (__ballot(state == ST_WALK)) {
                if constexpr (CR_WALK_PRIO != 0) __builtin_amdgcn_s_setprio(1);
                for (;;) {
                    walk_round<real, RES, ANIM, ORD, SCREEN, true, LAZY, sphere_loop<real, RES, ANIM, ORD, CAMK, SCREEN>()>(A, lds_entries, prims, ro, rd, rtime, ws, state == ST_WALK, A.walk_round_steps, c_node, c_prim, dgp, lds_screen);
                    bool done;
                    if constexpr (OFFS) done = ws.off >= walk_end; else done = ws.idx >= n_entries;
                    if (state == ST_WALK && done && ws.pending < 0) state = ST_SHADE;
                    const uint64_t walking = __ballot(state == ST_WALK);
                    if (!walking || 64u - (uint32_t)__popcll(walking) >= A.walk_exit_lanes) break;
                }
                if constexpr (CR_WALK_PRIO != 0) __builtin_amdgcn_s_setprio(0);
            }
        } else
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
template <typename real, bool ANIM, bool ORD = false, bool CAMK = false, bool RELAX = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, LatencyBlock), amdgpu_waves_per_eu(6, 6)))
pathtrace_kernel_latency(const KernelArgs<real> A) {
    pathtrace_body<real, RES_TOP, ANIM, ORD, CAMK, RELAX, false, false>(A);
}

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

}   // namespace cr

#endif   // __HIPCC__
