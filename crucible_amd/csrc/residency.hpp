// residency.hpp -- how much of a scene a launch stages in LDS and where it lies there: one layout,
// scene_layout, for every kernel that stages and every host computation of the bytes; one rule, choose_residency, for the render
// kernels' ladder (render.hpp walk_ladder) and the guide kernels' (aov_kernel.hpp aov_ladder_ord), which only fill a query
// and dispatch on the answer.  Free of the HIP runtime and of the record types -- sizes arrive as numbers --, so that a
// plain C++ compiler can check it (tests/residency_check.cpp), as it checks fastdiv.hpp, tree.hpp and adaptive.hpp.  How a
// launch is sized once the residency is settled is launch_plan.hpp's, which builds on this header.
#pragma once
#include "hd.hpp"

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace cr {

// Where the scene is read from: RES_GLOBAL everything through L2; RES_LDS entries | primitives |
// materials | textures staged in LDS; RES_TOP only the first lds_entries wrappers (top levels) in LDS.
enum : int { RES_GLOBAL = 0, RES_LDS = 1, RES_TOP = 2 };

CR_HD size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }

// The scene's LDS copy: records | primitives | materials | textures, each table at a multiple of 16 bytes.  The records
// at offset 0 are wrappers or screening records (the whole tree, or a window of its top); with_prims: the primitive table
// follows them (RES_LDS); with_side: materials and textures follow (RES_LDS, and RES_TOP where they ride along).  A table
// that is not staged takes no room.  `bytes` ends the last table; what a launch puts behind the scene (the waves' slots,
// the queue's state) begins at end().  stage_scene (megakernel.hpp) copies by this, and the host sizes its launches by it.
// The four sizes are the tables' bytes (records * bytes of one), formed by the caller: a kernel copies by the same products.
struct SceneLayout {
    size_t prims, mats, texs;   // offsets of the tables
    size_t bytes;
    CR_HD size_t end() const { return r16(bytes); }
};
CR_HD SceneLayout scene_layout(size_t record_bytes, size_t prim_bytes, size_t mat_bytes, size_t tex_bytes, bool with_prims, bool with_side) {
    SceneLayout l;
    l.bytes = record_bytes;
    l.prims = l.mats = l.texs = r16(record_bytes);
    if (with_prims) { l.bytes = l.prims + prim_bytes; l.mats = l.texs = l.prims + r16(prim_bytes); }
    if (with_side) { l.texs = l.mats + r16(mat_bytes); l.bytes = l.texs + tex_bytes; }
    return l;
}

// What the two side tables take behind a window: their own layout from offset 0
CR_HD size_t side_table_bytes(size_t mat_bytes, size_t tex_bytes) { return scene_layout(0, 0, mat_bytes, tex_bytes, false, true).end(); }

struct ResidencyQuery {
    int32_t n_entries;
    size_t entry_rec, screen_rec;        // bytes of one wrapper / one screening record of the tree's order
    bool ordered;
    bool can_screen;                     // false for an ordered f32 tree: it has no screening records, so no SCREEN kernels
    bool screen, screen_lds, plain_lds;  // WalkChoice: walk on screening records; the whole scene fits with them / with its wrappers
    size_t lds_bytes, lds_all_screen;    // LDS bytes of the whole scene with its wrappers / with screening records in their place
    size_t side_bytes;                   // the side tables behind a window: side_table_bytes(materials, textures)
    size_t lds_top_bytes, lds_side_limit;   // the handle's window and its limit for the side tables
    // The 6-waves-per-SIMD entry point: f32 trees of more than latency_entries wrappers, whole frames outside adaptive runs,
    // on a window of latency_top_bytes.  Its three 512-thread groups per CU share 160 KB: window, side tables and
    // latency_slot_bytes of relaxed sums' slots each.  The guide pass leaves whole_frame false: never.
    bool f32, whole_frame, adaptive;
    int32_t latency_entries;
    size_t latency_top_bytes, latency_slot_bytes;
};

struct Residency {
    int res;               // RES_*
    bool screen;           // a SCREEN kernel runs: the window (or the whole tree) holds screening records
    bool latency;          // the 6-waves-per-SIMD entry point runs (RES_TOP only, never a SCREEN kernel)
    int32_t lds_entries;   // records staged: all, the window's, none
    int32_t lds_side;      // RES_TOP: materials and textures follow the window
    size_t lds_bytes;      // the scene's LDS bytes
    bool clear_screen;     // the plain RES_LDS kernel: the caller nulls its screening pointer
};

// The ladder: the whole scene in LDS, else a window of the tree's top there (RES_TOP), else everything through L2.  What
// the tree orders differ in: an ordered f32 tree has no SCREEN kernels; the window's record size; and the side tables
// join the window on unordered trees only.
CR_HD Residency choose_residency(const ResidencyQuery& q) {
    Residency r = {RES_GLOBAL, q.can_screen && q.screen, false, 0, 0, 0, false};
    if (q.n_entries > 0 && (q.plain_lds || q.screen_lds)) {
        r.res = RES_LDS;
        r.lds_entries = q.n_entries;
        r.screen = q.can_screen && q.screen_lds;
        r.lds_bytes = r.screen ? q.lds_all_screen : q.lds_bytes;
        r.clear_screen = !r.screen;
        return r;
    }
    const bool latency = q.f32 && q.whole_frame && !q.adaptive && q.latency_entries > 0 && q.n_entries > q.latency_entries;
    // a window of screening records holds twice the wrappers
    const size_t window_rec = q.screen ? q.screen_rec : q.entry_rec;
    const size_t fit = (latency ? q.latency_top_bytes : q.lds_top_bytes) / window_rec;
    const int32_t top = (int32_t)((size_t)q.n_entries < fit ? (size_t)q.n_entries : fit);
    if (top <= 0) return r;
    // large scene: the top levels of the tree in LDS, everything else through L2
    r.res = RES_TOP;
    r.lds_entries = top;
    r.latency = latency;
    r.screen = r.screen && !latency;
    const SceneLayout window = scene_layout((size_t)top * window_rec, 0, 0, 0, false, false);
    r.lds_bytes = window.bytes;
    if (!q.ordered) {   // materials and textures ride along when they are small (the tree can be large with two materials)
        const size_t third = (size_t)160 * 1024 / 3 - 16, used = r.lds_bytes + q.latency_slot_bytes;
        const size_t cap = latency ? (third > used ? third - used : 0) : q.lds_side_limit;
        // the side tables begin where the window's layout ends, and side_bytes is what a layout of the two alone takes
        if (q.side_bytes <= (q.lds_side_limit < cap ? q.lds_side_limit : cap)) { r.lds_side = 1; r.lds_bytes = window.end() + q.side_bytes; }
    }
    return r;
}

// f(res, screen, latency) with the choice as std::integral_constant tags, so that a ladder names its kernel once.  Only
// what choose_residency can answer is instantiated: SCREEN where CAN_SCREEN, latency where CAN_LATENCY and then RES_TOP
// without SCREEN alone.
template <bool CAN_SCREEN, bool CAN_LATENCY, typename F>
auto residency_dispatch(const Residency& r, F&& f) {
    using no = std::false_type;
    auto by_screen = [&](auto res) {
        if constexpr (CAN_SCREEN) if (r.screen) return f(res, std::true_type{}, no{});
        return f(res, no{}, no{});
    };
    if (r.res == RES_LDS) return by_screen(std::integral_constant<int, RES_LDS>{});
    if (r.res == RES_TOP) {
        if constexpr (CAN_LATENCY) if (r.latency) return f(std::integral_constant<int, RES_TOP>{}, no{}, std::true_type{});
        return by_screen(std::integral_constant<int, RES_TOP>{});
    }
    return by_screen(std::integral_constant<int, RES_GLOBAL>{});
}

}   // namespace cr
