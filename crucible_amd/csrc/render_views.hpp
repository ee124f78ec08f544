// render_views.hpp -- the megakernels of cr_render_views_* (DESIGN.md 6.18): the keyed kernels of relaxed sums whose frames
// are views, each with a camera record of its own (pathtrace.hpp pathtrace_kernel_views, KernelArgs::views).  Included by
// render_views_f32.hip and render_views_f64.hip only, each of which instantiates views_ladder (both tree orders) for its
// precision.  The launch is render.hpp's launch<real, true>, whose finalize kernel stays with the relaxed unit that emits it.
#pragma once
#include "render.hpp"

namespace cr {

// (the sums' finalize is render_f32_relaxed.hip's / render_f64_relaxed.hip's: named here, not instantiated)
extern template int32_t fx_finalize<float>(CrHandle*, const unsigned long long*, float*, size_t, double, double, int32_t);
extern template int32_t fx_finalize<double>(CrHandle*, const unsigned long long*, double*, size_t, double, double, int32_t);

// The residency ladder of walk_ladder (render.hpp) over the VIEWS kernels: keyed primitives on the ANIM kernel, every
// other scene on CAMK, as a batch of frames runs.  The 6-waves-per-SIMD entry point has no counterpart here, so the
// query's latency inputs stay at never (relaxed sums: the residency does not change a byte).
template <typename real, bool ORD>
int32_t views_ladder(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, const WalkChoice& w, CrStats* stats, const FrameBatch<real>& fb) {
    constexpr bool f32 = std::is_same<real, float>::value;
    const Residency r = choose_residency(residency_query<real, ORD>(h, ds, w));
    a.lds_entries = r.lds_entries;
    if (r.lds_side) a.lds_side = 1;
    if (r.clear_screen) a.screen = nullptr;
    return residency_dispatch<!(ORD && f32), false>(r, [&](auto res, auto screen, auto) {
        constexpr int RES = decltype(res)::value;
        constexpr bool SCREEN = decltype(screen)::value;
        MegaKernel<real> k = {nullptr, nullptr, RES, true, false, false};
        if (w.anim) k.kern = pathtrace_kernel_views<real, RES, true, ORD, false, SCREEN>;
        else k.kern = pathtrace_kernel_views<real, RES, false, ORD, true, SCREEN>;
        return launch<real, true>(h, k, a, r.lds_bytes, stats, fb);
    });
}

// a unit's instantiations: the ladders of both tree orders, and with them every VIEWS kernel of its precision
#define CR_RENDER_VIEWS_UNIT(real)                                                                                                                          \
    template int32_t cr::views_ladder<real, false>(CrHandle*, KernelArgs<real>&, const DevScene<real>&, const WalkChoice&, CrStats*, const FrameBatch<real>&); \
    template int32_t cr::views_ladder<real, true>(CrHandle*, KernelArgs<real>&, const DevScene<real>&, const WalkChoice&, CrStats*, const FrameBatch<real>&);

}   // namespace cr
