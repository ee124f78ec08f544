// screen.hpp -- the kernels that derive a tree's f32 screening records (records.hpp: ScreenEntry, ScreenEntryO; walk.hpp: walk_round)
// from its wrappers.  Included by scene.hip alone: one of the kernels is no template, so every unit that read its
// definition would emit it.
#pragma once
#include "records.hpp"

namespace cr {

// One record per wrapper: its box plane by plane through screen_plane (records.hpp), its links copied.  Run after every
// upload and after every refit of the f64 boxes.
template <typename real>
__global__ void __launch_bounds__(256) screen_from_entries_kernel(const Entry<real>* e, ScreenEntry* s, int32_t n, int32_t* overflow) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const Entry<real> v = e[i];
    ScreenEntry o;
    for (int k = 0; k < 6; k++) screen_plane(v.b[k], o.b[k], overflow);
    o.skip = (uint32_t)v.skip << 5;
    o.hit = v.leaf < 0 ? (uint32_t)(-v.leaf) << 5 : (kScreenLeaf | (uint32_t)v.leaf);
    s[i] = o;
}

__global__ void __launch_bounds__(256) screen_from_ordered_entries_kernel(const EntryO<double>* e, ScreenEntryO* s, int32_t n, int32_t* overflow) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const EntryO<double> v = e[i];
    ScreenEntryO o;
    for (int k = 0; k < 6; k++) screen_plane(v.b[k], o.b[k], overflow);
    if (v.leaf < 0) { o.axis = (uint32_t)(-v.leaf) & 3u; o.hit = (uint32_t)ordered_left(v.leaf) << 6; }
    else { o.axis = 3u; o.hit = kScreenLeaf | (uint32_t)v.leaf; }
    for (int k = 0; k < 8; k++) o.skip[k] = (uint32_t)v.skip[k] << 6;
    s[i] = o;
}

}   // namespace cr
