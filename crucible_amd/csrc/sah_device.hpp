// CR_BVH_BUILD_DEVICE -- the CR_BVH_SAH / CR_BVH_SAH_ORDERED tree, built on the device.
// The same tree as SahBuilder's (tree.hpp), decision for decision: the device produces the node graph (left, right =
// left + 1, start, end, axis per node) and the final primitive order; SahBuilder::linearise and relayout_bfs run on the
// host on what comes back, and the wrapper boxes are filled bottom-up by run_box_kernels as for the LBVH.
//
//   large nodes (span > small_threshold), all of a level per round:
//     sah_bounds_kernel   centroid bounds per node       } a workgroup walks a contiguous chunk of `order`, reduces each
//     sah_bins_kernel     3 x 16 bins per node           } node's stretch of it in LDS, then adds that to the node's record
//     sah_split_kernel    one wave per node: the 45 planes, the winner, the two children (records of the next round,
//                         or entries of the small-subtree list)
//     sah_flags_kernel    goes-left flag per position, hipcub exclusive sum, sah_scatter_kernel: the stable partition
//   small subtrees (span <= small_threshold):
//     sah_small_kernel    one wave builds the whole subtree in LDS (its stretch of `order`, the bins, a range stack)
//
// The decision rules are the CR_HD functions below; both phases call the same ones, and tests/sah_device_check.cpp
// compiles them for the host and holds them to tests/sah_model.py.  Minima and maxima are taken on order-preserving
// integer keys (sah_key): they commute, a NaN is skipped rather than ordered, and of two zeros a minimum keeps -0 and a
// maximum +0 whatever the schedule -- which decides nothing: every use is a difference or a comparison.
#pragma once
#include "hd.hpp"   // CR_HD: inline under a plain C++ compiler (tests/sah_device_check.cpp)

#include <cstdint>

namespace cr {

constexpr int kSahBins = 16;                       // per axis
constexpr int kSahPlanes = kSahBins - 1;           // plane k: bins <= k | bins > k
constexpr int kSahAllBins = 3 * kSahBins;
constexpr uint64_t kSahKeyPosInf = 0xFFF0000000000000ull;   // sah_key(+inf): what a minimum starts from
constexpr uint64_t kSahKeyNegInf = 0x000FFFFFFFFFFFFFull;   // sah_key(-inf): what a maximum starts from

CR_HD uint64_t sah_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return b; }
CR_HD double sah_double(uint64_t b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
CR_HD double sah_inf() { return sah_double(0x7FF0000000000000ull); }

// The order-preserving key of x (a < b  <=>  key(a) < key(b); -0 below +0).  False for a NaN, which has no key: the
// caller skips it, as std::min(a, NaN) keeps a.
CR_HD bool sah_key(double x, uint64_t& k) {
    if (x != x) return false;
    const uint64_t b = sah_bits(x);
    k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return true;
}
CR_HD double sah_unkey(uint64_t k) { return sah_double((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k); }

// the bin of t = (cen - clo) * (16 / ext), clamped in floating point BEFORE the conversion.
// t >= 16 (inf included) is the last bin, anything that is not >= 0 (NaN included: 0 * inf, or a NaN centroid) the first.
CR_HD int sah_bin_of(double t) { return t >= (double)kSahBins ? kSahBins - 1 : (t >= 0.0 ? (int)t : 0); }

CR_HD double sah_centroid(double lo, double hi) { return 0.5 * (lo + hi); }

// (f): every product and sum rounded on its own (-ffp-contract=off on host and device)
CR_HD double sah_area(const double lo[3], const double hi[3]) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return 2.0 * ((dx * dy + dy * dz) + dz * dx);
}

// (c): an axis is a candidate only if ext = chi - clo is > 0 and finite; then scale = 16 / ext (which may be inf).
// With no centroid that is a number clo = +inf, chi = -inf and ext = -inf.
CR_HD bool sah_axis(double clo, double chi, double& scale) {
    const double ext = chi - clo;
    scale = 0.0;
    if (!(ext > 0.0) || !(ext < sah_inf())) return false;
    scale = (double)kSahBins / ext;
    return true;
}

// A primitive's centroid (box bx: lo xyz, hi xyz) into running bounds, as keys; a centroid that is no number bounds nothing.
CR_HD void sah_bound_centroid(const double* bx, uint64_t lo[3], uint64_t hi[3]) {
    for (int a = 0; a < 3; a++) {
        uint64_t k;
        if (!sah_key(sah_centroid(bx[a], bx[3 + a]), k)) continue;
        lo[a] = k < lo[a] ? k : lo[a];
        hi[a] = k > hi[a] ? k : hi[a];
    }
}

// A primitive's bin on every candidate axis, four bits each (0 on an axis that is none).
CR_HD uint32_t sah_bins_of(const double* bx, const double clo[3], const double scale[3], const bool ok[3]) {
    uint32_t packed = 0;
    for (int a = 0; a < 3; a++)
        if (ok[a]) packed |= (uint32_t)sah_bin_of((sah_centroid(bx[a], bx[3 + a]) - clo[a]) * scale[a]) << (4 * a);
    return packed;
}

// The candidate axes of a range from the keys of its centroid bounds.
CR_HD void sah_axes(const uint64_t* clo_k, const uint64_t* chi_k, double clo[3], double scale[3], bool ok[3]) {
    for (int a = 0; a < 3; a++) { clo[a] = sah_unkey(clo_k[a]); ok[a] = sah_axis(clo[a], sah_unkey(chi_k[a]), scale[a]); }
}

// The bins of a range: counts and the f64 unions of the primitive boxes, as keys.  lo / hi: [bin][3].
struct SahBins {
    uint32_t cnt[kSahAllBins];
    uint64_t lo[kSahAllBins * 3], hi[kSahAllBins * 3];
};

// (e), (f): the cost of plane k of axis a from that axis' 16 bins.  False where the plane is no candidate: a side is
// empty, or the cost is not < inf.  n_left: primitives in bins <= k.
CR_HD bool sah_plane_cost(const SahBins& b, int a, int k, double& cost, uint32_t& n_left) {
    const double inf = sah_inf();
    double l_lo[3] = {inf, inf, inf}, l_hi[3] = {-inf, -inf, -inf}, r_lo[3] = {inf, inf, inf}, r_hi[3] = {-inf, -inf, -inf};
    uint32_t nl = 0, nr = 0;
    for (int j = 0; j < kSahBins; j++) {
        const int at = a * kSahBins + j;
        const uint32_t c = b.cnt[at];
        if (!c) continue;
        const bool left = j <= k;
        if (left) nl += c; else nr += c;
        for (int d = 0; d < 3; d++) {
            const double l = sah_unkey(b.lo[at * 3 + d]), h = sah_unkey(b.hi[at * 3 + d]);
            if (left) { l_lo[d] = l < l_lo[d] ? l : l_lo[d]; l_hi[d] = h > l_hi[d] ? h : l_hi[d]; }
            else { r_lo[d] = l < r_lo[d] ? l : r_lo[d]; r_hi[d] = h > r_hi[d] ? h : r_hi[d]; }
        }
    }
    n_left = nl;
    cost = inf;
    if (nl == 0 || nr == 0) return false;
    cost = sah_area(l_lo, l_hi) * (double)nl + sah_area(r_lo, r_hi) * (double)nr;
    return cost < inf;
}

// (g): the first strict minimum in axis-major, plane-minor order is the lowest index axis * 15 + plane among the
// candidates of minimal cost.  Does candidate (cost, idx) beat (best, best_idx)?  No candidate: idx = kSahNone.
constexpr int kSahNone = 3 * kSahPlanes;
CR_HD bool sah_better(double cost, int idx, double best, int best_idx) {
    if (idx >= kSahNone) return false;
    if (best_idx >= kSahNone) return true;
    return cost < best || (cost == best && idx < best_idx);
}

// The decision of a range from its bins: the winning index axis * 15 + plane (kSahNone: no winner, the range splits in
// the middle with axis 0) and the size of the left side.  ok[a]: axis a is a candidate (sah_axis).  The serial form;
// sah_wave_pick below is the same over the lanes of a wave.
CR_HD int sah_pick(const SahBins& b, const bool ok[3], uint32_t& n_left) {
    int best = kSahNone;
    double best_cost = sah_inf();
    n_left = 0;
    for (int idx = 0; idx < kSahNone; idx++) {
        double cost; uint32_t nl;
        if (!ok[idx / kSahPlanes] || !sah_plane_cost(b, idx / kSahPlanes, idx % kSahPlanes, cost, nl)) continue;
        if (sah_better(cost, idx, best_cost, best)) { best = idx; best_cost = cost; n_left = nl; }
    }
    return best;
}

// One node of the graph the device hands back.  left < 0: a leaf of end - start = 1 or 2 primitives.
struct SahNodeRec { int32_t left, start, end, axis; };

struct SahDeviceStats { int32_t rounds = 0, large_nodes = 0, small_subtrees = 0, small_threshold = 0; };

// What one wave's subtree takes of LDS: two copies of its stretch of `order` and the packed bins of each primitive.
constexpr int32_t kSahSmallDefault = 256;   // not chosen by measurement yet: one wave's 64 lanes x 4, a fraction of the LDS
constexpr int32_t kSahSmallMax = 4096;      // 10 bytes per primitive + the bins: inside the 64 KiB a kernel gets unasked
constexpr int32_t kSahSmallMin = 2;         // a leaf

#if defined(__HIPCC__) && defined(CR_SAH_DEVICE_KERNELS)
// ================================================================== device only (sah_device.hip alone defines CR_SAH_DEVICE_KERNELS: the kernels are emitted by one unit)

// A large node of the current round.  sah_split_kernel (or the driver, for the root) creates the records of the next
// round with empty bounds and bins; bounds and bins kernels fill them; sah_split_kernel then decides.
struct SahSlot {
    uint64_t clo[3], chi[3];      // keys of the centroid bounds
    SahBins bins;
    int32_t node, start, end;
    int32_t mid, win, seg_left, seg_right, pad_;   // the decision: win = axis * 15 + plane or kSahNone; what `seg` becomes on either side
};

struct SahCounters { int32_t next_node, n_next, n_small, error; };

constexpr int kSahChunk = 2048;   // positions of `order` a workgroup of 256 walks

CR_D void sah_bins_clear(SahBins* b, int lane, int lanes) {
    for (int j = lane; j < kSahAllBins; j += lanes) b->cnt[j] = 0;
    for (int j = lane; j < kSahAllBins * 3; j += lanes) { b->lo[j] = kSahKeyPosInf; b->hi[j] = kSahKeyNegInf; }
}
CR_D void sah_slot_clear(SahSlot* s, int lane, int lanes) {
    if (lane < 3) { s->clo[lane] = kSahKeyPosInf; s->chi[lane] = kSahKeyNegInf; }
    sah_bins_clear(&s->bins, lane, lanes);
}

// A primitive into the bins of its range (LDS atomics); returns its three bins, four bits each.
CR_D uint32_t sah_bin_primitive(const double* bx, const double clo[3], const double scale[3], const bool ok[3], SahBins* b) {
    uint64_t klo[3] = {0, 0, 0}, khi[3] = {0, 0, 0};
    bool has[3];   // box coordinates are never NaN; one that were would bound nothing
    for (int d = 0; d < 3; d++) { const bool l = sah_key(bx[d], klo[d]), u = sah_key(bx[3 + d], khi[d]); has[d] = l && u; }
    const uint32_t packed = sah_bins_of(bx, clo, scale, ok);
    for (int a = 0; a < 3; a++) {
        if (!ok[a]) continue;
        const int at = a * kSahBins + (int)((packed >> (4 * a)) & 15);
        atomicAdd(&b->cnt[at], 1u);
        for (int d = 0; d < 3; d++) if (has[d]) {
            atomicMin((unsigned long long*)&b->lo[at * 3 + d], (unsigned long long)klo[d]);
            atomicMax((unsigned long long*)&b->hi[at * 3 + d], (unsigned long long)khi[d]);
        }
    }
    return packed;
}

// sah_pick over a wave: lane idx < 45 evaluates plane idx, a butterfly keeps the better of two by sah_better.  Every
// lane returns the winner.
CR_D int sah_wave_pick(const SahBins& b, const bool ok[3], int lane, uint32_t& n_left) {
    double cost = sah_inf();
    uint32_t nl = 0;
    int idx = kSahNone;
    if (lane < kSahNone && ok[lane / kSahPlanes] && sah_plane_cost(b, lane / kSahPlanes, lane % kSahPlanes, cost, nl)) idx = lane;
    for (int m = 32; m >= 1; m >>= 1) {
        const double oc = __shfl_xor(cost, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        const uint32_t on = (uint32_t)__shfl_xor((int)nl, m, 64);
        if (sah_better(oc, oi, cost, idx)) { cost = oc; idx = oi; nl = on; }
    }
    n_left = nl;
    return idx;
}

// The next stretch of a chunk: positions [pos, e) belong to large node `slot` (>= 0), or to no large node (slot < 0).
// `seg` holds, per position, the index of its large node's record or the complement of the end of a finished run.
CR_D void sah_stretch(const int32_t* seg, const SahSlot* slots, int32_t n_slots, int32_t pos, int32_t c1, int32_t& slot, int32_t& e) {
    const int32_t s = seg[pos];
    slot = -1;
    if (s < 0 || s >= n_slots) { e = ~s; }
    else { slot = s; e = slots[s].end; }
    if (e > c1) e = c1;
    if (e <= pos) e = pos + 1;   // cannot happen on a well-formed table; the walk must still end
}

__global__ void __launch_bounds__(256) sah_bounds_kernel(const int32_t* order, const int32_t* seg, int32_t n, const double* box, SahSlot* slots, int32_t n_slots) {
    __shared__ unsigned long long s_lo[3], s_hi[3];
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kSahChunk;
    const int32_t c1 = (int32_t)(c0 + kSahChunk < n ? c0 + kSahChunk : n);
    for (int32_t pos = (int32_t)c0; pos < c1;) {
        int32_t slot, e;
        sah_stretch(seg, slots, n_slots, pos, c1, slot, e);
        if (slot < 0) { pos = e; continue; }
        if (tid < 3) { s_lo[tid] = kSahKeyPosInf; s_hi[tid] = kSahKeyNegInf; }
        __syncthreads();
        uint64_t lo[3] = {kSahKeyPosInf, kSahKeyPosInf, kSahKeyPosInf}, hi[3] = {kSahKeyNegInf, kSahKeyNegInf, kSahKeyNegInf};
        for (int32_t i = pos + tid; i < e; i += 256) sah_bound_centroid(box + (size_t)order[i] * 6, lo, hi);
        for (int a = 0; a < 3; a++) {
            if (lo[a] != kSahKeyPosInf) atomicMin(&s_lo[a], (unsigned long long)lo[a]);
            if (hi[a] != kSahKeyNegInf) atomicMax(&s_hi[a], (unsigned long long)hi[a]);
        }
        __syncthreads();
        if (tid < 3) {
            atomicMin((unsigned long long*)&slots[slot].clo[tid], s_lo[tid]);
            atomicMax((unsigned long long*)&slots[slot].chi[tid], s_hi[tid]);
        }
        __syncthreads();
        pos = e;
    }
}

__global__ void __launch_bounds__(256) sah_bins_kernel(const int32_t* order, const int32_t* seg, int32_t n, const double* box, SahSlot* slots, int32_t n_slots,
                                                       uint16_t* pbins) {
    __shared__ SahBins s_bins;
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kSahChunk;
    const int32_t c1 = (int32_t)(c0 + kSahChunk < n ? c0 + kSahChunk : n);
    for (int32_t pos = (int32_t)c0; pos < c1;) {
        int32_t slot, e;
        sah_stretch(seg, slots, n_slots, pos, c1, slot, e);
        if (slot < 0) { pos = e; continue; }
        SahSlot* S = slots + slot;
        double clo[3], scale[3];
        bool ok[3];
        sah_axes(S->clo, S->chi, clo, scale, ok);
        sah_bins_clear(&s_bins, tid, 256);
        __syncthreads();
        for (int32_t i = pos + tid; i < e; i += 256) pbins[i] = (uint16_t)sah_bin_primitive(box + (size_t)order[i] * 6, clo, scale, ok, &s_bins);
        __syncthreads();
        for (int j = tid; j < kSahAllBins * 7; j += 256) {   // a bin's count, then its three minima and three maxima
            const int at = j / 7, f = j % 7;
            const uint32_t c = s_bins.cnt[at];
            if (!c) continue;
            if (f == 0) atomicAdd(&S->bins.cnt[at], c);
            else if (f <= 3) atomicMin((unsigned long long*)&S->bins.lo[at * 3 + f - 1], (unsigned long long)s_bins.lo[at * 3 + f - 1]);
            else atomicMax((unsigned long long*)&S->bins.hi[at * 3 + f - 4], (unsigned long long)s_bins.hi[at * 3 + f - 4]);
        }
        __syncthreads();
        pos = e;
    }
}

// One wave per large node: the decision, the node's record, and its two children -- a record of the next round where the
// child is large, an entry of the small-subtree list where it is not.
__global__ void __launch_bounds__(64) sah_split_kernel(SahSlot* cur, SahSlot* nxt, int32_t nxt_cap, SahNodeRec* nodes, int32_t node_cap,
                                                      int32_t* small_list, int32_t small_cap, SahCounters* ctr, int32_t small_threshold) {
    __shared__ SahBins s_bins;
    __shared__ int32_t s_child[4];   // node index of the left child; the children's `seg` values
    const int lane = (int)threadIdx.x;
    SahSlot* S = cur + blockIdx.x;
    for (int j = lane; j < (int)(sizeof(SahBins) / 8); j += 64) ((uint64_t*)&s_bins)[j] = ((const uint64_t*)&S->bins)[j];
    __syncthreads();
    double clo[3], scale[3];
    bool ok[3];
    sah_axes(S->clo, S->chi, clo, scale, ok);
    uint32_t n_left;
    const int win = sah_wave_pick(s_bins, ok, lane, n_left);
    const int32_t start = S->start, end = S->end, span = end - start;
    const int32_t mid = win < kSahNone ? start + (int32_t)n_left : start + span / 2;
    if (lane == 0) {
        const int32_t left = atomicAdd(&ctr->next_node, 2);
        s_child[0] = left;
        if (left < 0 || left + 2 > node_cap || mid <= start || mid >= end) { atomicExch(&ctr->error, 1); s_child[0] = -1; }
        else {
            nodes[S->node] = SahNodeRec{left, start, end, win < kSahNone ? win / kSahPlanes : 0};
            for (int c = 0; c < 2; c++) {
                const int32_t cs = c ? mid : start, ce = c ? end : mid;
                int32_t sv = ~ce;
                if (ce - cs > small_threshold) {
                    sv = atomicAdd(&ctr->n_next, 1);
                    if (sv >= nxt_cap) { atomicExch(&ctr->error, 2); sv = ~ce; }
                } else {
                    const int32_t k = atomicAdd(&ctr->n_small, 1);
                    if (k < small_cap) small_list[k] = left + c; else atomicExch(&ctr->error, 3);
                    nodes[left + c] = SahNodeRec{-1, cs, ce, 0};
                }
                s_child[1 + c] = sv;
            }
        }
    }
    __syncthreads();
    const int32_t left = s_child[0];
    if (left < 0) { if (lane == 0) { S->mid = end; S->win = kSahNone; S->seg_left = S->seg_right = ~end; } return; }
    for (int c = 0; c < 2; c++) {
        const int32_t sv = s_child[1 + c];
        if (sv < 0) continue;
        SahSlot* N = nxt + sv;
        sah_slot_clear(N, lane, 64);
        if (lane == 0) { N->node = left + c; N->start = c ? mid : start; N->end = c ? end : mid; }
    }
    if (lane == 0) { S->mid = mid; S->win = win; S->seg_left = s_child[1]; S->seg_right = s_child[2]; }
}

__global__ void sah_root_kernel(SahSlot* slots, int32_t n) {
    sah_slot_clear(slots, (int)threadIdx.x, (int)blockDim.x);
    if (threadIdx.x == 0) { slots->node = 0; slots->start = 0; slots->end = n; }
}

// (h): does position i go left?  With a winner by its bin, with none by its place in the range.
__global__ void sah_flags_kernel(const int32_t* seg, int32_t n, const SahSlot* slots, int32_t n_slots, const uint16_t* pbins, uint32_t* flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = seg[i];
    uint32_t f = 0;
    if (s >= 0 && s < n_slots) {
        const SahSlot& S = slots[s];
        if (S.win < kSahNone) f = (int)((pbins[i] >> (4 * (S.win / kSahPlanes))) & 15) <= S.win % kSahPlanes;
        else f = (int32_t)i - S.start < (S.mid - S.start);
    }
    flags[i] = f;
}

// The stable partition of every large node at once, from one exclusive sum of the flags over the whole array.
__global__ void sah_scatter_kernel(const int32_t* order, const int32_t* seg, int32_t n, const SahSlot* slots, int32_t n_slots, const uint32_t* flags,
                                   const uint32_t* scan, int32_t* order_out, int32_t* seg_out) {
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int32_t i = (int32_t)i64, s = seg[i];
    if (s < 0 || s >= n_slots) { order_out[i] = order[i]; seg_out[i] = s; return; }
    const SahSlot& S = slots[s];
    const int32_t r = (int32_t)(scan[i] - scan[S.start]);
    const bool left = flags[i] != 0;
    int32_t to = left ? S.start + r : S.mid + (i - S.start) - r;
    if (to < S.start || to >= S.end) to = i;   // cannot happen: flags and mid come from the same bins
    order_out[to] = order[i];
    seg_out[to] = left ? S.seg_left : S.seg_right;
}

// One wave builds the subtree of a range of at most `cap` primitives: its stretch of `order`, the bins and a range stack
// in LDS.  The smaller child is split next and the larger one stacked, so the stack stays below log2(cap) + 1 entries.
// Dynamic LDS: 2 * cap int32 (the stretch and the partition's target), cap uint16 (packed bins).
__global__ void __launch_bounds__(64) sah_small_kernel(int32_t* order, const double* box, SahNodeRec* nodes, int32_t node_cap, const int32_t* small_list,
                                                      SahCounters* ctr, int32_t cap) {
    extern __shared__ int32_t s_dyn[];
    __shared__ SahBins s_bins;
    __shared__ unsigned long long s_clo[3], s_chi[3];
    __shared__ int32_t s_stack[3 * 16];
    __shared__ int32_t s_left;
    int32_t* ord = s_dyn;
    int32_t* tmp = s_dyn + cap;
    uint16_t* pb = (uint16_t*)(s_dyn + 2 * cap);
    const int lane = (int)threadIdx.x;
    const int32_t root = small_list[blockIdx.x];
    const int32_t base = nodes[root].start, total = nodes[root].end - base;
    if (total < 1 || total > cap) { if (lane == 0) atomicExch(&ctr->error, 4); return; }
    for (int32_t j = lane; j < total; j += 64) ord[j] = order[base + j];
    int sp = 0;
    int32_t nd = root, s = 0, e = total;
    __syncthreads();
    for (;;) {
        const int32_t span = e - s;
        if (span <= 2) {
            if (lane == 0) nodes[nd] = SahNodeRec{-1, base + s, base + e, 0};
            if (sp == 0) break;
            sp--;
            nd = s_stack[3 * sp]; s = s_stack[3 * sp + 1]; e = s_stack[3 * sp + 2];
            continue;
        }
        if (lane < 3) { s_clo[lane] = kSahKeyPosInf; s_chi[lane] = kSahKeyNegInf; }
        sah_bins_clear(&s_bins, lane, 64);
        __syncthreads();
        {
            uint64_t lo[3] = {kSahKeyPosInf, kSahKeyPosInf, kSahKeyPosInf}, hi[3] = {kSahKeyNegInf, kSahKeyNegInf, kSahKeyNegInf};
            for (int32_t j = s + lane; j < e; j += 64) sah_bound_centroid(box + (size_t)ord[j] * 6, lo, hi);
            for (int a = 0; a < 3; a++) {
                if (lo[a] != kSahKeyPosInf) atomicMin(&s_clo[a], (unsigned long long)lo[a]);
                if (hi[a] != kSahKeyNegInf) atomicMax(&s_chi[a], (unsigned long long)hi[a]);
            }
        }
        __syncthreads();
        double clo[3], scale[3];
        bool ok[3];
        sah_axes((const uint64_t*)s_clo, (const uint64_t*)s_chi, clo, scale, ok);
        for (int32_t j = s + lane; j < e; j += 64) pb[j] = (uint16_t)sah_bin_primitive(box + (size_t)ord[j] * 6, clo, scale, ok, &s_bins);
        __syncthreads();
        uint32_t n_left;
        const int win = sah_wave_pick(s_bins, ok, lane, n_left);
        const int32_t mid = win < kSahNone ? s + (int32_t)n_left : s + span / 2;
        const int axis = win < kSahNone ? win / kSahPlanes : 0, plane = win % kSahPlanes;
        int32_t nl = 0, nr = 0;   // placed so far on either side
        for (int32_t j0 = s; j0 < e; j0 += 64) {   // (h): the stable partition, 64 positions at a time
            const int32_t j = j0 + lane;
            const bool valid = j < e;
            const bool left = valid && (win < kSahNone ? (int)((pb[j] >> (4 * axis)) & 15) <= plane : j < mid);
            const unsigned long long bl = __ballot(left), bv = __ballot(valid);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (valid) {
                int32_t to = left ? s + nl + __popcll(bl & below) : mid + nr + __popcll(bv & ~bl & below);
                if (to < s || to >= e) to = j;   // cannot happen: the flags and mid come from the same bins
                tmp[to] = ord[j];
            }
            nl += __popcll(bl); nr += __popcll(bv & ~bl);
        }
        __syncthreads();
        for (int32_t j = s + lane; j < e; j += 64) ord[j] = tmp[j];
        if (lane == 0) {
            int32_t left = atomicAdd(&ctr->next_node, 2);
            if (left < 0 || left + 2 > node_cap || mid <= s || mid >= e) { atomicExch(&ctr->error, 5); left = -1; }
            else nodes[nd] = SahNodeRec{left, base + s, base + e, axis};
            s_left = left;
        }
        __syncthreads();
        const int32_t left = s_left;
        if (left < 0) return;   // the driver sees the error word
        const bool left_smaller = mid - s <= e - mid;
        if (sp >= 16) { if (lane == 0) atomicExch(&ctr->error, 6); return; }   // cannot happen: the stacked range is the larger half
        if (lane == 0) {
            s_stack[3 * sp] = left_smaller ? left + 1 : left;
            s_stack[3 * sp + 1] = left_smaller ? mid : s;
            s_stack[3 * sp + 2] = left_smaller ? e : mid;
        }
        sp++;
        if (left_smaller) { nd = left; e = mid; } else { nd = left + 1; s = mid; }
        __syncthreads();
    }
    __syncthreads();
    for (int32_t j = lane; j < total; j += 64) order[base + j] = ord[j];
}

#endif   // __HIPCC__ && CR_SAH_DEVICE_KERNELS

}   // namespace cr
