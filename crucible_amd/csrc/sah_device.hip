// sah_device.hip -- the driver of the device-side binned-SAH build (sah_device.hpp): rounds over the large
// nodes of a level, then one wave per small subtree; hands build_dev_scene the node graph and the primitive order.
#include "handle.hpp"
#define CR_SAH_DEVICE_KERNELS
#include "sah_device.hpp"
#include <hipcub/hipcub.hpp>

namespace cr {

// CRUCIBLE_SAH_SMALL, read at every build and clamped to what a wave's LDS holds
int32_t sah_small_threshold() {
    int32_t t = kSahSmallDefault;
    if (const char* e = getenv("CRUCIBLE_SAH_SMALL")) { char* end = nullptr; const long v = strtol(e, &end, 10); if (end != e) t = (int32_t)std::min<long>(std::max<long>(v, kSahSmallMin), kSahSmallMax); }
    return t;
}

#define SAH_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(h, CR_ERR_HIP, std::string("device SAH build: ") + hipGetErrorString(e_)); } while (0)

int32_t build_sah_device(CrHandle* h, const double* boxes, int32_t n, std::vector<SahNodeRec>& nodes, std::vector<int32_t>& order, SahDeviceStats& st) {
    st = SahDeviceStats();
    nodes.clear();
    if (n < 1) return CR_OK;
    SAH_TRY(h->sah_work.box.ensure((size_t)n * 48));
    SAH_TRY(hipMemcpyAsync(h->sah_work.box.p, boxes, (size_t)n * 48, hipMemcpyHostToDevice, h->stream));
    return build_sah_device_resident(h, n, nodes, order, st);
}

int32_t build_sah_device_resident(CrHandle* h, int32_t n, std::vector<SahNodeRec>& nodes, std::vector<int32_t>& order, SahDeviceStats& st) {
    st = SahDeviceStats();
    const int32_t T = st.small_threshold = sah_small_threshold();
    nodes.clear();
    if (n < 1) return CR_OK;
    const int32_t node_cap = 2 * n + 2;
    // the working set lives on the handle (SahDeviceWork): grow-only, so a rebuild of the same scene allocates nothing
    SahDeviceWork& w = h->sah_work;
    DevBuf &d_box = w.box, *d_order = w.order, *d_seg = w.seg, &d_pbins = w.pbins, &d_flags = w.flags, &d_scan = w.scan, &d_tmp = w.tmp, *d_slots = w.slots,
           &d_nodes = w.nodes, &d_small = w.small, &d_ctr = w.ctr;
    const bool large = n > T;
    if (d_box.bytes < (size_t)n * 48) return fail(h, CR_ERR_HIP, "device SAH build: the primitive boxes are not on the device");
    order.resize(n);
    for (int32_t i = 0; i < n; i++) order[i] = i;
    SAH_TRY(d_order[0].ensure((size_t)n * 4));
    SAH_TRY(hipMemcpyAsync(d_order[0].p, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    SAH_TRY(d_nodes.ensure((size_t)node_cap * sizeof(SahNodeRec)));
    SAH_TRY(d_small.ensure((size_t)n * 4));
    SAH_TRY(d_ctr.ensure(sizeof(SahCounters)));
    SahCounters ctr{1, 0, large ? 0 : 1, 0};
    SAH_TRY(hipMemcpyAsync(d_ctr.p, &ctr, sizeof ctr, hipMemcpyHostToDevice, h->stream));
    int cur = 0;
    if (large) {
        const int32_t slot_bound = n / (T + 1) + 1;   // disjoint ranges of more than T primitives each
        size_t tmp_bytes = 0;
        SAH_TRY(d_order[1].ensure((size_t)n * 4));
        SAH_TRY(d_seg[0].ensure((size_t)n * 4)); SAH_TRY(d_seg[1].ensure((size_t)n * 4));
        SAH_TRY(d_pbins.ensure((size_t)n * 2));
        SAH_TRY(d_flags.ensure((size_t)n * 4)); SAH_TRY(d_scan.ensure((size_t)n * 4));
        SAH_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint32_t*)d_flags.p, (uint32_t*)d_scan.p, n, h->stream));
        SAH_TRY(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        SAH_TRY(hipMemsetAsync(d_seg[0].p, 0, (size_t)n * 4, h->stream));   // every position: record 0, the root
        SAH_TRY(d_slots[0].ensure(sizeof(SahSlot)));
        hipLaunchKernelGGL(sah_root_kernel, dim3(1), dim3(64), 0, h->stream, (SahSlot*)d_slots[0].p, n);
        SAH_TRY(hipGetLastError());
        const dim3 chunks((unsigned)(((int64_t)n + kSahChunk - 1) / kSahChunk)), per_pos((unsigned)(((int64_t)n + 255) / 256));
        int32_t active = 1;
        int s_cur = 0;
        while (active > 0) {
            const int32_t nxt_cap = (int32_t)std::min<int64_t>(2 * (int64_t)active, slot_bound);
            SAH_TRY(d_slots[s_cur ^ 1].ensure((size_t)nxt_cap * sizeof(SahSlot)));
            SAH_TRY(hipMemsetAsync((char*)d_ctr.p + offsetof(SahCounters, n_next), 0, 4, h->stream));
            SahSlot* slots = (SahSlot*)d_slots[s_cur].p;
            const int32_t *ord = (const int32_t*)d_order[cur].p, *seg = (const int32_t*)d_seg[cur].p;
            hipLaunchKernelGGL(sah_bounds_kernel, chunks, dim3(256), 0, h->stream, ord, seg, n, (const double*)d_box.p, slots, active);
            hipLaunchKernelGGL(sah_bins_kernel, chunks, dim3(256), 0, h->stream, ord, seg, n, (const double*)d_box.p, slots, active, (uint16_t*)d_pbins.p);
            hipLaunchKernelGGL(sah_split_kernel, dim3((unsigned)active), dim3(64), 0, h->stream, slots, (SahSlot*)d_slots[s_cur ^ 1].p, nxt_cap,
                               (SahNodeRec*)d_nodes.p, node_cap, (int32_t*)d_small.p, n, (SahCounters*)d_ctr.p, T);
            hipLaunchKernelGGL(sah_flags_kernel, per_pos, dim3(256), 0, h->stream, seg, n, (const SahSlot*)slots, active, (const uint16_t*)d_pbins.p, (uint32_t*)d_flags.p);
            SAH_TRY(hipGetLastError());
            SAH_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, (const uint32_t*)d_flags.p, (uint32_t*)d_scan.p, n, h->stream));
            hipLaunchKernelGGL(sah_scatter_kernel, per_pos, dim3(256), 0, h->stream, ord, seg, n, (const SahSlot*)slots, active, (const uint32_t*)d_flags.p,
                               (const uint32_t*)d_scan.p, (int32_t*)d_order[cur ^ 1].p, (int32_t*)d_seg[cur ^ 1].p);
            SAH_TRY(hipGetLastError());
            SAH_TRY(hipMemcpyAsync(&ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, h->stream));   // the large nodes left: once per round
            SAH_TRY(hipStreamSynchronize(h->stream));
            if (ctr.error || ctr.n_next < 0 || ctr.n_next > nxt_cap) return fail(h, CR_ERR_HIP, "device SAH build: a round left an inconsistent state");
            st.rounds++;
            st.large_nodes += active;
            active = ctr.n_next;
            cur ^= 1; s_cur ^= 1;
        }
    } else {
        const SahNodeRec root{-1, 0, n, 0};
        const int32_t zero = 0;
        SAH_TRY(hipMemcpyAsync(d_nodes.p, &root, sizeof root, hipMemcpyHostToDevice, h->stream));
        SAH_TRY(hipMemcpyAsync(d_small.p, &zero, 4, hipMemcpyHostToDevice, h->stream));
        SAH_TRY(hipStreamSynchronize(h->stream));   // the two sources are locals
    }
    const int32_t n_small = ctr.n_small;
    if (n_small < 1 || n_small > n) return fail(h, CR_ERR_HIP, "device SAH build: bad small-subtree count");
    const int32_t cap = std::min(T, n);
    hipLaunchKernelGGL(sah_small_kernel, dim3((unsigned)n_small), dim3(64), (size_t)cap * 10 + 16, h->stream, (int32_t*)d_order[cur].p, (const double*)d_box.p,
                       (SahNodeRec*)d_nodes.p, node_cap, (const int32_t*)d_small.p, (SahCounters*)d_ctr.p, cap);
    SAH_TRY(hipGetLastError());
    SAH_TRY(hipMemcpyAsync(&ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, h->stream));
    SAH_TRY(hipMemcpyAsync(order.data(), d_order[cur].p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    SAH_TRY(hipStreamSynchronize(h->stream));
    if (ctr.error || ctr.next_node < 1 || ctr.next_node > node_cap) return fail(h, CR_ERR_HIP, "device SAH build: the small-subtree pass left an inconsistent state");
    nodes.resize((size_t)ctr.next_node);
    SAH_TRY(hipMemcpyAsync(nodes.data(), d_nodes.p, nodes.size() * sizeof(SahNodeRec), hipMemcpyDeviceToHost, h->stream));
    SAH_TRY(hipStreamSynchronize(h->stream));
#undef SAH_TRY
    st.small_subtrees = n_small;
    // what linearise will follow: every node named once, children inside the array, ranges that nest
    const int32_t total = (int32_t)nodes.size();
    std::vector<char> seen((size_t)total, 0);
    seen[0] = 1;
    if (nodes[0].start != 0 || nodes[0].end != n) return fail(h, CR_ERR_HIP, "device SAH build: malformed node graph");
    for (int32_t i = 0; i < total; i++) {
        const SahNodeRec& nd = nodes[i];
        if (!seen[i] || nd.start < 0 || nd.end > n || nd.end <= nd.start) return fail(h, CR_ERR_HIP, "device SAH build: malformed node graph");
        if (nd.left < 0) { if (nd.end - nd.start > 2) return fail(h, CR_ERR_HIP, "device SAH build: malformed node graph"); continue; }
        if (nd.left < 1 || nd.left + 1 >= total || seen[nd.left] || seen[nd.left + 1] || nd.axis < 0 || nd.axis > 2)
            return fail(h, CR_ERR_HIP, "device SAH build: malformed node graph");
        const SahNodeRec &l = nodes[nd.left], &r = nodes[nd.left + 1];
        if (l.start != nd.start || l.end != r.start || r.end != nd.end) return fail(h, CR_ERR_HIP, "device SAH build: malformed node graph");
        seen[nd.left] = seen[nd.left + 1] = 1;
    }
    std::vector<char> placed((size_t)n, 0);
    for (int32_t i = 0; i < n; i++) {
        if (order[i] < 0 || order[i] >= n || placed[order[i]]) return fail(h, CR_ERR_HIP, "device SAH build: the primitive order is no permutation");
        placed[order[i]] = 1;
    }
    return CR_OK;
}

}   // namespace cr
