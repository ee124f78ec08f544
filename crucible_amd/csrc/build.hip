// build.hip -- from the handle's host copy of the scene to a precision's device copy (build_dev_scene): filters hidden
// primitives, builds the BVH in the reference's topology (or the opt-in SAH / LBVH trees), lays tree and primitives out
// for the device and uploads them; cr_export_bvh hands the tree back, cr_build_info what the build did.  Also the second
// tree of refit_boxes = CR_REFIT_REBUILD (build_frame_scene, select_tree; cr_export_render_bvh, cr_frame_build_info).  Includes hipcub
// (as sah_device.hip does, the driver of the device-side SAH build this unit calls under CR_BVH_BUILD_DEVICE).
#include "handle.hpp"
#include "lbvh.hpp"
#include "sah_device.hpp"
#include "pack.hpp"
#include "refit.hpp"
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <thread>

namespace cr {

// ---------------------------------------------------------------- BVH build
// BVHWrapper::help_generate (src/objects/bvhwrapper.rs:46-78) emitted as a threaded
// pre-order array.  Node box = union of the range's construction-time primitive boxes
// (:47-50); axis = longest_axis with strict '>' (bvh.rs:82-94); span 1 and 2 become
// leaves without sorting (:58-63); span >= 3: stable sort by box min on the axis
// (sort_by is stable, :66-67), mid = start + span/2 (:71).
template <typename real> struct Builder {
    std::vector<real> bmin[3], bmax[3];
    std::vector<int32_t> order;
    std::vector<Entry<real>> entries;

    // Number of wrappers of a range of `span` primitives: a pure function of the span (median split),
    // so every subtree's position in the pre-order array is known before it is built and subtrees can
    // be built by independent threads.
    static int32_t tree_size(int32_t span) {
        if (span <= 2) return span > 0 ? 1 : 0;
        return 1 + tree_size(span / 2) + tree_size(span - span / 2);   // depth log2(n), two distinct spans per level
    }

    void build_root(int32_t n) {
        sizes.clear();
        entries.assign((size_t)size_of(n), Entry<real>());
        build(0, n, 0, 0);
    }

  private:
    std::map<int32_t, int32_t> sizes;
    int32_t size_of(int32_t span) {
        if (span <= 2) return span > 0 ? 1 : 0;
        auto it = sizes.find(span);
        if (it != sizes.end()) return it->second;
        int32_t v = 1 + size_of(span / 2) + size_of(span - span / 2);
        sizes[span] = v;
        return v;
    }

    void build(int32_t start, int32_t end, int32_t idx, int depth) {
        real lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
        for (int32_t i = start; i < end; i++) {
            int32_t p = order[i];
            for (int a = 0; a < 3; a++) {   // Interval::tight_enclose, utils.rs:629-633
                lo[a] = lo[a] <= bmin[a][p] ? lo[a] : bmin[a][p];
                hi[a] = hi[a] >= bmax[a][p] ? hi[a] : bmax[a][p];
            }
        }
        real sx = hi[0] - lo[0], sy = hi[1] - lo[1], sz = hi[2] - lo[2];
        int axis = (sx > sy) ? ((sx > sz) ? 0 : 2) : ((sy > sz) ? 1 : 2);
        int32_t span = end - start;
        Entry<real> e;
        e.b[0] = lo[0]; e.b[1] = hi[0]; e.b[2] = lo[1]; e.b[3] = hi[1]; e.b[4] = lo[2]; e.b[5] = hi[2];
        e.skip = idx + 1; e.leaf = -1;
        if (span <= 2) { e.leaf = (start << 1) | (span - 1); entries[idx] = e; return; }
        const std::vector<real>& key = bmin[axis];
        std::stable_sort(order.begin() + start, order.begin() + end, [&](int32_t a, int32_t b) { return key[a] < key[b]; });
        int32_t mid = start + span / 2;
        const int32_t left_idx = idx + 1, right_idx = idx + 1 + sizes_at(span / 2);
        e.skip = idx + sizes_at(span);
        entries[idx] = e;
        if (depth < 4 && span >= (1 << 15)) {   // the two halves touch disjoint ranges of `order` and `entries`
            std::thread t([&] { build(start, mid, left_idx, depth + 1); });
            build(mid, end, right_idx, depth + 1);
            t.join();
        } else {
            build(start, mid, left_idx, depth + 1);
            build(mid, end, right_idx, depth + 1);
        }
    }
    int32_t sizes_at(int32_t span) const {   // read-only after build_root filled the table (thread-safe)
        if (span <= 2) return span > 0 ? 1 : 0;
        return sizes.at(span);
    }

};

// DFS pre-order -> level order with explicit links.  In pre-order the left child of inner entry i is
// i + 1 and `skip` already names the next wrapper after the subtree; storing the tree level by level
// (stable in DFS order within a level) puts the top of the tree first, which is what a partial LDS
// copy wants.  The walk order is unchanged: it follows the links, not the storage order.
template <typename real>
void relayout_bfs(std::vector<Entry<real>>& entries, std::vector<int32_t>& level_begin, std::vector<int8_t>* axis = nullptr) {
    const int32_t n = (int32_t)entries.size();
    level_begin.assign(1, 0);
    if (n == 0) return;
    std::vector<int32_t> level(n, 0), order_idx(n), new_of(n + 1);
    std::vector<int32_t> stack_end;   // ends (skip) of the enclosing inner wrappers
    for (int32_t i = 0; i < n; i++) {
        while (!stack_end.empty() && stack_end.back() <= i) stack_end.pop_back();
        level[i] = (int32_t)stack_end.size();
        if (entries[i].leaf < 0) stack_end.push_back(entries[i].skip);
    }
    for (int32_t i = 0; i < n; i++) order_idx[i] = i;
    std::stable_sort(order_idx.begin(), order_idx.end(), [&](int32_t a, int32_t b) { return level[a] < level[b]; });
    for (int32_t k = 0; k < n; k++) new_of[order_idx[k]] = k;
    new_of[n] = n;
    for (int32_t k = 1; k < n; k++) if (level[order_idx[k]] != level[order_idx[k - 1]]) level_begin.push_back(k);
    level_begin.push_back(n);
    std::vector<Entry<real>> out(n);
    for (int32_t k = 0; k < n; k++) {
        const int32_t i = order_idx[k];
        Entry<real> e = entries[i];
        e.skip = new_of[e.skip];
        if (e.leaf < 0) e.leaf = -new_of[i + 1];   // left child
        out[k] = e;
    }
    entries.swap(out);
    if (axis && !axis->empty()) {
        std::vector<int8_t> ax(n);
        for (int32_t k = 0; k < n; k++) ax[k] = (*axis)[order_idx[k]];
        axis->swap(ax);
    }
}

// SURVEY 8(f) row 1 -- CR_BVH_SAH: a binned surface-area-heuristic builder (16 bins per axis on the
// primitive-box centroids, all three axes tried, cost = area_L * n_L + area_R * n_R) instead of the
// reference's median split.  It emits the same wrapper array (boxes = union of the range's primitive boxes,
// leaves of one or two primitives, walked left then right with the shrinking interval), so the kernels and
// BVHWrapper::hit's semantics are unchanged; only the topology differs.  Decisions are made in f64 from the
// `real` boxes and are deterministic (stable partition, fixed tie-breaks), so cr_export_bvh reproduces the
// tree for a checker.
template <typename real> struct SahBuilder {
    const std::vector<real>* bmin;   // [3]
    const std::vector<real>* bmax;   // [3]
    std::vector<int32_t>* order;
    struct Node { real b[6]; int32_t left, right, start, end, axis; };
    std::vector<Node> nodes;
    std::atomic<int32_t> next{0};
    static constexpr int kBins = 16;

    static double area(const double lo[3], const double hi[3]) {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }

    // Bin of t = (cen - clo) * (kBins / ext), clamped in floating point BEFORE the conversion: when ext is so small that
    // kBins / ext overflows, t is inf, or 0 * inf = NaN for the centroid at clo, and converting either to int is undefined.
    // t >= kBins (inf included) is the last bin, anything that is not >= 0 (NaN included) the first.
    static int bin_of(double t) { return t >= (double)kBins ? kBins - 1 : (t >= 0.0 ? (int)t : 0); }

    void build_root(int32_t n) {
        nodes.assign((size_t)std::max(1, 2 * n), Node());
        next = 1;
        build(0, 0, n, 0);
    }

    void build(int32_t ni, int32_t start, int32_t end, int depth) {
        std::vector<int32_t>& ord = *order;
        Node nd;
        nd.left = nd.right = -1; nd.start = start; nd.end = end; nd.axis = 0;
        real lo[3], hi[3];
        double clo[3], chi[3];
        for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); clo[a] = INFINITY; chi[a] = -INFINITY; }
        for (int32_t i = start; i < end; i++) {
            const int32_t p = ord[i];
            for (int a = 0; a < 3; a++) {
                lo[a] = lo[a] <= bmin[a][p] ? lo[a] : bmin[a][p];
                hi[a] = hi[a] >= bmax[a][p] ? hi[a] : bmax[a][p];
                const double cen = 0.5 * ((double)bmin[a][p] + (double)bmax[a][p]);
                clo[a] = std::min(clo[a], cen); chi[a] = std::max(chi[a], cen);
            }
        }
        nd.b[0] = lo[0]; nd.b[1] = hi[0]; nd.b[2] = lo[1]; nd.b[3] = hi[1]; nd.b[4] = lo[2]; nd.b[5] = hi[2];
        const int32_t span = end - start;
        if (span <= 2) { nodes[ni] = nd; return; }

        int best_axis = -1, best_plane = -1;
        double best_cost = INFINITY;
        for (int a = 0; a < 3; a++) {
            const double ext = chi[a] - clo[a];
            if (!(ext > 0.0) || !std::isfinite(ext)) continue;
            const double scale = (double)kBins / ext;
            int32_t cnt[kBins] = {0};
            double blo[kBins][3], bhi[kBins][3];
            for (int k = 0; k < kBins; k++) for (int d = 0; d < 3; d++) { blo[k][d] = INFINITY; bhi[k][d] = -INFINITY; }
            for (int32_t i = start; i < end; i++) {
                const int32_t p = ord[i];
                const double cen = 0.5 * ((double)bmin[a][p] + (double)bmax[a][p]);
                const int k = bin_of((cen - clo[a]) * scale);
                cnt[k]++;
                for (int d = 0; d < 3; d++) { blo[k][d] = std::min(blo[k][d], (double)bmin[d][p]); bhi[k][d] = std::max(bhi[k][d], (double)bmax[d][p]); }
            }
            double r_area[kBins];
            int32_t r_cnt[kBins];
            {   // suffix sweep: everything in bins k..end
                double l3[3] = {INFINITY, INFINITY, INFINITY}, h3[3] = {-INFINITY, -INFINITY, -INFINITY};
                int32_t c = 0;
                for (int k = kBins - 1; k >= 1; k--) {
                    if (cnt[k]) for (int d = 0; d < 3; d++) { l3[d] = std::min(l3[d], blo[k][d]); h3[d] = std::max(h3[d], bhi[k][d]); }
                    c += cnt[k];
                    r_cnt[k] = c; r_area[k] = c ? area(l3, h3) : 0.0;
                }
            }
            double l3[3] = {INFINITY, INFINITY, INFINITY}, h3[3] = {-INFINITY, -INFINITY, -INFINITY};
            int32_t c = 0;
            for (int k = 0; k + 1 < kBins; k++) {   // plane k: bins 0..k | k+1..end
                if (cnt[k]) for (int d = 0; d < 3; d++) { l3[d] = std::min(l3[d], blo[k][d]); h3[d] = std::max(h3[d], bhi[k][d]); }
                c += cnt[k];
                if (c == 0 || r_cnt[k + 1] == 0) continue;
                const double cost = area(l3, h3) * (double)c + r_area[k + 1] * (double)r_cnt[k + 1];
                if (cost < best_cost) { best_cost = cost; best_axis = a; best_plane = k; }
            }
        }
        int32_t mid;
        if (best_axis < 0) mid = start + span / 2;   // coincident centroids (or non-finite extents): split the list
        else {
            const int a = best_axis;
            const double scale = (double)kBins / (chi[a] - clo[a]);
            auto it = std::stable_partition(ord.begin() + start, ord.begin() + end, [&](int32_t p) {
                const double cen = 0.5 * ((double)bmin[a][p] + (double)bmax[a][p]);
                return bin_of((cen - clo[a]) * scale) <= best_plane;
            });
            mid = (int32_t)(it - ord.begin());
        }
        nd.left = next.fetch_add(2);
        nd.right = nd.left + 1;
        nd.axis = best_axis < 0 ? 0 : best_axis;   // the left child holds the lower centroids along this axis
        nodes[ni] = nd;
        if (depth < 4 && span >= (1 << 15)) {   // the halves touch disjoint ranges of `order` and distinct nodes
            std::thread t([&] { build(nd.left, start, mid, depth + 1); });
            build(nd.right, mid, end, depth + 1);
            t.join();
        } else {
            build(nd.left, start, mid, depth + 1);
            build(nd.right, mid, end, depth + 1);
        }
    }

    // Node graph -> pre-order wrapper array with skip links (the layout Builder emits).
    void linearise(std::vector<Entry<real>>& out, std::vector<int8_t>& axis) const {
        out.clear(); axis.clear();
        std::vector<int32_t> stack{0}, open;   // open: pre-order indices of inner wrappers awaiting their end
        std::vector<std::pair<int32_t, int32_t>> todo;   // (node, pre-order index of the parent) -- iterative DFS
        struct Frame { int32_t node; int32_t state; int32_t idx; };
        std::vector<Frame> fr{{0, 0, -1}};
        while (!fr.empty()) {
            Frame& f = fr.back();
            const Node& nd = nodes[f.node];
            if (f.state == 0) {
                f.idx = (int32_t)out.size();
                Entry<real> e;
                for (int k = 0; k < 6; k++) e.b[k] = nd.b[k];
                e.skip = f.idx + 1; e.leaf = -1;
                if (nd.left < 0) { e.leaf = (nd.start << 1) | (nd.end - nd.start - 1); out.push_back(e); axis.push_back(-1); fr.pop_back(); continue; }
                out.push_back(e); axis.push_back((int8_t)nd.axis);
                f.state = 1;
                fr.push_back({nd.left, 0, -1});
            } else if (f.state == 1) {
                f.state = 2;
                fr.push_back({nd.right, 0, -1});
            } else {
                out[f.idx].skip = (int32_t)out.size();
                fr.pop_back();
            }
        }
    }
};

// CR_BVH_LBVH (lbvh.hpp): keys, sort and topology on the device; the node graph is then numbered into the
// level-order wrapper array (one primitive per leaf wrapper -- pairing sibling leaves measured slower: both
// primitives get tested on every visit; boxes are filled in later by run_box_kernels).  `order` receives the primitives' sorted order.
template <typename real>
int32_t build_lbvh(CrHandle* h, const std::vector<Prim<real>>& src, const std::vector<real>* bmin, const std::vector<real>* bmax,
                   std::vector<int32_t>& order, std::vector<Entry<real>>& entries, std::vector<int32_t>& level_begin) {
    const int32_t n = (int32_t)src.size();
    entries.clear();
    level_begin.assign(1, 0);
    if (n == 0) return CR_OK;
    LbvhBounds bnd;
    for (int a = 0; a < 3; a++) {
        double lo = INFINITY, hi = -INFINITY;
        for (int32_t i = 0; i < n; i++) {
            const double cen = 0.5 * ((double)bmin[a][i] + (double)bmax[a][i]);
            lo = std::min(lo, cen); hi = std::max(hi, cen);
        }
        bnd.lo[a] = std::isfinite(lo) ? lo : 0.0;
        bnd.inv_ext[a] = (std::isfinite(hi - lo) && hi > lo) ? 1.0 / (hi - lo) : 0.0;
    }
    DevBuf d_src, d_keys, d_keys2, d_idx, d_idx2, d_tmp, d_children;
    auto cleanup = [&] { d_src.release(); d_keys.release(); d_keys2.release(); d_idx.release(); d_idx2.release(); d_tmp.release(); d_children.release(); };
#define LBVH_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(h, CR_ERR_HIP, hipGetErrorString(e_)); } } while (0)
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
    cleanup();
    // node graph -> level-order wrappers with links (what relayout_bfs would produce from a pre-order array), in one
    // breadth-first pass: a child < 0 is ~(sorted position of a primitive); siblings get adjacent indices
    const int32_t total = 2 * n - 1;
    entries.assign((size_t)total, Entry<real>());
    level_begin.assign(1, 0);
    if (n == 1) { entries[0].leaf = 0; entries[0].skip = 1; level_begin.push_back(1); return CR_OK; }
    std::vector<int32_t> ref((size_t)total);   // node reference (as in `children`) of each new index
    ref[0] = 0;
    entries[0].skip = total;
    int32_t level_first = 0, level_end = 1, next = 1;
    std::vector<char> seen((size_t)(n - 1), 0);
    while (level_first < level_end) {
        for (int32_t k = level_first; k < level_end; k++) {
            const int32_t r = ref[k];
            Entry<real>& e = entries[k];
            if (r < 0) { e.leaf = (~r) << 1; continue; }              // one primitive
            if (r >= n - 1 || seen[r] || next + 2 > total) return fail(h, CR_ERR_HIP, "LBVH: malformed topology from the device");
            seen[r] = 1;
            const int32_t cl = children[2 * r], cr = children[2 * r + 1];
            if ((cl < 0 && ~cl >= n) || (cr < 0 && ~cr >= n)) return fail(h, CR_ERR_HIP, "LBVH: malformed topology from the device");
            e.leaf = -next;
            ref[next] = cl; ref[next + 1] = cr;
            entries[next].skip = next + 1;                            // after the left subtree comes the right child
            entries[next + 1].skip = e.skip;                          // after the right subtree: whatever follows the parent
            next += 2;
        }
        level_first = level_end; level_end = next;
        level_begin.push_back(level_first);
    }
    entries.resize((size_t)next);
    for (Entry<real>& e : entries) if (e.skip == total) e.skip = next;   // "no wrapper follows" = the final count
    if (level_begin.back() != next) level_begin.push_back(next);
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
    SahBuilder<real> sb;
    sb.bmin = bmin; sb.bmax = bmax; sb.order = &order;
    if (on_device) {
        std::vector<SahNodeRec> graph;
        int32_t rc;
        if (resident) rc = build_sah_device_resident(h, n, graph, order, dev_stats);
        else {
            std::vector<double> box6((size_t)n * 6);
            for (int32_t i = 0; i < n; i++) for (int a = 0; a < 3; a++) { box6[(size_t)i * 6 + a] = (double)bmin[a][i]; box6[(size_t)i * 6 + 3 + a] = (double)bmax[a][i]; }
            rc = build_sah_device(h, box6.data(), n, graph, order, dev_stats);
        }
        if (rc != CR_OK) return rc;
        sb.nodes.assign(graph.size(), typename SahBuilder<real>::Node());
        for (size_t i = 0; i < graph.size(); i++) {
            typename SahBuilder<real>::Node& nd = sb.nodes[i];
            nd.left = graph[i].left < 0 ? -1 : graph[i].left; nd.right = graph[i].left < 0 ? -1 : graph[i].left + 1;
            nd.start = graph[i].start; nd.end = graph[i].end; nd.axis = graph[i].axis;
        }
    } else sb.build_root(n);
    sb.linearise(entries, axis);
    relayout_bfs(entries, level_begin, &axis);
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
    if (ds.ordered) {   // per-octant skip links, parents before children (level order)
        const int32_t ne = (int32_t)entries.size();
        std::vector<EntryO<real>> eo((size_t)ne);
        for (int32_t i = 0; i < ne; i++) {
            for (int k = 0; k < 6; k++) eo[i].b[k] = entries[i].b[k];
            eo[i].unused = 0;
            const int32_t leaf = entries[i].leaf;
            eo[i].leaf = leaf < 0 ? -((-leaf) * 4 + axis[i]) : leaf;
        }
        if (ne > 0) for (int o = 0; o < 8; o++) eo[0].skip[o] = ne;
        for (int32_t i = 0; i < ne; i++) {
            const int32_t leaf = entries[i].leaf;
            if (leaf >= 0) continue;
            const int32_t left = -leaf;
            for (int o = 0; o < 8; o++) {
                const int32_t nearc = left + ((o >> axis[i]) & 1), farc = left + 1 - ((o >> axis[i]) & 1);
                eo[nearc].skip[o] = farc;
                eo[farc].skip[o] = eo[i].skip[o];
            }
        }
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
    if (ds.n_entries > 0) {
        int32_t rc = make_screen(h, ds, ds.entries.p, ds.screen, &ds.screen_usable);
        if (rc != CR_OK) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else ds.screen.release();
    return CR_OK;
}

template <typename real> int32_t build_dev_scene(CrHandle* h) {
    DevScene<real>& ds = dev_scene<real>(h);
    if (ds.built) return CR_OK;
    auto t_begin = std::chrono::steady_clock::now();
    const bool timing = getenv("CRUCIBLE_BUILD_TIMING") != nullptr;
    auto lap = [&](const char* what) { if (timing) fprintf(stderr, "[build] %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); };
    // The objects the BVH build sees, in list order (bvhwrapper.rs:16-26): visible spheres and triangles, and every
    // list whatever it holds.  Under the opt-in trees a list's visible objects stand in for it.
    struct Obj { int32_t desc, first, count, inner; };   // count < 0: a primitive; inner >= 0: a BVHWrapper element (index into `inners`)
    const bool ref_tree = h->bvh_mode == CR_BVH_REFERENCE;
    std::vector<Obj> objs;
    std::vector<std::vector<int32_t>> inner_members;   // per BVHWrapper element: its visible objects (descriptor indices)
    for (size_t i = 0; i < h->prims.size(); i++) {
        const CrPrimitive& p = h->prims[i];
        if (p.flags & CR_PRIM_MEMBER) continue;
        if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) {
            const int32_t first = (int32_t)p.v[0], count = (int32_t)p.v[1];
            if (!ref_tree) { for (int32_t k = first; k < first + count; k++) if (!(h->prims[k].flags & CR_PRIM_HIDDEN)) objs.push_back({k, 0, -1, -1}); continue; }
            if (p.kind == CR_PRIM_LIST) { objs.push_back({(int32_t)i, first, count, -1}); continue; }
            std::vector<int32_t> vis;   // new_wrapper drops the hidden objects (bvhwrapper.rs:16-26)
            for (int32_t k = first; k < first + count; k++) if (!(h->prims[k].flags & CR_PRIM_HIDDEN)) vis.push_back(k);
            if (vis.empty()) { objs.push_back({(int32_t)i, first, 0, -1}); continue; }   // ... and returns an empty list for none (:28-30)
            objs.push_back({(int32_t)i, first, count, (int32_t)inner_members.size()});
            inner_members.push_back(std::move(vis));
        } else if (!(p.flags & CR_PRIM_HIDDEN)) objs.push_back({(int32_t)i, 0, -1, -1});
    }
    const int32_t n = (int32_t)objs.size();
    Builder<real> b;
    for (int a = 0; a < 3; a++) { b.bmin[a].resize(n); b.bmax[a].resize(n); }
    b.order.resize(n);
    std::vector<Prim<real>> src(n);
    bool any_keys = false, any_lists = false;
    ds.has_triangles = false; ds.has_spheres = false;
    auto make_prim = [&](const CrPrimitive& p) {
        const Prim<real> q = pack_prim<real>(p);
        any_keys |= p.key_count > 0;
        ds.has_triangles |= p.kind == CR_PRIM_TRIANGLE;
        ds.has_spheres |= p.kind == CR_PRIM_SPHERE;
        return q;
    };
    auto prim_box = [](const Prim<real>& q, real lo[3], real hi[3]) {
        if (q.kind() == CR_PRIM_SPHERE) {   // Sphere::new, sphere.rs:29-30; Aabb::new_from_points bvh.rs:44-64
            const real r = q.g[3];
            for (int a = 0; a < 3; a++) {
                const real l = q.g[a] + (-r), u = q.g[a] + r;
                if (l <= u) { lo[a] = l; hi[a] = u; } else { lo[a] = u; hi[a] = l; }
            }
        } else {                            // Triangle::new, triangle.rs:28-35 (f64::min/max)
            for (int a = 0; a < 3; a++) {
                hi[a] = std::fmax(q.g[a], std::fmax(q.g[3 + a], q.g[6 + a]));
                lo[a] = std::fmin(q.g[a], std::fmin(q.g[3 + a], q.g[6 + a]));
            }
        }
    };
    // BVHWrapper elements: the inner trees, by the reference's own build over their visible objects
    std::vector<Builder<real>> inners(inner_members.size());
    std::vector<std::vector<Prim<real>>> inner_src(inner_members.size());
    for (size_t w = 0; w < inners.size(); w++) {
        const std::vector<int32_t>& mem = inner_members[w];
        const int32_t m = (int32_t)mem.size();
        Builder<real>& ib = inners[w];
        for (int a = 0; a < 3; a++) { ib.bmin[a].resize(m); ib.bmax[a].resize(m); }
        ib.order.resize(m);
        inner_src[w].resize(m);
        for (int32_t k = 0; k < m; k++) {
            inner_src[w][k] = make_prim(h->prims[mem[k]]);
            real lo[3], hi[3];
            prim_box(inner_src[w][k], lo, hi);
            for (int a = 0; a < 3; a++) { ib.bmin[a][k] = lo[a]; ib.bmax[a][k] = hi[a]; }
            ib.order[k] = k;
        }
        ib.build_root(m);
    }
    for (int32_t i = 0; i < n; i++) {
        const Obj& o = objs[i];
        b.order[i] = i;
        real lo[3], hi[3];
        if (o.count < 0) {
            src[i] = make_prim(h->prims[o.desc]);
            prim_box(src[i], lo, hi);
        } else if (o.inner >= 0) {   // the wrapper's box: its root's (new_from_vec, bvhwrapper.rs:39)
            const Entry<real>& root = inners[o.inner].entries[0];
            for (int a = 0; a < 3; a++) { lo[a] = root.b[2 * a]; hi[a] = root.b[2 * a + 1]; }
        } else {   // HitList: Aabb::default() (hitlist.rs:13-18), grown by add() over every object, hidden or not (hitlist.rs:24-27)
            any_lists = true;
            for (int a = 0; a < 3; a++) { lo[a] = std::numeric_limits<real>::infinity(); hi[a] = -std::numeric_limits<real>::infinity(); }
            if (!(h->prims[o.desc].flags & CR_LIST_EMPTY_BOX))
                for (int32_t k = o.first; k < o.first + o.count; k++) {
                    CrPrimitive m = h->prims[k];
                    Prim<real> q;
                    for (int j = 0; j < 9; j++) q.g[j] = (real)m.v[j];
                    q.kind_mat = m.kind & 1;
                    real ml[3], mh[3];
                    prim_box(q, ml, mh);
                    for (int a = 0; a < 3; a++) {   // Interval::tight_enclose, utils.rs:631-635
                        lo[a] = lo[a] <= ml[a] ? lo[a] : ml[a];
                        hi[a] = hi[a] >= mh[a] ? hi[a] : mh[a];
                    }
                }
        }
        for (int a = 0; a < 3; a++) { b.bmin[a][i] = lo[a]; b.bmax[a][i] = hi[a]; }
    }
    std::vector<int8_t> axis;
    struct Run { int32_t first, count; bool pseudo; };
    std::vector<Run> spliced_runs;              // scenes with a BVHWrapper element: the primitive run of every leaf record
    std::vector<Prim<real>> spliced_prims;      // ... and the primitive records in the order the runs name them
    bool spliced = false;
    ds.ordered = h->bvh_mode == CR_BVH_SAH_ORDERED;
    lap("primitive records and boxes");
    const auto t_tree = std::chrono::steady_clock::now();
    const bool lbvh = h->bvh_mode == CR_BVH_LBVH;
    const bool sah_device = h->bvh_device && (h->bvh_mode == CR_BVH_SAH || h->bvh_mode == CR_BVH_SAH_ORDERED);
    bool device_boxes = lbvh;   // the wrapper boxes are filled in on the device after the upload
    SahDeviceStats dev_stats;
    if (lbvh) {
        int32_t rc = build_lbvh<real>(h, src, b.bmin, b.bmax, b.order, b.entries, ds.level_begin);
        if (rc != CR_OK) return rc;
    } else if (n > 0 && h->bvh_mode != CR_BVH_REFERENCE) {
        int32_t rc = sah_tree<real>(h, b.bmin, b.bmax, n, sah_device && n >= 3, false, b.order, b.entries, axis, ds.level_begin, dev_stats);
        if (rc != CR_OK) return rc;
        device_boxes = sah_device && n >= 3;
    } else if (n > 0) {
        b.build_root(n);
        if (!inners.empty()) {
            // A leaf wrapper that holds a BVHWrapper element becomes an inner record: the element's own tree is spliced in
            // as one child; a primitive or list beside it becomes a record of its own with an empty box (which the box
            // test always passes, bvh.rs:96-130 -- BVHWrapper::hit tests that child without any box), and a span-1
            // wrapper (the element twice, bvhwrapper.rs:56-58) gets an empty record as its second child: the second walk
            // of the same tree cannot find anything closer.  Every leaf names its primitive run through `runs`.
            std::vector<Entry<real>> sp;
            std::function<void(int32_t)> emit;
            auto new_run = [&](int32_t first, int32_t count, bool pseudo) { spliced_runs.push_back({first, count, pseudo}); return (int32_t)spliced_runs.size() - 1; };
            auto append_obj = [&](const Obj& o, int32_t order_pos) {
                if (o.count < 0) spliced_prims.push_back(src[order_pos]);
                else for (int32_t k = o.first; k < o.first + o.count; k++) if (!(h->prims[k].flags & CR_PRIM_HIDDEN)) spliced_prims.push_back(make_prim(h->prims[k]));
            };
            const real inf = std::numeric_limits<real>::infinity();
            auto pseudo_leaf = [&](int32_t first, int32_t count) {
                Entry<real> pe;
                for (int a = 0; a < 3; a++) { pe.b[2 * a] = inf; pe.b[2 * a + 1] = -inf; }
                pe.leaf = new_run(first, count, true);
                pe.skip = (int32_t)sp.size() + 1;
                sp.push_back(pe);
            };
            emit = [&](int32_t i) {
                const Entry<real> e = b.entries[i];
                const int32_t idx = (int32_t)sp.size();
                sp.push_back(e);
                if (e.leaf < 0) { emit(i + 1); emit(b.entries[i + 1].skip); sp[idx].skip = (int32_t)sp.size(); return; }
                const int32_t start = e.leaf >> 1, span = (e.leaf & 1) + 1;
                bool any_inner = false;
                for (int32_t k = 0; k < span; k++) any_inner |= objs[b.order[start + k]].inner >= 0;
                if (!any_inner) {
                    const int32_t first = (int32_t)spliced_prims.size();
                    for (int32_t k = 0; k < span; k++) append_obj(objs[b.order[start + k]], b.order[start + k]);
                    sp[idx].leaf = new_run(first, (int32_t)spliced_prims.size() - first, false);
                    sp[idx].skip = idx + 1;
                    return;
                }
                sp[idx].leaf = -1;
                for (int32_t k = 0; k < span; k++) {
                    const Obj& o = objs[b.order[start + k]];
                    if (o.inner < 0) {
                        const int32_t first = (int32_t)spliced_prims.size();
                        append_obj(o, b.order[start + k]);
                        pseudo_leaf(first, (int32_t)spliced_prims.size() - first);
                        continue;
                    }
                    const Builder<real>& ib = inners[o.inner];
                    const int32_t base = (int32_t)sp.size();
                    for (const Entry<real>& ie : ib.entries) {
                        Entry<real> c = ie;
                        c.skip += base;
                        if (c.leaf >= 0) {
                            const int32_t s0 = c.leaf >> 1, cnt = (c.leaf & 1) + 1, first = (int32_t)spliced_prims.size();
                            for (int32_t q = 0; q < cnt; q++) spliced_prims.push_back(inner_src[o.inner][ib.order[s0 + q]]);
                            c.leaf = new_run(first, cnt, false);
                        }
                        sp.push_back(c);
                    }
                }
                if (span == 1) pseudo_leaf((int32_t)spliced_prims.size(), 0);
                sp[idx].skip = (int32_t)sp.size();
            };
            emit(0);
            b.entries.swap(sp);
            spliced = true;
        }
        relayout_bfs(b.entries, ds.level_begin);
    }
    else ds.level_begin.assign(1, 0);
    lap("tree");
    const double tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tree).count();
    // Primitive records in leaf order; a list contributes its visible objects in the list's order (a hidden object
    // returns no hit before anything is computed: sphere.rs:62, triangle.rs:87).
    std::vector<Prim<real>> leaf_prims;
    leaf_prims.reserve(n);
    std::vector<int32_t> first_of((size_t)n + 1);
    if (spliced) leaf_prims.swap(spliced_prims);
    else for (int32_t i = 0; i < n; i++) {
        const Obj& o = objs[b.order[i]];
        first_of[i] = (int32_t)leaf_prims.size();
        if (o.count < 0) leaf_prims.push_back(src[b.order[i]]);
        else for (int32_t k = o.first; k < o.first + o.count; k++) if (!(h->prims[k].flags & CR_PRIM_HIDDEN)) leaf_prims.push_back(make_prim(h->prims[k]));
    }
    if (!spliced) first_of[n] = (int32_t)leaf_prims.size();
    if (leaf_prims.size() >= ((size_t)1 << 29)) return fail(h, CR_ERR_INVALID_ARG, "too many primitives");
    // What the device walks: a leaf wrapper names a run of primitive records.  One or two records fit the wrapper
    // itself; a leaf that holds a list names its run through the side table (first, count).
    std::vector<Entry<real>> dev_entries;
    std::vector<int32_t> leaf_runs;
    if (spliced) {
        dev_entries = b.entries;
        for (Entry<real>& e : dev_entries) {
            if (e.leaf < 0) continue;
            const Run r = spliced_runs[e.leaf];
            if (!r.pseudo && (r.count == 1 || r.count == 2)) e.leaf = (r.first << 1) | (r.count - 1);
            else { e.leaf = kLeafRun | (r.pseudo ? kLeafPseudo : 0) | (int32_t)(leaf_runs.size() / 2); leaf_runs.push_back(r.first); leaf_runs.push_back(r.count); }
        }
    } else if (any_lists) {
        dev_entries = b.entries;
        for (Entry<real>& e : dev_entries) {
            if (e.leaf < 0) continue;
            const int32_t start = e.leaf >> 1, span = (e.leaf & 1) + 1;
            const int32_t first = first_of[start], count = first_of[start + span] - first;
            if (count == 1 || count == 2) e.leaf = (first << 1) | (count - 1);
            else { e.leaf = kLeafRun | (int32_t)(leaf_runs.size() / 2); leaf_runs.push_back(first); leaf_runs.push_back(count); }
        }
    }
    const std::vector<Entry<real>>& up_entries = (any_lists || spliced) ? dev_entries : b.entries;

    // Device texture table, materials, textures and keyframes (pack.hpp)
    const std::vector<int32_t> tex_remap = live_texture_remap(h->materials.data(), h->materials.size(), h->textures.data(), h->textures.size());
    std::vector<Mat<real>> mats(h->materials.size());
    for (size_t i = 0; i < mats.size(); i++) mats[i] = pack_mat<real>(h->materials[i], h->textures.data(), tex_remap.data());
    std::vector<Tex<real>> texs;
    for (size_t i = 0; i < h->textures.size(); i++)
        if (tex_remap[i] >= 0) texs.push_back(pack_tex<real>(h->textures[i], tex_remap.data()));
    std::vector<Key<real>> keys(h->keys.size());
    if (!keys.empty()) memset(keys.data(), 0, keys.size() * sizeof(Key<real>));
    for (size_t i = 0; i < h->keys.size(); i++) key_to_real(h->keys[i], keys[i]);

    { int32_t rc = upload_entries<real>(h, ds, b.entries, up_entries, axis); if (rc != CR_OK) return rc; }
    HIP_TRY(h, upload(ds.leaf_runs, leaf_runs.data(), leaf_runs.size() * sizeof(int32_t)));
    ds.has_leaf_runs = !leaf_runs.empty();
    ds.has_lists = any_lists;
    HIP_TRY(h, upload(ds.prims, leaf_prims.data(), leaf_prims.size() * sizeof(Prim<real>)));
    if (!ds.side_tables) {   // a rebuild after cr_update_primitives: these still hold the uploaded scene's
        HIP_TRY(h, upload(ds.mats, mats.data(), mats.size() * sizeof(Mat<real>)));
        HIP_TRY(h, upload(ds.texs, texs.data(), texs.size() * sizeof(Tex<real>)));
        HIP_TRY(h, upload(ds.keys, keys.data(), keys.size() * sizeof(Key<real>)));
        ds.side_tables = true;
    }
    ds.desc_pos_valid = !any_lists && !spliced && !h->has_list_elements;
    if (ds.desc_pos_valid) {   // every object is one primitive: record i of leaf_prims is objs[b.order[i]]
        std::vector<int32_t> pos(h->prims.size(), -1);
        for (int32_t i = 0; i < n; i++) pos[(size_t)objs[b.order[i]].desc] = i;
        HIP_TRY(h, upload(ds.desc_pos, pos.data(), pos.size() * sizeof(int32_t)));
    }
    ds.n_entries = (int32_t)b.entries.size(); ds.n_prims = (int32_t)leaf_prims.size(); ds.n_mats = (int32_t)mats.size(); ds.n_texs = (int32_t)texs.size();
    ds.n_scene_keys = (int32_t)h->keys.size();
    ds.lds_bytes = r16(b.entries.size() * ds.entry_bytes) + r16(leaf_prims.size() * sizeof(Prim<real>)) +
                   r16(mats.size() * sizeof(Mat<real>)) + r16(texs.size() * sizeof(Tex<real>));
    ds.animated = any_keys;
    // device builders: the construction-time primitive boxes, bottom-up, on the device; then the screening records
    { int32_t rc = finish_boxes<real>(h, ds, b.entries, device_boxes, real(0), real(0), false); if (rc != CR_OK) return rc; }
    lap("uploads and boxes");
    ds.host_entries = b.entries;
    ds.host_axis = axis;
    ds.leaf_desc.resize(n);
    for (int32_t i = 0; i < n; i++) ds.leaf_desc[i] = objs[b.order[i]].desc;
    ds.in_desc.resize(n);
    for (int32_t i = 0; i < n; i++) ds.in_desc[i] = objs[i].desc;
    ds.base_order = b.order;
    frame_scene<real>(h).frame_valid = false;   // built from the tree this one replaces
    frame_scene<real>(h).info = CrBuildInfo();
    ds.last_walk = kWalkNone;
    ds.has_bvh_elements = spliced;
    ds.built = true;
    ds.info = CrBuildInfo();
    ds.info.bvh_mode = h->bvh_mode;
    ds.info.built_on_device = (lbvh || (sah_device && n >= 3)) ? 1 : 0;   // fewer than 3 primitives are one leaf, written on the host
    ds.info.n_wrappers = ds.n_entries;
    ds.info.device_rounds = dev_stats.rounds; ds.info.large_nodes = dev_stats.large_nodes;
    ds.info.small_subtrees = dev_stats.small_subtrees; ds.info.small_threshold = dev_stats.small_threshold;
    ds.info.tree_ms = tree_ms;
    ds.info.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    h->upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return CR_OK;
}

// cr_export_bvh: the wrapper tree the device walks, re-expressed as the reference's BVHWrapper tree (each
// wrapper = box + left/right child) in walk order.  A leaf wrapper of one primitive holds it twice, as the
// reference's span-1 wrappers do (bvhwrapper.rs:58-60).
template <typename real>
int32_t export_tree(CrHandle* h, const DevScene<real>& ds, const std::vector<Entry<real>>& E, const char* what, double* boxes, int32_t* children,
                    int32_t* split_axis, int32_t capacity, int32_t* n_out) {
    if (ds.has_bvh_elements) return fail(h, CR_ERR_UNSUPPORTED, std::string(what) + ": the scene holds a BVHWrapper element (CR_BVH_REFERENCE): its records are not two-children wrappers");
    *n_out = (int32_t)E.size();
    if (!boxes || !children || capacity < (int32_t)E.size()) return E.empty() || (!boxes && !children) ? CR_OK : fail(h, CR_ERR_INVALID_ARG, std::string(what) + ": capacity too small");
    if (E.empty()) return CR_OK;
    struct Frame { int32_t entry, out, state; };
    std::vector<Frame> fr{{0, -1, 0}};
    int32_t n = 0;
    while (!fr.empty()) {
        Frame& f = fr.back();
        const Entry<real>& e = E[f.entry];
        if (f.state == 0) {
            f.out = n++;
            for (int k = 0; k < 6; k++) boxes[6 * f.out + k] = (double)e.b[k];
            if (split_axis) split_axis[f.out] = (ds.ordered && e.leaf < 0) ? (int32_t)ds.host_axis[f.entry] : -1;
            if (e.leaf >= 0) {
                const int32_t first = e.leaf >> 1, count = (e.leaf & 1) + 1;
                children[2 * f.out] = ~ds.leaf_desc[first];
                children[2 * f.out + 1] = ~ds.leaf_desc[first + count - 1];
                fr.pop_back();
                continue;
            }
            f.state = 1;
            children[2 * f.out] = n;                 // the left child is exported next
            const int32_t left = -e.leaf;
            fr.push_back({left, -1, 0});
        } else if (f.state == 1) {
            f.state = 2;
            children[2 * f.out + 1] = n;
            const int32_t right = E[-e.leaf].skip;   // the wrapper after the left subtree
            fr.push_back({right, -1, 0});
        } else fr.pop_back();
    }
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
    // the side tables are the base tree's (not owned: a DevBuf without an allocation of its own releases nothing)
    for (auto pr : {std::make_pair(&fs.mats, &base.mats), std::make_pair(&fs.texs, &base.texs), std::make_pair(&fs.keys, &base.keys)}) {
        pr.first->p = pr.second->p; pr.first->raw = nullptr; pr.first->bytes = pr.second->bytes; pr.first->pad = pr.second->pad;
    }
    fs.ordered = base.ordered; fs.animated = base.animated; fs.has_triangles = base.has_triangles; fs.has_spheres = base.has_spheres;
    fs.has_leaf_runs = false; fs.has_lists = false; fs.has_bvh_elements = false; fs.desc_pos_valid = false;
    fs.n_mats = base.n_mats; fs.n_texs = base.n_texs; fs.n_scene_keys = base.n_scene_keys;
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
    } else {           // the same rule on the host (CR_HD), from the handle's copy of the scene
        std::vector<Key<real>> keys(h->keys.size() + 1);
        memset(keys.data(), 0, keys.size() * sizeof(Key<real>));
        for (size_t i = 0; i < h->keys.size(); i++) key_to_real(h->keys[i], keys[i]);
        for (int a = 0; a < 3; a++) { bmin[a].resize(n); bmax[a].resize(n); }
        for (int32_t j = 0; j < n; j++) {
            const Prim<real> q = pack_prim<real>(h->prims[(size_t)base.in_desc[j]]);
            real lo[3], hi[3];
            for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
            prim_box_over(q, keys.data(), ta, tb, lo, hi, true);
            for (int a = 0; a < 3; a++) { bmin[a][j] = lo[a]; bmax[a][j] = hi[a]; }
        }
    }
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
    fs.lds_bytes = r16(entries.size() * fs.entry_bytes) + r16((size_t)n * sizeof(Prim<real>)) + r16((size_t)fs.n_mats * sizeof(Mat<real>)) + r16((size_t)fs.n_texs * sizeof(Tex<real>));
    // the boxes a refit gives this topology for [ta, tb], on the device for either builder; then the screening records
    rc = finish_boxes<real>(h, fs, entries, true, ta, tb, true);
    if (rc != CR_OK) return rc;
    fs.host_entries.swap(entries);
    fs.host_axis.swap(axis);
    fs.leaf_desc.resize(n);
    for (int32_t i = 0; i < n; i++) fs.leaf_desc[i] = base.in_desc[(size_t)order[i]];
    fs.built = true;
    fs.frame_valid = true; fs.frame_ta = ta; fs.frame_tb = tb;
    fs.info.bvh_mode = h->bvh_mode;
    fs.info.built_on_device = on_device ? 1 : 0;
    fs.info.n_wrappers = fs.n_entries;
    fs.info.device_rounds = dev_stats.rounds; fs.info.large_nodes = dev_stats.large_nodes;
    fs.info.small_subtrees = dev_stats.small_subtrees; fs.info.small_threshold = dev_stats.small_threshold;
    fs.info.tree_ms = tree_ms;
    fs.info.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
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
