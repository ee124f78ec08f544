// tree.hpp -- the host side of every tree this library builds, free of the HIP runtime: from the caller's primitive list to
// the wrapper records, the primitive order and the leaf runs that build.hip uploads, and back to the two-children tree
// cr_export_bvh returns.  Plain vectors in, plain vectors out; build.hip calls these functions stage by stage and adds the
// device work between them, and tests/tree_check.cpp compiles them with a plain C++ compiler and holds them to the models
// and the oracle (tests/test_tree_host.py), also under sanitizers.  Stages, in build_dev_scene's order:
//   scene_boxes       the objects the build sees, their records and construction-time boxes, the inner trees of BVHWrapper elements
//   host_topology     the topology where the host builds it, by the mode's builder:
//   reference_tree    CR_BVH_REFERENCE: Builder, the splice of inner trees, relayout_bfs
//   sah_host_tree     CR_BVH_SAH / CR_BVH_SAH_ORDERED on the host: SahBuilder, linearise, relayout_bfs
//   sah_graph_tree    ... from the node graph of the device builder (sah_device.hpp)
//   lbvh_bounds, lbvh_number   CR_BVH_LBVH: what the device's keys are normalised to; its node graph numbered level by level
//   layout_leaves     the primitive records in leaf order and the records that name runs of them
//   ordered_entries   CR_BVH_SAH_ORDERED: EntryO records with per-octant links
//   export_walk       the wrapper array re-expressed as the reference's BVHWrapper tree
#pragma once
#include "lbvh.hpp"
#include "pack.hpp"
#include "records.hpp"
#include "sah_device.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <map>
#include <thread>
#include <vector>

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

    // The node graph of the device builder (sah_device.hpp) in this builder's form; the boxes stay zero (run_box_kernels fills them in).
    void from_graph(const std::vector<SahNodeRec>& graph) {
        nodes.assign(graph.size(), Node());
        for (size_t i = 0; i < graph.size(); i++) {
            Node& nd = nodes[i];
            nd.left = graph[i].left < 0 ? -1 : graph[i].left; nd.right = graph[i].left < 0 ? -1 : graph[i].left + 1;
            nd.start = graph[i].start; nd.end = graph[i].end; nd.axis = graph[i].axis;
        }
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

// The CR_BVH_SAH / CR_BVH_SAH_ORDERED tree over n >= 1 primitive boxes, built on the host: the pre-order
// wrappers re-laid level by level, the split axes and the primitive order.
template <typename real>
void sah_host_tree(const std::vector<real>* bmin, const std::vector<real>* bmax, int32_t n, std::vector<int32_t>& order,
                   std::vector<Entry<real>>& entries, std::vector<int8_t>& axis, std::vector<int32_t>& level_begin) {
    SahBuilder<real> sb;
    sb.bmin = bmin; sb.bmax = bmax; sb.order = &order;
    sb.build_root(n);
    sb.linearise(entries, axis);
    relayout_bfs(entries, level_begin, &axis);
}
// ... from the node graph the device builder hands back (its primitive order is the caller's already; the boxes are not set)
template <typename real>
void sah_graph_tree(const std::vector<SahNodeRec>& graph, std::vector<Entry<real>>& entries, std::vector<int8_t>& axis, std::vector<int32_t>& level_begin) {
    SahBuilder<real> sb;
    sb.from_graph(graph);
    sb.linearise(entries, axis);
    relayout_bfs(entries, level_begin, &axis);
}

// ---------------------------------------------------------------- CR_BVH_LBVH (lbvh.hpp)
// What the device's Morton keys are normalised to: the bounds of the box midpoints of n primitives.
template <typename real> LbvhBounds lbvh_bounds(const std::vector<real>* bmin, const std::vector<real>* bmax, int32_t n) {
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
    return bnd;
}

// The node graph of n >= 1 sorted primitives (children: two per internal node, as lbvh_children gives them) -> level-order
// wrappers with links (what relayout_bfs would produce from a pre-order array), in one breadth-first pass: a child < 0 is
// ~(sorted position of a primitive); siblings get adjacent indices.  One primitive per leaf wrapper -- pairing sibling
// leaves measured slower: both primitives get tested on every visit; the boxes are left for run_box_kernels.  False for a
// graph that is no tree over those primitives (a reference out of range, a node reached twice): nothing is read out of bounds.
template <typename real>
bool lbvh_number(const std::vector<int32_t>& children, int32_t n, std::vector<Entry<real>>& entries, std::vector<int32_t>& level_begin) {
    const int32_t total = 2 * n - 1;
    entries.assign((size_t)total, Entry<real>());
    level_begin.assign(1, 0);
    if (n == 1) { entries[0].leaf = 0; entries[0].skip = 1; level_begin.push_back(1); return true; }
    if (children.size() < (size_t)2 * (size_t)(n - 1)) return false;
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
            if (r >= n - 1 || seen[r] || next + 2 > total) return false;
            seen[r] = 1;
            const int32_t cl = children[2 * r], cr = children[2 * r + 1];
            if ((cl < 0 && ~cl >= n) || (cr < 0 && ~cr >= n)) return false;
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
    return true;
}

// ---------------------------------------------------------------- CR_BVH_SAH_ORDERED
// The EntryO records of a level-order wrapper array: per-octant skip links, parents before children.
template <typename real>
std::vector<EntryO<real>> ordered_entries(const std::vector<Entry<real>>& entries, const std::vector<int8_t>& axis) {
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
    return eo;
}

// ---------------------------------------------------------------- objects and boxes
// An object the BVH build sees.  count < 0: a primitive; inner >= 0: a BVHWrapper element (index into SceneBoxes::inners)
struct Obj { int32_t desc, first, count, inner; };

// What the packed records of a scene hold (every record a build packs is counted, whichever stage packs it)
struct PrimKinds { bool any_keys = false, has_triangles = false, has_spheres = false; };

template <typename real> Prim<real> make_prim(const CrPrimitive& p, PrimKinds& kinds) {
    kinds.any_keys |= p.key_count > 0;
    kinds.has_triangles |= p.kind == CR_PRIM_TRIANGLE;
    kinds.has_spheres |= p.kind == CR_PRIM_SPHERE;
    return pack_prim<real>(p);
}

// The construction-time box of a primitive record
template <typename real> void prim_box(const Prim<real>& q, real lo[3], real hi[3]) {
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
}

// The box of a HitList element: Aabb::default() (hitlist.rs:13-18), grown by add() over every object, hidden or not (hitlist.rs:24-27)
template <typename real> void list_box(const std::vector<CrPrimitive>& prims, const Obj& o, real lo[3], real hi[3]) {
    for (int a = 0; a < 3; a++) { lo[a] = std::numeric_limits<real>::infinity(); hi[a] = -std::numeric_limits<real>::infinity(); }
    if (prims[o.desc].flags & CR_LIST_EMPTY_BOX) return;
    for (int32_t k = o.first; k < o.first + o.count; k++) {
        const CrPrimitive& m = prims[k];
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

// Stage 1: what the tree builders start from.
template <typename real> struct SceneBoxes {
    std::vector<Obj> objs;                              // the objects, in list order
    Builder<real> b;                                    // their boxes (bmin, bmax), order = identity; the builders fill the rest
    std::vector<Prim<real>> src;                        // the record of every object that is a primitive
    std::vector<Builder<real>> inners;                  // per BVHWrapper element: its own tree, by the reference's build
    std::vector<std::vector<Prim<real>>> inner_src;     // ... and the records of its visible objects
    PrimKinds kinds;
    bool any_lists = false;                             // some object is a HitList element
};

// The objects the BVH build sees, in list order (bvhwrapper.rs:16-26): visible spheres and triangles, and every
// list whatever it holds.  Under the opt-in trees (ref_tree = false) a list's visible objects stand in for it.
// inner_members: per BVHWrapper element, its visible objects (descriptor indices).
inline void list_objects(const std::vector<CrPrimitive>& prims, bool ref_tree, std::vector<Obj>& objs, std::vector<std::vector<int32_t>>& inner_members) {
    for (size_t i = 0; i < prims.size(); i++) {
        const CrPrimitive& p = prims[i];
        if (p.flags & CR_PRIM_MEMBER) continue;
        if (p.kind == CR_PRIM_LIST || p.kind == CR_PRIM_BVH) {
            const int32_t first = (int32_t)p.v[0], count = (int32_t)p.v[1];
            if (!ref_tree) { for (int32_t k = first; k < first + count; k++) if (!(prims[k].flags & CR_PRIM_HIDDEN)) objs.push_back({k, 0, -1, -1}); continue; }
            if (p.kind == CR_PRIM_LIST) { objs.push_back({(int32_t)i, first, count, -1}); continue; }
            std::vector<int32_t> vis;   // new_wrapper drops the hidden objects (bvhwrapper.rs:16-26)
            for (int32_t k = first; k < first + count; k++) if (!(prims[k].flags & CR_PRIM_HIDDEN)) vis.push_back(k);
            if (vis.empty()) { objs.push_back({(int32_t)i, first, 0, -1}); continue; }   // ... and returns an empty list for none (:28-30)
            objs.push_back({(int32_t)i, first, count, (int32_t)inner_members.size()});
            inner_members.push_back(std::move(vis));
        } else if (!(p.flags & CR_PRIM_HIDDEN)) objs.push_back({(int32_t)i, 0, -1, -1});
    }
}

template <typename real> void scene_boxes(const std::vector<CrPrimitive>& prims, bool ref_tree, SceneBoxes<real>& in) {
    std::vector<std::vector<int32_t>> inner_members;
    list_objects(prims, ref_tree, in.objs, inner_members);
    // BVHWrapper elements: the inner trees, by the reference's own build over their visible objects
    in.inners.resize(inner_members.size());
    in.inner_src.resize(inner_members.size());
    for (size_t w = 0; w < in.inners.size(); w++) {
        const std::vector<int32_t>& mem = inner_members[w];
        const int32_t m = (int32_t)mem.size();
        Builder<real>& ib = in.inners[w];
        for (int a = 0; a < 3; a++) { ib.bmin[a].resize(m); ib.bmax[a].resize(m); }
        ib.order.resize(m);
        in.inner_src[w].resize(m);
        for (int32_t k = 0; k < m; k++) {
            in.inner_src[w][k] = make_prim<real>(prims[mem[k]], in.kinds);
            real lo[3], hi[3];
            prim_box(in.inner_src[w][k], lo, hi);
            for (int a = 0; a < 3; a++) { ib.bmin[a][k] = lo[a]; ib.bmax[a][k] = hi[a]; }
            ib.order[k] = k;
        }
        ib.build_root(m);
    }
    const int32_t n = (int32_t)in.objs.size();
    Builder<real>& b = in.b;
    for (int a = 0; a < 3; a++) { b.bmin[a].resize(n); b.bmax[a].resize(n); }
    b.order.resize(n);
    in.src.resize(n);
    for (int32_t i = 0; i < n; i++) {
        const Obj& o = in.objs[i];
        b.order[i] = i;
        real lo[3], hi[3];
        if (o.count < 0) {
            in.src[i] = make_prim<real>(prims[o.desc], in.kinds);
            prim_box(in.src[i], lo, hi);
        } else if (o.inner >= 0) {   // the wrapper's box: its root's (new_from_vec, bvhwrapper.rs:39)
            const Entry<real>& root = in.inners[o.inner].entries[0];
            for (int a = 0; a < 3; a++) { lo[a] = root.b[2 * a]; hi[a] = root.b[2 * a + 1]; }
        } else {
            in.any_lists = true;
            list_box(prims, o, lo, hi);
        }
        for (int a = 0; a < 3; a++) { b.bmin[a][i] = lo[a]; b.bmax[a][i] = hi[a]; }
    }
}

// The primitive records of the object at position `pos` of the builder's input, appended to `out`: its own, or a list's
// visible objects in the list's order (a hidden object returns no hit before anything is computed: sphere.rs:62, triangle.rs:87).
template <typename real>
void append_object(const std::vector<CrPrimitive>& prims, SceneBoxes<real>& in, int32_t pos, std::vector<Prim<real>>& out) {
    const Obj& o = in.objs[pos];
    if (o.count < 0) out.push_back(in.src[pos]);
    else for (int32_t k = o.first; k < o.first + o.count; k++) if (!(prims[k].flags & CR_PRIM_HIDDEN)) out.push_back(make_prim<real>(prims[k], in.kinds));
}

// ---------------------------------------------------------------- the splice of inner trees (CR_BVH_REFERENCE)
// A leaf wrapper that holds a BVHWrapper element becomes an inner record: the element's own tree is spliced in
// as one child; a primitive or list beside it becomes a record of its own with an empty box (which the box
// test always passes, bvh.rs:96-130 -- BVHWrapper::hit tests that child without any box), and a span-1
// wrapper (the element twice, bvhwrapper.rs:56-58) gets an empty record as its second child: the second walk
// of the same tree cannot find anything closer.  Every leaf names its primitive run through `runs`.
struct Run { int32_t first, count; bool pseudo; };
template <typename real> struct Spliced {
    bool on = false;                    // the scene holds a BVHWrapper element: the records below replace the tree's own
    std::vector<Entry<real>> entries;   // pre-order; a leaf's `leaf` is an index into runs
    std::vector<Run> runs;              // the primitive run of every leaf record
    std::vector<Prim<real>> prims;      // the primitive records in the order the runs name them
};

template <typename real> int32_t splice_run(Spliced<real>& s, int32_t first, int32_t count, bool pseudo) {
    s.runs.push_back({first, count, pseudo});
    return (int32_t)s.runs.size() - 1;
}
template <typename real> void splice_pseudo_leaf(Spliced<real>& s, int32_t first, int32_t count) {
    const real inf = std::numeric_limits<real>::infinity();
    Entry<real> pe;
    for (int a = 0; a < 3; a++) { pe.b[2 * a] = inf; pe.b[2 * a + 1] = -inf; }
    pe.leaf = splice_run(s, first, count, true);
    pe.skip = (int32_t)s.entries.size() + 1;
    s.entries.push_back(pe);
}
// Record i of the pre-order tree in.b.entries and everything below it, appended to s.entries
template <typename real> void splice_emit(const std::vector<CrPrimitive>& prims, SceneBoxes<real>& in, int32_t i, Spliced<real>& s) {
    const Builder<real>& b = in.b;
    const Entry<real> e = b.entries[i];
    const int32_t idx = (int32_t)s.entries.size();
    s.entries.push_back(e);
    if (e.leaf < 0) {
        splice_emit(prims, in, i + 1, s);
        splice_emit(prims, in, b.entries[i + 1].skip, s);
        s.entries[idx].skip = (int32_t)s.entries.size();
        return;
    }
    const int32_t start = e.leaf >> 1, span = (e.leaf & 1) + 1;
    bool any_inner = false;
    for (int32_t k = 0; k < span; k++) any_inner |= in.objs[b.order[start + k]].inner >= 0;
    if (!any_inner) {
        const int32_t first = (int32_t)s.prims.size();
        for (int32_t k = 0; k < span; k++) append_object(prims, in, b.order[start + k], s.prims);
        s.entries[idx].leaf = splice_run(s, first, (int32_t)s.prims.size() - first, false);
        s.entries[idx].skip = idx + 1;
        return;
    }
    s.entries[idx].leaf = -1;
    for (int32_t k = 0; k < span; k++) {
        const Obj& o = in.objs[b.order[start + k]];
        if (o.inner < 0) {
            const int32_t first = (int32_t)s.prims.size();
            append_object(prims, in, b.order[start + k], s.prims);
            splice_pseudo_leaf(s, first, (int32_t)s.prims.size() - first);
            continue;
        }
        const Builder<real>& ib = in.inners[o.inner];
        const int32_t base = (int32_t)s.entries.size();
        for (const Entry<real>& ie : ib.entries) {
            Entry<real> c = ie;
            c.skip += base;
            if (c.leaf >= 0) {
                const int32_t s0 = c.leaf >> 1, cnt = (c.leaf & 1) + 1, first = (int32_t)s.prims.size();
                for (int32_t q = 0; q < cnt; q++) s.prims.push_back(in.inner_src[o.inner][ib.order[s0 + q]]);
                c.leaf = splice_run(s, first, cnt, false);
            }
            s.entries.push_back(c);
        }
    }
    if (span == 1) splice_pseudo_leaf(s, (int32_t)s.prims.size(), 0);
    s.entries[idx].skip = (int32_t)s.entries.size();
}

// CR_BVH_REFERENCE over n >= 1 objects: the reference's tree, the inner trees spliced in, level by level.
template <typename real>
void reference_tree(const std::vector<CrPrimitive>& prims, SceneBoxes<real>& in, std::vector<int32_t>& level_begin, Spliced<real>& s) {
    in.b.build_root((int32_t)in.objs.size());
    if (!in.inners.empty()) {
        splice_emit(prims, in, 0, s);
        in.b.entries.swap(s.entries);
        s.on = true;
    }
    relayout_bfs(in.b.entries, level_begin);
}

// Stage 2 where the host builds the tree (every mode but CR_BVH_LBVH and the device SAH builder): the mode's builder.
template <typename real>
void host_topology(const std::vector<CrPrimitive>& prims, int32_t mode, SceneBoxes<real>& in, std::vector<int8_t>& axis, std::vector<int32_t>& level_begin,
                   Spliced<real>& s) {
    const int32_t n = (int32_t)in.objs.size();
    if (n == 0) level_begin.assign(1, 0);
    else if (mode == CR_BVH_REFERENCE) reference_tree(prims, in, level_begin, s);
    else sah_host_tree(in.b.bmin, in.b.bmax, n, in.b.order, in.b.entries, axis, level_begin);
}

// ---------------------------------------------------------------- leaf layout
// What the device walks: a leaf wrapper names a run of primitive records.  One or two records fit the wrapper
// itself; a leaf that holds a list names its run through the side table (first, count).
template <typename real> struct LeafLayout {
    std::vector<Prim<real>> leaf_prims;     // primitive records in leaf order
    std::vector<int32_t> first_of;          // without a splice: leaf-order position of an object -> its first record; [n]: the count
    std::vector<Entry<real>> dev_entries;   // scenes with lists or a splice: in.b.entries with leaves that name record runs
    std::vector<int32_t> leaf_runs;         // (first, count) pairs
    bool own_entries = false;               // dev_entries is what the device walks (otherwise in.b.entries itself)
};

// False: more primitive records than a leaf link can name.
template <typename real>
bool layout_leaves(const std::vector<CrPrimitive>& prims, SceneBoxes<real>& in, Spliced<real>& s, LeafLayout<real>& lay) {
    const int32_t n = (int32_t)in.objs.size();
    const Builder<real>& b = in.b;
    lay.leaf_prims.reserve(n);
    lay.first_of.resize((size_t)n + 1);
    if (s.on) lay.leaf_prims.swap(s.prims);
    else {
        for (int32_t i = 0; i < n; i++) {
            lay.first_of[i] = (int32_t)lay.leaf_prims.size();
            append_object(prims, in, b.order[i], lay.leaf_prims);
        }
        lay.first_of[n] = (int32_t)lay.leaf_prims.size();
    }
    if (lay.leaf_prims.size() >= ((size_t)1 << 29)) return false;
    lay.own_entries = s.on || in.any_lists;
    if (lay.own_entries) lay.dev_entries = b.entries;
    for (Entry<real>& e : lay.dev_entries) {
        if (e.leaf < 0) continue;
        int32_t first, count;
        bool pseudo = false;
        if (s.on) { const Run r = s.runs[e.leaf]; first = r.first; count = r.count; pseudo = r.pseudo; }
        else {
            const int32_t start = e.leaf >> 1, span = (e.leaf & 1) + 1;
            first = lay.first_of[start]; count = lay.first_of[start + span] - first;
        }
        if (!pseudo && (count == 1 || count == 2)) e.leaf = (first << 1) | (count - 1);
        else { e.leaf = kLeafRun | (pseudo ? kLeafPseudo : 0) | (int32_t)(lay.leaf_runs.size() / 2); lay.leaf_runs.push_back(first); lay.leaf_runs.push_back(count); }
    }
    return true;
}

// leaf-order position -> index in the caller's primitive list
template <typename real> std::vector<int32_t> leaf_descs(const SceneBoxes<real>& in) {
    std::vector<int32_t> out(in.objs.size());
    for (size_t i = 0; i < out.size(); i++) out[i] = in.objs[in.b.order[i]].desc;
    return out;
}

// ---------------------------------------------------------------- export
// cr_export_bvh: the wrapper tree the device walks, re-expressed as the reference's BVHWrapper tree (each
// wrapper = box + left/right child) in walk order.  A leaf wrapper of one primitive holds it twice, as the
// reference's span-1 wrappers do (bvhwrapper.rs:58-60).  E is not empty; boxes, children (and split_axis, if given) hold E.size() wrappers.
template <typename real>
void export_walk(const std::vector<Entry<real>>& E, const std::vector<int8_t>& host_axis, const std::vector<int32_t>& leaf_desc, bool ordered,
                 double* boxes, int32_t* children, int32_t* split_axis) {
    struct Frame { int32_t entry, out, state; };
    std::vector<Frame> fr{{0, -1, 0}};
    int32_t n = 0;
    while (!fr.empty()) {
        Frame& f = fr.back();
        const Entry<real>& e = E[f.entry];
        if (f.state == 0) {
            f.out = n++;
            for (int k = 0; k < 6; k++) boxes[6 * f.out + k] = (double)e.b[k];
            if (split_axis) split_axis[f.out] = (ordered && e.leaf < 0) ? (int32_t)host_axis[f.entry] : -1;
            if (e.leaf >= 0) {
                const int32_t first = e.leaf >> 1, count = (e.leaf & 1) + 1;
                children[2 * f.out] = ~leaf_desc[first];
                children[2 * f.out + 1] = ~leaf_desc[first + count - 1];
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
}

}   // namespace cr
