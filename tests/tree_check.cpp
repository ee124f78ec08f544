// The host tree code of crucible_amd/csrc/tree.hpp on the CPU: compiled with a plain C++ compiler (no device, no HIP
// runtime), run through the same stage functions build_dev_scene calls, in its order, and printed for
// tests/test_tree_host.py, which holds the output to tests/sah_model.py, tests/lbvh_model.py and the oracle.
//   tree_check tree FILE     CR_BVH_REFERENCE, CR_BVH_SAH, CR_BVH_SAH_ORDERED: "spliced S", "wrappers N", then what
//                            cr_export_bvh returns, a wrapper per line: the box as hexadecimal floats, two children, the split
//                            axis.  With a BVHWrapper element (S = 1, no export): the records the device walks (leaf, skip),
//                            the leaf runs (first, count), and per primitive record the material index of its descriptor.
//   tree_check links FILE    CR_BVH_SAH_ORDERED: per EntryO record "left axis" of the Entry record (-1 -1 for a leaf), the
//                            eight near children by ordered_near (-1 for a leaf) and the eight skip links.
//   tree_check lbvh FILE     CR_BVH_LBVH with the device's steps done on the host (lbvh_key, a stable sort, lbvh_children):
//                            "wrappers N", the children of the export per line, then "order" and the sorted descriptor indices.
//   tree_check number FILE   lbvh_number on a given node graph.  FILE: int32 n, m, then m int32 children.  "ok 0" or "ok 1 N".
// FILE of the first three: int32 is_f64, bvh_mode, n_prims, then n_prims CrPrimitive records.
#include "tree.hpp"

#include <cstdio>
#include <numeric>

using namespace cr;

template <typename real> struct Built {
    SceneBoxes<real> in;
    std::vector<int8_t> axis;
    std::vector<int32_t> level_begin;
    Spliced<real> spliced;
    LeafLayout<real> lay;
};

// CR_BVH_LBVH's device part on the host: what lbvh_key_kernel, the radix sort of (key, index) and lbvh_topology_kernel compute
template <typename real> bool lbvh_host(Built<real>& t) {
    Builder<real>& b = t.in.b;
    const int32_t n = (int32_t)t.in.src.size();
    b.entries.clear();
    t.level_begin.assign(1, 0);
    if (n == 0) return true;
    const LbvhBounds bnd = lbvh_bounds(b.bmin, b.bmax, n);
    std::vector<uint64_t> keys(n), sorted(n);
    for (int32_t i = 0; i < n; i++) {
        double c[3];
        lbvh_centroid(t.in.src[i], c);
        keys[i] = lbvh_key(c, bnd.lo, bnd.inv_ext);
    }
    std::iota(b.order.begin(), b.order.end(), 0);
    std::stable_sort(b.order.begin(), b.order.end(), [&](int32_t x, int32_t y) { return keys[x] < keys[y]; });
    for (int32_t i = 0; i < n; i++) sorted[i] = keys[b.order[i]];
    std::vector<int32_t> children((size_t)2 * std::max(1, n - 1));
    for (int32_t i = 0; i + 1 < n; i++) lbvh_children(sorted.data(), n, i, children[2 * i], children[2 * i + 1]);
    return lbvh_number(children, n, b.entries, t.level_begin);
}

// The host stages of build_dev_scene, in its order
template <typename real> bool build(const std::vector<CrPrimitive>& prims, int32_t mode, Built<real>& t) {
    scene_boxes(prims, mode == CR_BVH_REFERENCE, t.in);
    if (mode == CR_BVH_LBVH) { if (!lbvh_host(t)) return false; }
    else host_topology(prims, mode, t.in, t.axis, t.level_begin, t.spliced);
    return layout_leaves(prims, t.in, t.spliced, t.lay);
}

template <typename real> int run(const char* what, const std::vector<CrPrimitive>& prims, int32_t mode) {
    Built<real> t;
    if (!build(prims, mode, t)) { fprintf(stderr, "the build failed\n"); return 1; }
    const std::vector<Entry<real>>& E = t.in.b.entries;
    const int32_t ne = (int32_t)E.size();
    if (!strcmp(what, "links")) {
        const std::vector<EntryO<real>> eo = ordered_entries(E, t.axis);
        for (int32_t i = 0; i < ne; i++) {
            printf("%d %d", E[i].leaf < 0 ? -E[i].leaf : -1, E[i].leaf < 0 ? (int)t.axis[i] : -1);
            for (int o = 0; o < 8; o++) printf(" %d", eo[i].leaf < 0 ? ordered_near(eo[i].leaf, o) : -1);
            for (int o = 0; o < 8; o++) printf(" %d", eo[i].skip[o]);
            printf("\n");
        }
        return 0;
    }
    printf("spliced %d\nwrappers %d\n", t.spliced.on ? 1 : 0, ne);
    if (t.spliced.on) {   // export_tree refuses; what the device walks instead
        for (const Entry<real>& e : t.lay.dev_entries) printf("%d %d\n", e.leaf, e.skip);
        printf("runs %d\n", (int)(t.lay.leaf_runs.size() / 2));
        for (size_t i = 0; i + 1 < t.lay.leaf_runs.size(); i += 2) printf("%d %d\n", t.lay.leaf_runs[i], t.lay.leaf_runs[i + 1]);
        printf("prims %d\n", (int)t.lay.leaf_prims.size());
        for (const Prim<real>& p : t.lay.leaf_prims) printf("%d\n", p.kind_mat >> 1);
        return 0;
    }
    const std::vector<int32_t> leaf_desc = leaf_descs(t.in);
    std::vector<double> boxes((size_t)ne * 6);
    std::vector<int32_t> children((size_t)ne * 2), split_axis((size_t)ne);
    if (ne) export_walk(E, t.axis, leaf_desc, mode == CR_BVH_SAH_ORDERED, boxes.data(), children.data(), split_axis.data());
    const bool lbvh = !strcmp(what, "lbvh");
    for (int32_t i = 0; i < ne; i++) {
        if (!lbvh) for (int k = 0; k < 6; k++) printf("%a ", boxes[(size_t)i * 6 + k]);   // (an LBVH's boxes are filled in on the device)
        printf("%d %d %d\n", children[2 * i], children[2 * i + 1], split_axis[i]);
    }
    if (lbvh) {
        printf("order %d\n", (int)leaf_desc.size());
        for (int32_t d : leaf_desc) printf("%d\n", d);
    }
    return 0;
}

static int number(FILE* f) {
    int32_t head[2];
    if (fread(head, sizeof head, 1, f) != 1 || head[0] < 1 || head[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> children((size_t)head[1]);
    if (!children.empty() && fread(children.data(), 4, children.size(), f) != children.size()) { fprintf(stderr, "short file\n"); return 2; }
    std::vector<Entry<float>> entries;
    std::vector<int32_t> level_begin;
    if (!lbvh_number(children, head[0], entries, level_begin)) { printf("ok 0\n"); return 0; }
    printf("ok 1 %d\n", (int)entries.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: tree_check tree|links|lbvh|number FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    if (!strcmp(argv[1], "number")) { const int rc = number(f); fclose(f); return rc; }
    int32_t head[3];
    if (fread(head, sizeof head, 1, f) != 1 || head[2] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<CrPrimitive> prims((size_t)head[2]);
    if (!prims.empty() && fread(prims.data(), sizeof(CrPrimitive), prims.size(), f) != prims.size()) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    return head[0] ? run<double>(argv[1], prims, head[1]) : run<float>(argv[1], prims, head[1]);
}
