// CPU validation of the Karras construction in crucible_amd/csrc/lbvh.hpp (built and run by tests/test_lbvh_host.py):
// random keys with many duplicates and all-equal keys, several sizes -- every leaf reached exactly once, every
// internal node referenced exactly once, sibling ranges adjacent, the root covering everything.  Two more modes hand
// lbvh_children and lbvh_key of given inputs to tests/test_lbvh_model_host.py (children_mode, keys_mode below).
#include "lbvh.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
using namespace cr;
static bool check(const std::vector<uint64_t>& keys) {
    const int32_t n = (int32_t)keys.size();
    std::vector<int32_t> ch(2 * std::max(1, n - 1));
    for (int32_t i = 0; i < n - 1; i++) lbvh_children(keys.data(), n, i, ch[2 * i], ch[2 * i + 1]);
    // every internal node except 0 and every leaf must be referenced exactly once; ranges must nest
    std::vector<int> ref_int(n, 0), ref_leaf(n, 0);
    struct R { int32_t lo, hi; };
    std::vector<R> range(n);
    // compute ranges by DFS from the root (explicit stack), detect cycles by visit count
    std::vector<int32_t> st{0};
    std::vector<int> seen(n, 0);
    long visited = 0;
    // post-order range computation
    std::vector<std::pair<int32_t,int>> fr{{0,0}};
    while (!fr.empty()) {
        auto [v, s] = fr.back();
        if (s == 0) {
            if (seen[v]++) { printf("internal %d visited twice\n", v); return false; }
            visited++;
            fr.back().second = 1;
            for (int k = 0; k < 2; k++) { int32_t c = ch[2 * v + k]; if (c >= 0) { if (c >= n - 1) { printf("bad child\n"); return false; } ref_int[c]++; fr.push_back({c, 0}); } else { if (~c >= n) { printf("bad leaf\n"); return false; } ref_leaf[~c]++; } }
        } else {
            R r{INT32_MAX, -1};
            for (int k = 0; k < 2; k++) { int32_t c = ch[2 * v + k]; R cr = c >= 0 ? range[c] : R{~c, ~c}; r.lo = std::min(r.lo, cr.lo); r.hi = std::max(r.hi, cr.hi); }
            // left child's range must end right before the right child's begins
            int32_t cl = ch[2 * v], crr = ch[2 * v + 1];
            R a = cl >= 0 ? range[cl] : R{~cl, ~cl}, b = crr >= 0 ? range[crr] : R{~crr, ~crr};
            if (a.hi + 1 != b.lo) { printf("children of %d not adjacent: [%d,%d] [%d,%d]\n", v, a.lo, a.hi, b.lo, b.hi); return false; }
            range[v] = r;
            fr.pop_back();
        }
    }
    if (visited != n - 1) { printf("visited %ld of %d internals\n", visited, n - 1); return false; }
    for (int32_t i = 0; i < n; i++) if (ref_leaf[i] != 1) { printf("leaf %d referenced %d times\n", i, ref_leaf[i]); return false; }
    for (int32_t i = 1; i < n - 1; i++) if (ref_int[i] != 1) { printf("internal %d referenced %d times\n", i, ref_int[i]); return false; }
    if (range[0].lo != 0 || range[0].hi != n - 1) { printf("root range wrong\n"); return false; }
    return true;
}
// The whole of a binary file, as 8-byte words
static bool read_words(const char* path, std::vector<uint64_t>& w) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t buf[4096];
    size_t got;
    while ((got = fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    return true;
}
// `lbvh_check children FILE`: FILE holds key sets, each a count n (u64) followed by n sorted u64 keys; writes, per set,
// lbvh_children of its n - 1 internal nodes as int32 pairs (left, right) to stdout.  tests/test_lbvh_model_host.py
// compares them with the radix tree of tests/lbvh_model.py.
static int children_mode(const char* path) {
    std::vector<uint64_t> w;
    if (!read_words(path, w)) return 2;
    for (size_t at = 0; at < w.size();) {
        const uint64_t n = w[at++];
        if (n < 1 || n > (uint64_t)INT32_MAX || at + n > w.size()) return 3;
        std::vector<int32_t> ch(2 * (size_t)(n - 1));
        for (int32_t i = 0; i < (int32_t)n - 1; i++) lbvh_children(w.data() + at, (int32_t)n, i, ch[2 * i], ch[2 * i + 1]);
        if (!ch.empty() && fwrite(ch.data(), 4, ch.size(), stdout) != ch.size()) return 4;
        at += n;
    }
    return 0;
}
// `lbvh_check keys FILE`: FILE holds rows of nine doubles (centroid, lo, inv_ext); writes lbvh_key of each row as u64.
static int keys_mode(const char* path) {
    std::vector<uint64_t> w;
    if (!read_words(path, w) || w.size() % 9) return 2;
    std::vector<uint64_t> out(w.size() / 9);
    for (size_t r = 0; r < out.size(); r++) {
        double d[9];
        memcpy(d, w.data() + 9 * r, sizeof d);
        out[r] = lbvh_key(d, d + 3, d + 6);
    }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), stdout) != out.size()) return 4;
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "children")) return children_mode(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "keys")) return keys_mode(argv[2]);
    if (argc != 1) { fprintf(stderr, "usage: lbvh_check [children FILE | keys FILE]\n"); return 2; }
    std::mt19937_64 rng(7);
    long ok = 0;
    for (int trial = 0; trial < 4000; trial++) {
        int n = 2 + (int)(rng() % (trial < 3000 ? 40 : 5000));
        int mode = trial % 4;
        std::vector<uint64_t> k(n);
        for (auto& x : k) x = mode == 0 ? rng() >> 1 : mode == 1 ? (rng() % 7) : mode == 2 ? 42 : ((rng() % 3) << 60 | (rng() % 4));
        std::sort(k.begin(), k.end());
        if (!check(k)) { printf("FAILED trial %d n %d mode %d\n", trial, n, mode); return 1; }
        ok++;
    }
    // spread / key sanity
    double lo[3] = {0, 0, 0}, inv[3] = {1, 1, 1};
    double c0[3] = {0, 0, 0}, c1[3] = {1, 1, 1}, cx[3] = {1, 0, 0};
    printf("ok %ld trees; key(0)=%llx key(1)=%llx key(x)=%llx\n", ok, (unsigned long long)lbvh_key(c0, lo, inv), (unsigned long long)lbvh_key(c1, lo, inv), (unsigned long long)lbvh_key(cx, lo, inv));
    return 0;
}
