// views_pack_check.cpp -- the camera table of cr_render_views_* on the CPU (tests/test_views_abi.py): compiles
// crucible_amd/csrc/pack.hpp's pack_views / pack_view_keys, what prepare_args packs the views' records and the shared key
// table with, with a plain C++ compiler and prints them for a fixed set of cameras.
//   views_pack_check f32|f64 N  from_0 at_0  from_1 at_1 ...   (the key counts of the N views)
// Key i of the call (counted over all views in order, look_from keys before look_at keys within a view) carries t1 = i,
// and view k's camera has vfov 20 + k, so the output shows where every key landed and which record is which.
// Output: "total T", then per view "view k first_from n_from first_at n_at animated same", same = 1 when the record
// equals what pack_camera + pack_camera_frame make of the camera alone in every field but the two offsets; then
// "keys" and the t1 of every key of the table in order.
#include "pack.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <typename real>
static int run(const std::vector<int>& nf, const std::vector<int>& na) {
    const int n = (int)nf.size();
    std::vector<std::vector<CrKeyframe>> fk((size_t)n), ak((size_t)n);
    std::vector<CrCameraDesc> cams((size_t)n);
    int next = 0;
    for (int k = 0; k < n; k++) {
        for (int pass = 0; pass < 2; pass++) {
            std::vector<CrKeyframe>& dst = pass ? ak[(size_t)k] : fk[(size_t)k];
            for (int i = 0; i < (pass ? na[(size_t)k] : nf[(size_t)k]); i++) {
                CrKeyframe key;
                memset(&key, 0, sizeof key);
                key.t0 = 0.0; key.t1 = (double)next++; key.a = 0.25 * (i + 1); key.channel = i % 3; key.interp = i & 1;
                dst.push_back(key);
            }
        }
        CrCameraDesc& c = cams[(size_t)k];
        memset(&c, 0, sizeof c);
        c.image_width = 13; c.image_height = 9; c.vfov_degrees = 20.0 + k; c.defocus_angle_degrees = k & 1 ? 0.6 : 0.0; c.focus_dist = 4.0 + k;
        c.look_from[0] = 1.0 + k; c.look_from[1] = 2.0; c.look_from[2] = 7.0; c.look_at[1] = 0.5; c.vup[1] = 1.0;
        c.from_key_count = nf[(size_t)k]; c.at_key_count = na[(size_t)k];
        c.from_keys = fk[(size_t)k].data(); c.at_keys = ak[(size_t)k].data();
    }
    std::vector<cr::CamConst<real>> table((size_t)n);
    memset((void*)table.data(), 0, table.size() * sizeof(cr::CamConst<real>));
    const long long total = (long long)cr::pack_views<real>(cams.data(), n, table.data());
    printf("total %lld\n", total);
    for (int k = 0; k < n; k++) {
        cr::CamConst<real> alone;
        memset((void*)&alone, 0, sizeof alone);
        cr::pack_camera(&cams[(size_t)k], alone);
        cr::pack_camera_frame(alone);
        cr::CamConst<real> t = table[(size_t)k];
        const int ff = t.from_key_first, af = t.at_key_first;
        t.from_key_first = alone.from_key_first; t.at_key_first = alone.at_key_first;
        printf("view %d %d %d %d %d %d %d\n", k, ff, t.from_key_count, af, t.at_key_count, t.animated, memcmp(&t, &alone, sizeof t) == 0 ? 1 : 0);
    }
    std::vector<cr::Key<real>> keys((size_t)(total > 0 ? total : 1));
    cr::pack_view_keys<real>(cams.data(), n, keys.data());
    printf("keys");
    for (long long i = 0; i < total; i++) printf(" %d", (int)keys[(size_t)i].t1);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: views_pack_check f32|f64 N from_0 at_0 ...\n"); return 2; }
    const int n = atoi(argv[2]);
    if (n < 1 || argc != 3 + 2 * n) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<int> nf, na;
    for (int k = 0; k < n; k++) { nf.push_back(atoi(argv[3 + 2 * k])); na.push_back(atoi(argv[4 + 2 * k])); }
    return strcmp(argv[1], "f64") == 0 ? run<double>(nf, na) : run<float>(nf, na);
}
