// residency_check.cpp -- crucible_amd/csrc/residency.hpp on the CPU (tests/test_residency_host.py): the residency rule and
// the scene's layout over a case file, one case per line (launch()'s chunk and tile rules: tests/launch_plan_check.cpp):
//   R n_entries entry_rec screen_rec ordered can_screen screen screen_lds plain_lds lds_bytes lds_all_screen side_bytes
//     lds_top_bytes lds_side_limit f32 whole_frame adaptive latency_entries latency_top_bytes latency_slot_bytes
//       -> "res screen latency lds_entries lds_side lds_bytes clear_screen"
//   L n_records record_rec n_prims prim_rec n_mats mat_rec n_texs tex_rec with_prims with_side
//       -> "prims mats texs bytes end": scene_layout over the tables' bytes, formed as handle.hpp forms them (count * record)
#include "residency.hpp"

#include <cstdio>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'R') {
            long long v[19];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            cr::ResidencyQuery q = {};
            q.n_entries = (int32_t)v[0]; q.entry_rec = (size_t)v[1]; q.screen_rec = (size_t)v[2];
            q.ordered = v[3] != 0; q.can_screen = v[4] != 0; q.screen = v[5] != 0; q.screen_lds = v[6] != 0; q.plain_lds = v[7] != 0;
            q.lds_bytes = (size_t)v[8]; q.lds_all_screen = (size_t)v[9]; q.side_bytes = (size_t)v[10];
            q.lds_top_bytes = (size_t)v[11]; q.lds_side_limit = (size_t)v[12];
            q.f32 = v[13] != 0; q.whole_frame = v[14] != 0; q.adaptive = v[15] != 0;
            q.latency_entries = (int32_t)v[16]; q.latency_top_bytes = (size_t)v[17]; q.latency_slot_bytes = (size_t)v[18];
            const cr::Residency r = cr::choose_residency(q);
            printf("%d %d %d %d %d %zu %d\n", r.res, r.screen ? 1 : 0, r.latency ? 1 : 0, r.lds_entries, r.lds_side, r.lds_bytes, r.clear_screen ? 1 : 0);
        } else if (kind == 'L') {
            long long v[10];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            const cr::SceneLayout l = cr::scene_layout((size_t)v[0] * (size_t)v[1], (size_t)v[2] * (size_t)v[3], (size_t)v[4] * (size_t)v[5],
                                                       (size_t)v[6] * (size_t)v[7], v[8] != 0, v[9] != 0);
            printf("%zu %zu %zu %zu %zu\n", l.prims, l.mats, l.texs, l.bytes, l.end());
        } else return 2;
    }
    fclose(f);
    return 0;
}
