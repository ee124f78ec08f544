// launch_plan_check.cpp -- crucible_amd/csrc/launch_plan.hpp on the CPU (tests/test_launch_plan_host.py): how launch() and
// aov_launch() cut their work into kernel launches, over a case file, one case per line, one line of numbers per case:
//   C sg_total grid block chunk_override   -> the chunk
//   T n                                    -> "lw lh" of the default tile
//   X n                                    -> log2 of fx_scale_for(n)
//   P tile_lw tile_lh n_samples block_log2 relax res scene_lds_bytes max_block block
//       -> "lw lh fx_off lds_base lds_per_wave use_lds bytes(max_block) bytes(block)"
//   K relax keyed latency list n_frames whole adaptive   -> 0 ok, 1 one frame per launch, 2 whole frames, 3 no tile list
//   S <query> alloc_fails                  -> "refusal tiled batch lw lh tiles_x tiles_y ns fpl fx_acc_bytes sample_buf_bytes sg_acc_bytes"
//     <query>: relax sample_granular s_begin s_end reg_w reg_h real_bytes sample_buf_limit work_counter_max lw lh tile_fixed
//              n_frames adaptive split_passes fixed_sums px_tiles_x px_tiles_y;  alloc_fails: lane_owns_pixel is applied, as
//              launch() applies it when a buffer cannot be had
//   B <query> n_cus per_cu block chunk_override
//       -> "grid n_threads n_launches", then per launch "f0 fn b0 b1 groups sg_total blocks chunk": the loops of launch()
//   F ns n_samples n_tiles fit grid block chunk_override   -> "groups sg_total blocks chunk" of one batch
//   G n_cus per_cu work block lanes_per_item               -> "blocks n_threads"
//   U tiles_x tiles_y groups batch batch_frames n_cus per_cu block work_counter_max
//       -> "unit_groups unit_chunks frame_tiles frame_units frames_per_launch n_launches units_of_the_last_launch"
#include "launch_plan.hpp"

#include <cinttypes>
#include <cstdio>

static bool read_query(FILE* f, cr::SampleQuery& q) {
    long long v[18];
    for (long long& x : v)
        if (fscanf(f, "%lld", &x) != 1) return false;
    q.relax = v[0] != 0; q.sample_granular = v[1] != 0; q.s_begin = (int32_t)v[2]; q.s_end = (int32_t)v[3];
    q.reg_w = (uint32_t)v[4]; q.reg_h = (uint32_t)v[5]; q.real_bytes = (size_t)v[6]; q.sample_buf_limit = (size_t)v[7];
    q.work_counter_max = (uint64_t)v[8]; q.lw = (int)v[9]; q.lh = (int)v[10]; q.tile_fixed = v[11] != 0; q.n_frames = (int32_t)v[12];
    q.adaptive = v[13] != 0; q.split_passes = v[14] != 0; q.fixed_sums = v[15] != 0; q.px_tiles_x = (uint32_t)v[16]; q.px_tiles_y = (uint32_t)v[17];
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'C') {
            uint64_t total, grid, block;
            int chunk_override;
            if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &total, &grid, &block, &chunk_override) != 4) return 2;
            printf("%u\n", cr::work_chunk(total, grid, block, chunk_override));
        } else if (kind == 'T') {
            long long n;
            if (fscanf(f, "%lld", &n) != 1) return 2;
            int lw = -1, lh = -1;
            cr::default_tile(n, lw, lh);
            printf("%d %d\n", lw, lh);
        } else if (kind == 'X') {
            long long n;
            if (fscanf(f, "%lld", &n) != 1) return 2;
            printf("%d\n", std::ilogb(cr::fx_scale_for(n)));
        } else if (kind == 'P') {
            long long v[9];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            const cr::TilePlan t = cr::plan_tile((int)v[0], (int)v[1], v[2], (int)v[3], v[4] != 0, (int)v[5], (size_t)v[6], (int)v[7]);
            printf("%d %d %zu %zu %zu %d %zu %zu\n", t.lw, t.lh, t.fx_off, t.lds_base, t.lds_per_wave, t.use_lds ? 1 : 0, t.lds_bytes((int)v[7]), t.lds_bytes((int)v[8]));
        } else if (kind == 'K') {
            long long v[7];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            printf("%d\n", (int)cr::check_call_shape(v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, (int32_t)v[4], v[5] != 0, v[6] != 0));
        } else if (kind == 'S') {
            cr::SampleQuery q = {};
            int alloc_fails;
            if (!read_query(f, q) || fscanf(f, "%d", &alloc_fails) != 1) return 2;
            cr::SamplePlan p = cr::plan_samples(q);
            if (alloc_fails) cr::lane_owns_pixel(p);
            printf("%d %d %d %d %d %u %u %u %d %zu %zu %zu\n", (int)p.refusal, p.tiled ? 1 : 0, p.batch, p.lw, p.lh, p.tiles_x, p.tiles_y, p.ns, p.fpl, p.fx_acc_bytes,
                   p.sample_buf_bytes, p.sg_acc_bytes);
        } else if (kind == 'B') {
            cr::SampleQuery q = {};
            int n_cus, per_cu, block, chunk_override;
            if (!read_query(f, q) || fscanf(f, "%d %d %d %d", &n_cus, &per_cu, &block, &chunk_override) != 4) return 2;
            const cr::SamplePlan p = cr::plan_samples(q);
            if (p.refusal != cr::kPlanOk || p.batch <= 0) return 3;   // (a case of S)
            const cr::GridPlan gp = cr::plan_grid(n_cus, per_cu, p.grid_work(q.s_end - q.s_begin), block, 1);
            int n_launches = 0;
            for (int pass = 0; pass < 2; pass++) {   // count, then print
                if (pass) printf("%u %u %d", gp.blocks, gp.n_threads, n_launches);
                for (int32_t f0 = 0; f0 < q.n_frames; f0 += p.fpl) {
                    const int32_t fn = p.fpl < q.n_frames - f0 ? p.fpl : q.n_frames - f0;
                    for (int64_t b0 = q.s_begin; b0 < q.s_end; b0 += p.batch) {
                        const int32_t b1 = cr::batch_end(b0, p.batch, q.s_end);
                        const cr::BatchLaunch bl = cr::plan_batch(p.ns, b1 - (int32_t)b0, p.tiles(), fn, false, gp.blocks, block, chunk_override);
                        if (pass) printf(" %d %d %d %d %u %u %u %u", f0, fn, (int32_t)b0, b1, bl.groups, bl.sg_total, bl.blocks, bl.chunk);
                        else n_launches++;
                    }
                }
            }
            printf("\n");
        } else if (kind == 'F') {
            long long v[7];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            const cr::BatchLaunch bl = cr::plan_batch((uint32_t)v[0], (int32_t)v[1], (uint64_t)v[2], 1, v[3] != 0, (uint32_t)v[4], (int)v[5], (int)v[6]);
            printf("%u %u %u %u\n", bl.groups, bl.sg_total, bl.blocks, bl.chunk);
        } else if (kind == 'G') {
            long long v[5];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            const cr::GridPlan gp = cr::plan_grid((int)v[0], (int)v[1], (uint64_t)v[2], (int)v[3], (int)v[4]);
            printf("%u %u\n", gp.blocks, gp.n_threads);
        } else if (kind == 'U') {
            long long v[9];
            for (long long& x : v)
                if (fscanf(f, "%lld", &x) != 1) return 2;
            const cr::GuidePlan g = cr::plan_guide_units((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], v[3] != 0, (uint32_t)v[4], (int)v[5], (int)v[6], (int)v[7], (uint64_t)v[8]);
            uint64_t n_launches = 0, last = 0;
            for (uint64_t f0 = 0; f0 < g.n_frames; f0 += g.frames_per_launch) { n_launches++; last = g.units(g.slice_frames(f0)); }   // aov_launch's loop
            printf("%u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g.unit_groups, g.unit_chunks, g.frame_tiles, g.frame_units, g.frames_per_launch, n_launches, last);
        } else return 2;
    }
    fclose(f);
    return 0;
}
