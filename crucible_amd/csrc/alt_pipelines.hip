// alt_pipelines.hip -- the two alternative render pipelines, CRUCIBLE_PIPELINE=wavefront (wavefront.hpp) and =queue
// (queue.hpp): reference-order cross-checks of the megakernel on unordered trees, not product paths.  The only unit that
// includes their headers and emits their kernels.
#include "handle.hpp"
#include "wavefront.hpp"
#include "queue.hpp"

namespace cr {

// a queue kernel gives up where a wave waits too long on an LDS queue: its abort word, read once the launch has run
int32_t check_queue_abort(CrHandle* h) {
    if (!h->check_abort) return CR_OK;
    uint64_t aborted = 0;
    HIP_TRY(h, hipMemcpy(&aborted, (uint64_t*)h->counters.p + 4, sizeof aborted, hipMemcpyDeviceToHost));
    h->check_abort = false;
    if (aborted) return fail(h, CR_ERR_HIP, "queue pipeline: a wave timed out waiting on an LDS queue (image incomplete)");
    return CR_OK;
}

// ---------------------------------------------------------------- LDS-queue megakernel (queue.hpp)
template <typename real, int RES, bool ANIM>
int32_t launch_queue(CrHandle* h, const KernelArgs<real>& args_in, size_t scene_lds_bytes, CrStats* stats) {
    KernelArgs<real> args = args_in;
    auto kern = queue_kernel<real, RES, ANIM>;
    const size_t lds_bytes = r16(scene_lds_bytes) + queue_state_bytes<real>();
    HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int per_cu = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)QK_SLOTS, lds_bytes));
    if (per_cu < 1) return fail(h, CR_ERR_HIP, "queue kernel does not fit on a CU");
    const uint32_t total_work = args.tiles_x * args.tiles_y * 64u;
    uint32_t grid = (uint32_t)(h->n_cus * per_cu);
    const uint32_t need_blocks = (total_work + QK_SLOTS - 1) / QK_SLOTS;
    if (grid > need_blocks) grid = need_blocks;
    if (grid < 1) grid = 1;
    args.n_threads = grid * QK_SLOTS;
    args.queue_walk_waves = (uint32_t)h->queue_walk_waves;
    args.queue_min_batch = (uint32_t)h->queue_min_batch; args.queue_patience = (uint32_t)h->queue_patience;
    HIP_TRY(h, h->att_stack.ensure((size_t)3 * (size_t)std::max(1, args.max_depth) * args.n_threads * sizeof(real)));
    args.att_stack = (real*)h->att_stack.p;
    HIP_TRY(h, hipMemsetAsync(h->work_counter.p, 0, 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, 64 * sizeof(uint64_t), h->stream));
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(QK_SLOTS), lds_bytes, h->stream, args);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->last_block = (int)QK_SLOTS; h->last_grid = (int)grid; h->check_abort = true;
    if (stats) {   // the abort word first: an incomplete image reports no stats
        HIP_TRY(h, hipEventSynchronize(h->ev1));
        int32_t rc = check_queue_abort(h);
        if (rc != CR_OK) return rc;
        return finish_stats(h, stats, (uint64_t)args.cam.W * (uint64_t)args.cam.H * (uint64_t)(args.sample_end - args.sample_begin), args.n_entries, RES);
    }
    return CR_OK;
}

// ---------------------------------------------------------------- wavefront pipeline driver
template <typename real, int RES, bool ANIM>
int32_t wf_extend_config(CrHandle* h, size_t lds_bytes, int& block, int& grid) {
    constexpr bool LDS = RES != RES_GLOBAL;
    auto kern = wf_extend_kernel<real, RES, ANIM>;
    if (LDS) HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int per_cu = 1;   // an override above the kernel's largest workgroup leaves no candidate (the megakernel ignores such an override)
    int32_t rc = pick_block(h, (const void*)kern, MaxBlock<real>::value, false, LDS ? lds_bytes : 0, 0, "extend kernel does not fit on a CU", block, per_cu);
    if (rc != CR_OK) return rc;
    grid = h->n_cus * per_cu;
    return CR_OK;
}

template <typename real, int RES, bool ANIM>
int32_t wf_run(CrHandle* h, WfArgs<real>& W, size_t lds_bytes, int32_t s_begin, int32_t s_count, int32_t batch_cap, CrStats* stats) {
    constexpr bool LDS = RES != RES_GLOBAL;
    int block = 256, grid = 1;
    int32_t rc = wf_extend_config<real, RES, ANIM>(h, lds_bytes, block, grid);
    if (rc != CR_OK) return rc;
    const size_t npix = (size_t)W.k.cam.W * W.k.cam.H;
    const uint32_t logic_grid = (W.n_slots + 255) / 256;
    const uint32_t fin_grid = (uint32_t)((npix + 255) / 256);
    HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, 64 * sizeof(uint64_t), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->wf_acc.p, 0, npix * 3 * sizeof(real), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->wf_job.p, 0xFF, (size_t)W.n_slots * 4, h->stream));
    // no slot may look like it holds a ray before the logic kernel gives it one: recycled device memory can hold
    // WF_PENDING from an earlier handle, and extend would walk that slot's stale ray (extra node tests, same image)
    HIP_TRY(h, hipMemsetAsync(h->wf_hit_prim.p, 0, (size_t)W.n_slots * 4, h->stream));
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    int iterations = 0;
    const int LAG = 4, RING = 8;
    const int64_t s_end = (int64_t)s_begin + s_count;
    for (int64_t b0 = s_begin; b0 < s_end; b0 += batch_cap) {   // (64 bits: b0 + batch_cap may pass INT32_MAX)
        W.batch_begin = (int32_t)b0;
        W.batch_samples = (int32_t)std::min<int64_t>(batch_cap, s_end - b0);
        W.n_jobs = (uint32_t)W.batch_samples * W.total_work;
        W.last_batch = (b0 + W.batch_samples >= s_end) ? 1 : 0;
        HIP_TRY(h, hipMemsetAsync(h->wf_ctrl.p, 0, 1024, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->wf_chunk.p, 0, ((size_t)W.n_slots / 64 + 1) * 8, h->stream));
        for (int it = 0;; it++) {
            W.ctrl_set = (uint32_t)(it & 1);
            W.ring_slot = h->wf_ring_dev + (it % RING);
            hipLaunchKernelGGL((wf_logic_kernel<real, ANIM>), dim3(logic_grid), dim3(256), 0, h->stream, W);
            hipLaunchKernelGGL((wf_extend_kernel<real, RES, ANIM>), dim3(grid), dim3(block), LDS ? lds_bytes : 0, h->stream, W);
            HIP_TRY(h, hipEventRecord(h->wf_ev[it % RING], h->stream));
            iterations++;
            if (it >= LAG) {   // lagged check: the GPU is already LAG iterations ahead, so it never waits for the host
                int k = it - LAG;
                HIP_TRY(h, hipEventSynchronize(h->wf_ev[k % RING]));
                if (((const uint32_t*)h->wf_ring_host.p)[k % RING] == 0) break;   // logic found nothing to trace and no job left: batch done
            }
        }
        hipLaunchKernelGGL((wf_finalize_kernel<real>), dim3(fin_grid), dim3(256), 0, h->stream, W);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->last_block = block; h->last_grid = grid; h->wf_last_iterations = iterations;
    if (stats) {
        rc = finish_stats(h, stats, (uint64_t)npix * (uint64_t)s_count, W.k.n_entries, RES);
        if (rc != CR_OK) return rc;
#ifdef CR_DIAG
        {
            uint64_t d[16];
            HIP_TRY(h, hipMemcpy(d, h->counters.p, sizeof d, hipMemcpyDeviceToHost));
            fprintf(stderr, "[diag-wf] block=%d grid=%d iterations=%d rounds=%llu walk_wave_steps=%llu leaf_lane=%llu leaf_wave=%llu clk_refill=%llu clk_walk=%llu clk_leaf=%llu clk_total=%llu lane_steps=%llu\n",
                    block, grid, iterations, (unsigned long long)d[4], (unsigned long long)d[5], (unsigned long long)d[6], (unsigned long long)d[7],
                    (unsigned long long)d[8], (unsigned long long)d[9], (unsigned long long)d[10], (unsigned long long)d[11], (unsigned long long)d[1]);
        }
#endif
    }
    return CR_OK;
}

template <typename real>
int32_t render_wavefront(CrHandle* h, const KernelArgs<real>& a, DevScene<real>& ds, bool anim, CrStats* stats) {
    WfArgs<real> W;
    memset(&W, 0, sizeof W);
    W.k = a;
    const size_t npix = (size_t)a.cam.W * a.cam.H;
    const int32_t s_begin = a.sample_begin, s_count = a.sample_end - a.sample_begin;
    W.total_work = a.tiles_x * a.tiles_y * 64u;
    // samples per batch: bounded by the per-sample colour buffer and by 32-bit job ids
    int64_t cap = (int64_t)(h->wf_sample_bytes / (npix * 3 * sizeof(real)));
    cap = std::min<int64_t>(cap, (int64_t)0xF0000000u / W.total_work);
    cap = std::max<int64_t>(1, std::min<int64_t>(cap, std::max(1, s_count)));
    const uint64_t jobs_first = (uint64_t)cap * W.total_work;
    W.n_slots = (uint32_t)std::min<uint64_t>(h->wf_slots, (jobs_first + 63) / 64 * 64);
    const size_t N = W.n_slots;
    HIP_TRY(h, h->wf_job.ensure(N * 4));
    HIP_TRY(h, h->wf_rng.ensure(N * 8));
    HIP_TRY(h, h->wf_ray.ensure(N * 7 * sizeof(real)));
    HIP_TRY(h, h->wf_depth.ensure(N * 8));
    HIP_TRY(h, h->wf_hit_t.ensure(N * sizeof(real)));
    HIP_TRY(h, h->wf_hit_prim.ensure(N * 4));
    HIP_TRY(h, h->wf_chunk.ensure((N / 64 + 1) * 8));
    HIP_TRY(h, h->wf_ctrl.ensure(1024));
    HIP_TRY(h, h->wf_samples.ensure((size_t)cap * npix * 3 * sizeof(real)));
    HIP_TRY(h, h->wf_acc.ensure(npix * 3 * sizeof(real)));
    HIP_TRY(h, h->att_stack.ensure((size_t)3 * (size_t)std::max(1, a.max_depth) * N * sizeof(real)));
    // the ring, its device address and its events: each made once, so a call that failed halfway is completed by the next
    HIP_TRY(h, h->wf_ring_host.ensure(64, hipHostMallocMapped));
    if (!h->wf_ring_dev) HIP_TRY(h, hipHostGetDevicePointer((void**)&h->wf_ring_dev, h->wf_ring_host.p, 0));
    for (int i = 0; i < 8; i++) HIP_TRY(h, h->wf_ev[i].create(hipEventDisableTiming));
    W.k.att_stack = (real*)h->att_stack.p;
    W.k.n_threads = W.n_slots;
    W.job = (uint32_t*)h->wf_job.p; W.rng = (uint64_t*)h->wf_rng.p; W.ray = (real*)h->wf_ray.p; W.depth = (int32_t*)h->wf_depth.p;
    W.hit_t = (real*)h->wf_hit_t.p; W.hit_prim = (int32_t*)h->wf_hit_prim.p; W.job_chunk = (uint32_t*)h->wf_chunk.p;
    W.ctrl = (uint32_t*)h->wf_ctrl.p; W.sample_rgb = (real*)h->wf_samples.p; W.acc = (real*)h->wf_acc.p;
    // the extend kernel stages entries | primitives when both fit, else the top levels of the tree
    const size_t full = whole_scene_layout(ds, sizeof(Entry<real>), false).end();
    const int32_t bc = (int32_t)cap;
    if (ds.n_entries > 0 && full <= h->lds_limit) {
        W.k.lds_entries = ds.n_entries;
        return anim ? wf_run<real, RES_LDS, true>(h, W, full, s_begin, s_count, bc, stats) : wf_run<real, RES_LDS, false>(h, W, full, s_begin, s_count, bc, stats);
    }
    const int32_t top = (int32_t)std::min<size_t>((size_t)ds.n_entries, h->lds_top_bytes / sizeof(Entry<real>));
    if (top > 0) {
        W.k.lds_entries = top;
        const size_t bytes = (size_t)top * sizeof(Entry<real>);
        return anim ? wf_run<real, RES_TOP, true>(h, W, bytes, s_begin, s_count, bc, stats) : wf_run<real, RES_TOP, false>(h, W, bytes, s_begin, s_count, bc, stats);
    }
    W.k.lds_entries = 0;
    return anim ? wf_run<real, RES_GLOBAL, true>(h, W, 0, s_begin, s_count, bc, stats) : wf_run<real, RES_GLOBAL, false>(h, W, 0, s_begin, s_count, bc, stats);
}

// The LDS-queue megakernel when scene + slot arrays fit in LDS (whole, or a window of the tree); *launched = false where
// they do not: the caller renders with the plain megakernel.
template <typename real>
int32_t render_queue(CrHandle* h, KernelArgs<real>& a, const DevScene<real>& ds, bool anim, CrStats* stats, bool* launched) {
    const size_t budget = 160 * 1024, state = queue_state_bytes<real>();
    // a slot packs its pixel as i | j << 16 and its counters as depth_left | stack_n << 16 (stack_n <= max_depth)
    if (a.cam.W > kQueueMaxExtent || a.cam.H > kQueueMaxExtent || a.max_depth > kQueueMaxDepth) { *launched = false; return CR_OK; }
    *launched = true;
    if (ds.n_entries > 0 && ds.lds_bytes + 16 + state <= budget) {
        a.lds_entries = ds.n_entries;
        return anim ? launch_queue<real, RES_LDS, true>(h, a, ds.lds_bytes, stats) : launch_queue<real, RES_LDS, false>(h, a, ds.lds_bytes, stats);
    }
    if (ds.n_entries > 0 && state + 16 * 1024 <= budget) {
        const size_t top_bytes = std::min(h->lds_top_bytes, (budget - state - 64) & ~(size_t)1023);
        a.lds_entries = (int32_t)std::min<size_t>((size_t)ds.n_entries, top_bytes / sizeof(Entry<real>));
        const size_t bytes = (size_t)a.lds_entries * sizeof(Entry<real>);
        return anim ? launch_queue<real, RES_TOP, true>(h, a, bytes, stats) : launch_queue<real, RES_TOP, false>(h, a, bytes, stats);
    }
    *launched = false;
    return CR_OK;
}

template int32_t render_wavefront<float>(CrHandle*, const KernelArgs<float>&, DevScene<float>&, bool, CrStats*);
template int32_t render_wavefront<double>(CrHandle*, const KernelArgs<double>&, DevScene<double>&, bool, CrStats*);
template int32_t render_queue<float>(CrHandle*, KernelArgs<float>&, const DevScene<float>&, bool, CrStats*, bool*);
template int32_t render_queue<double>(CrHandle*, KernelArgs<double>&, const DevScene<double>&, bool, CrStats*, bool*);

}   // namespace cr
