// Device check for tests/test_gpu_walk_offset.py: the f64 SCREEN walk as the headline's kernels run it
// (crucible_amd/csrc/walk.hpp WalkOffset) -- a segment begun with walk_begin_screened<true>(ws, ro, rd, start), then the
// megakernel's loop around walk_round<double, RES_LDS, false, false, true, true, /*LAZY_INV*/ true, SPHERE_LOOP> on a state whose
// position is the LDS address of the next screening record, compared with the sentinel `end` -- one wave per 64 lanes, with the
// tree staged as pathtrace_body stages it (screening records with their links turned into LDS addresses, then the primitive
// records), up to the whole LDS of a CU (kLdsLimit, the handle's lds_limit: the launch asks for the bytes it stages).
// Inputs, lane loop and per-ray output are those of tests/walk_lazy_check.hip; f64 scenes on the unordered tree only.
//
// usage: walk_offset_check CASE_DIR...      per CASE_DIR:
//   scene.bin, rays.in, sched.in, assign.in
//   -> tree.out
//   -> lds.out, lds_sl.out (SPHERE_LOOP): S x P x n RayOut, then S x P x B WaveOut; lds.bytes: the staged bytes, as text
// Exit code 0 when it ran; 2 on an I/O, input or HIP error.
#define CR_DIAG 1
#include "pathtrace.hpp"
#include "tree.hpp"
#include "screen.hpp"
#include "handle.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace cr;

struct RayOut {
    int32_t best;        // leaf-order index of the closest primitive, -1 = none
    int32_t mat;         // that record's material index (the corpus gives every primitive its own), -1 = none
    uint64_t t_bits;     // the bits of best_t (an f32's in the low word)
    uint32_t nodes, prims;   // the ray's own node tests and primitive tests
};
struct WaveOut {
    uint32_t rounds, leaf_phases, band_lanes;   // DG_ROUND_WAVE, DG_LEAFPH_WAVE, DG_BAND_LANE
    uint32_t survived;   // how often the wave left the walk loop while a lane still held a parked leaf
    uint32_t unscreened;   // rays that walk_begin_screened put outside screen_in_range (the compare/select form)
    uint32_t resumed;      // lanes that left the walk loop with their walk unfinished and resumed it in the next outer iteration
};

CR_D uint64_t bits_of(double t) { return (uint64_t)__double_as_longlong(t); }
CR_D uint64_t bits_of(float t) { return (uint64_t)__float_as_uint(t); }

constexpr size_t kLdsLimit = 160 * 1024;   // a CU's LDS

template <bool SL>
__global__ void __launch_bounds__(64) walk_kernel(KernelArgs<double> A, const double* rays, const int32_t* assign, int32_t K, uint32_t budget,
                                                  RayOut* out, WaveOut* wout) {
    using real = double;
    using ScreenT = ScreenEntry;
    constexpr int RES = RES_LDS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // pathtrace_body's staging of a SCREEN kernel with the scene whole in LDS: the screening records, then the primitives
    auto copy = [&](const void* src, size_t off, size_t bytes) {
        const uint32_t* s = (const uint32_t*)src;
        uint32_t* d = (uint32_t*)(smem + off);
        for (size_t i = threadIdx.x; i < bytes / 4; i += blockDim.x) d[i] = s[i];
    };
    copy(A.screen, 0, (size_t)A.lds_entries * sizeof(ScreenT));
    const Entry<real>* lds_entries = (const Entry<real>*)smem;
    const void* lds_screen = (const void*)smem;
    const size_t o1 = (((size_t)A.n_entries * sizeof(ScreenT) + 15) & ~(size_t)15);
    copy(A.prims, o1, (size_t)A.n_prims * sizeof(Prim<real>));
    const Prim<real>* prims = (const Prim<real>*)(smem + o1);
    __syncthreads();
    {
        const uint32_t base = screen_lds_base<RES>(smem);
        ScreenT* rec = (ScreenT*)smem;
        for (int32_t i = (int32_t)threadIdx.x; i < A.n_entries; i += (int32_t)blockDim.x) {
            rec[i].skip += base;
            if (!(rec[i].hit & kScreenLeaf)) rec[i].hit += base;
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x;
    const int32_t* queue = assign + ((size_t)blockIdx.x * 64 + lane) * (size_t)K;
    const int32_t n_entries = A.n_entries;
    Diag dg;
    for (int k = 0; k < DG_N; k++) dg.v[k] = 0;
    unsigned long long c_node = 0, node0 = 0;
    uint32_t c_prim = 0, prim0 = 0, survived = 0, unscreened = 0, resumed = 0;
    int32_t qi = 0, cur = -1;
    bool walking = false;
    V3<real> ro = mk<real>(0, 0, 0), rd = mk<real>(0, 0, 1);
    real rtime = 0;
    const uint32_t start = screen_lds_base<RES>(smem), end = start + ((uint32_t)n_entries << 5);
    WalkOffset ws;
    ws.invf = mk<float>(0, 0, 0); ws.unscreened = false;
    ws.dd = 0; ws.rda = quot_divide<real>(); ws.best_t = 0; ws.best = -1; ws.off = end; ws.pending = -1;
    for (;;) {
        if (cur < 0 && qi < K && queue[qi] >= 0) {   // the lane's next ray
            cur = queue[qi++];
            const double* r = rays + 7 * (size_t)cur;
            ro = mk<real>((real)r[0], (real)r[1], (real)r[2]);
            rd = mk<real>((real)r[3], (real)r[4], (real)r[5]);
            rtime = (real)r[6];
            walk_begin_screened<true>(ws, ro, rd, start);
            if (ws.unscreened) unscreened++;
            node0 = c_node; prim0 = c_prim;
            walking = n_entries > 0;
        }
        if (!__ballot(cur >= 0)) break;
        if (__ballot(walking)) {
            for (;;) {   // pathtrace_body's walk loop
                walk_round<real, RES, false, false, true, true, true, SL>(A, lds_entries, prims, ro, rd, rtime, ws, walking, budget, c_node, c_prim, &dg, lds_screen);
                if (walking && ws.off >= end && ws.pending < 0) walking = false;
                const uint64_t w = __ballot(walking);
                if (!w || 64u - (uint32_t)__popcll(w) >= A.walk_exit_lanes) break;
            }
            if (__ballot(walking && ws.pending >= 0) && lane == 0) survived++;
            if (walking) resumed++;
        }
        if (cur >= 0 && !walking) {   // the walk is complete
            RayOut o;
            o.best = ws.best;
            o.mat = ws.best >= 0 ? A.prims[ws.best].mat() : -1;
            o.t_bits = bits_of(ws.best_t);
            o.nodes = (uint32_t)(c_node - node0); o.prims = c_prim - prim0;
            out[cur] = o;
            cur = -1;
        }
    }
    WaveOut* wo = wout + blockIdx.x;
    if (dg.v[DG_ROUND_WAVE]) atomicAdd(&wo->rounds, dg.v[DG_ROUND_WAVE]);
    if (dg.v[DG_LEAFPH_WAVE]) atomicAdd(&wo->leaf_phases, dg.v[DG_LEAFPH_WAVE]);
    if (dg.v[DG_BAND_LANE]) atomicAdd(&wo->band_lanes, dg.v[DG_BAND_LANE]);
    if (survived) atomicAdd(&wo->survived, survived);
    if (unscreened) atomicAdd(&wo->unscreened, unscreened);
    if (resumed) atomicAdd(&wo->resumed, resumed);
}

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)

static bool read_file(const std::string& path, std::vector<char>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "%s: cannot open\n", path.c_str()); return false; }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(len > 0 ? (size_t)len : 0);
    const size_t got = out.empty() ? 0 : fread(out.data(), 1, out.size(), f);
    fclose(f);
    return got == out.size();
}
static bool write_file(const std::string& path, const void* a, size_t na, const void* b = nullptr, size_t nb = 0) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = (na == 0 || fwrite(a, 1, na, f) == na) && (nb == 0 || fwrite(b, 1, nb, f) == nb);
    return (fclose(f) == 0) && ok;
}

// a device copy whose pointer is misaligned by `pad` bytes, as DevBuf::ensure leaves the wrapper arrays (entry_pad)
struct Buf {
    void* base = nullptr;
    void* p = nullptr;
    hipError_t make(const void* src, size_t bytes, size_t pad = 0) {
        hipError_t e = hipMalloc(&base, (bytes ? bytes : 16) + pad);
        if (e != hipSuccess) return e;
        p = (char*)base + pad;
        return bytes && src ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
    ~Buf() { if (base) (void)hipFree(base); }
};

struct Inputs {
    std::vector<CrPrimitive> prims;
    int32_t mode = 0;
    std::vector<double> rays;
    std::vector<int32_t> sched, assign;
    int32_t P = 0, B = 0, K = 0;
    size_t n_rays() const { return rays.size() / 7; }
    size_t S() const { return sched.size() / 3; }
};

template <bool SL>
int run_kernel(const std::string& dir, const char* name, const Inputs& in, KernelArgs<double> A, const double* d_rays, const int32_t* d_assign) {
    A.lds_entries = A.n_entries;
    const size_t lds_bytes = (((size_t)A.n_entries * sizeof(ScreenEntry) + 15) & ~(size_t)15) + (size_t)A.n_prims * sizeof(Prim<double>);
    if (lds_bytes > kLdsLimit) { fprintf(stderr, "%s: the staged tree does not fit\n", dir.c_str()); return 2; }
    CHECK(hipFuncSetAttribute((const void*)walk_kernel<SL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    {
        const std::string text = std::to_string(lds_bytes) + "\n";
        if (!write_file(dir + "/lds.bytes", text.data(), text.size())) return 2;
    }
    const size_t n = in.n_rays(), S = in.S(), per = (size_t)in.P * n, wper = (size_t)in.P * in.B;
    Buf d_out, d_wave;
    CHECK(d_out.make(nullptr, S * per * sizeof(RayOut)));
    CHECK(d_wave.make(nullptr, S * wper * sizeof(WaveOut)));
    CHECK(hipMemset(d_out.p, 0xff, S * per * sizeof(RayOut)));   // a ray that is never written shows
    CHECK(hipMemset(d_wave.p, 0, S * wper * sizeof(WaveOut)));
    for (size_t s = 0; s < S; s++) {
        A.walk_leaf_min = (uint32_t)in.sched[3 * s + 1];
        A.walk_exit_lanes = (uint32_t)in.sched[3 * s + 2];
        for (int32_t p = 0; p < in.P; p++) {
            hipLaunchKernelGGL((walk_kernel<SL>), dim3((unsigned)in.B), dim3(64), lds_bytes, 0, A, d_rays,
                               d_assign + (size_t)p * in.B * 64 * in.K, in.K, (uint32_t)in.sched[3 * s], (RayOut*)d_out.p + s * per + (size_t)p * n,
                               (WaveOut*)d_wave.p + s * wper + (size_t)p * in.B);
        }
        CHECK(hipGetLastError());
    }
    CHECK(hipDeviceSynchronize());
    std::vector<RayOut> out(S * per);
    std::vector<WaveOut> wave(S * wper);
    CHECK(hipMemcpy(out.data(), d_out.p, out.size() * sizeof(RayOut), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(wave.data(), d_wave.p, wave.size() * sizeof(WaveOut), hipMemcpyDeviceToHost));
    if (!write_file(dir + "/" + name + ".out", out.data(), out.size() * sizeof(RayOut), wave.data(), wave.size() * sizeof(WaveOut))) return 2;
    printf("%s %s: %zu rays x %zu schedules x %d permutations, %zu bytes staged\n", dir.c_str(), name, n, S, in.P, lds_bytes);
    return 0;
}

static int run_case(const std::string& dir, const Inputs& in) {
    using real = double;
    // the host stages of build_dev_scene, in its order
    SceneBoxes<real> sb;
    std::vector<int8_t> axis;
    std::vector<int32_t> level_begin;
    Spliced<real> spliced;
    LeafLayout<real> lay;
    scene_boxes(in.prims, in.mode == CR_BVH_REFERENCE, sb);
    host_topology(in.prims, in.mode, sb, axis, level_begin, spliced);
    if (!layout_leaves(in.prims, sb, spliced, lay) || spliced.on) { fprintf(stderr, "%s: a scene this check does not take\n", dir.c_str()); return 2; }
    const std::vector<Entry<real>>& E = sb.b.entries;
    const int32_t ne = (int32_t)E.size();
    if (ne == 0) { fprintf(stderr, "%s: no wrappers\n", dir.c_str()); return 2; }
    for (const int32_t r : in.assign) if (r < -1 || r >= (int32_t)in.n_rays()) { fprintf(stderr, "%s: a ray index out of range\n", dir.c_str()); return 2; }
    {   // the tree as cr_export_bvh returns it
        const std::vector<int32_t> leaf_desc = leaf_descs(sb);
        std::vector<double> boxes((size_t)ne * 6);
        std::vector<int32_t> tail((size_t)ne * 3);
        export_walk(E, axis, leaf_desc, false, boxes.data(), tail.data(), tail.data() + (size_t)ne * 2);
        std::vector<char> head(4 + boxes.size() * 8);
        memcpy(head.data(), &ne, 4);
        memcpy(head.data() + 4, boxes.data(), boxes.size() * 8);
        if (!write_file(dir + "/tree.out", head.data(), head.size(), tail.data(), tail.size() * 4)) return 2;
    }
    // uploads: the records of the mode with entry_pad, the primitive records, the leaf runs
    using Rec = Entry<real>;
    using SRec = ScreenEntry;
    Buf d_entries, d_prims, d_runs, d_screen, d_flag, d_rays, d_assign;
    {
        const std::vector<Entry<real>>& dev = lay.own_entries ? lay.dev_entries : E;
        CHECK(d_entries.make(dev.data(), dev.size() * sizeof(Entry<real>), entry_pad<Rec>()));
    }
    CHECK(d_prims.make(lay.leaf_prims.data(), lay.leaf_prims.size() * sizeof(Prim<real>)));
    CHECK(d_runs.make(lay.leaf_runs.data(), lay.leaf_runs.size() * sizeof(int32_t)));
    CHECK(d_rays.make(in.rays.data(), in.rays.size() * sizeof(double)));
    CHECK(d_assign.make(in.assign.data(), in.assign.size() * sizeof(int32_t)));
    // the screening records (scene.hip make_screen)
    {
        const int32_t zero = 0;
        CHECK(d_flag.make(&zero, sizeof zero));
        CHECK(d_screen.make(nullptr, (size_t)ne * sizeof(SRec), entry_pad<SRec>()));
        const dim3 grid((unsigned)((ne + 255) / 256));
        hipLaunchKernelGGL(screen_from_entries_kernel<real>, grid, dim3(256), 0, 0, (const Entry<real>*)d_entries.p, (ScreenEntry*)d_screen.p, ne, (int32_t*)d_flag.p);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        int32_t overflow = 0;
        CHECK(hipMemcpy(&overflow, d_flag.p, sizeof overflow, hipMemcpyDeviceToHost));
        if (overflow) { fprintf(stderr, "%s: a box plane beyond the f32 range\n", dir.c_str()); return 2; }
    }
    KernelArgs<real> A;
    memset(&A, 0, sizeof A);
    A.entries = (const Entry<real>*)d_entries.p;
    A.prims = (const Prim<real>*)d_prims.p;
    A.leaf_runs = lay.leaf_runs.empty() ? nullptr : (const int32_t*)d_runs.p;
    A.screen = d_screen.p;
    A.n_entries = ne; A.n_prims = (int32_t)lay.leaf_prims.size();
    A.lds_entries = 0;
    A.uniform_kind = (sb.kinds.has_spheres && !sb.kinds.has_triangles) ? 0 : ((sb.kinds.has_triangles && !sb.kinds.has_spheres) ? 1 : -1);
    const double* rays = (const double*)d_rays.p;
    const int32_t* assign = (const int32_t*)d_assign.p;
    if (!lay.leaf_runs.empty()) { fprintf(stderr, "%s: a list element (the static kernels do not walk one)\n", dir.c_str()); return 2; }
    int rc = run_kernel<false>(dir, "lds", in, A, rays, assign);
    if (rc == 0) rc = run_kernel<true>(dir, "lds_sl", in, A, rays, assign);
    return rc;
}

static int run_dir(const std::string& dir) {
    std::vector<char> scene, rays, sched, assign;
    if (!read_file(dir + "/scene.bin", scene) || !read_file(dir + "/rays.in", rays) || !read_file(dir + "/sched.in", sched) ||
        !read_file(dir + "/assign.in", assign)) return 2;
    Inputs in;
    int32_t head[3];
    if (scene.size() < sizeof head) return 2;
    memcpy(head, scene.data(), sizeof head);
    if (head[2] < 0 || scene.size() != sizeof head + (size_t)head[2] * sizeof(CrPrimitive)) { fprintf(stderr, "%s/scene.bin: bad size\n", dir.c_str()); return 2; }
    in.mode = head[1];
    in.prims.resize((size_t)head[2]);
    if (head[2]) memcpy(in.prims.data(), scene.data() + sizeof head, scene.size() - sizeof head);
    if (rays.empty() || rays.size() % 56 || sched.empty() || sched.size() % 12 || assign.size() < 12) { fprintf(stderr, "%s: bad input sizes\n", dir.c_str()); return 2; }
    in.rays.resize(rays.size() / 8);
    memcpy(in.rays.data(), rays.data(), rays.size());
    in.sched.resize(sched.size() / 4);
    memcpy(in.sched.data(), sched.data(), sched.size());
    int32_t pbk[3];
    memcpy(pbk, assign.data(), sizeof pbk);
    in.P = pbk[0]; in.B = pbk[1]; in.K = pbk[2];
    if (in.P < 1 || in.B < 1 || in.K < 1 || assign.size() != 12 + (size_t)in.P * in.B * 64 * in.K * 4) { fprintf(stderr, "%s/assign.in: bad size\n", dir.c_str()); return 2; }
    in.assign.resize((assign.size() - 12) / 4);
    memcpy(in.assign.data(), assign.data() + 12, assign.size() - 12);
    for (size_t s = 0; s < in.S(); s++)
        if (in.sched[3 * s] < 0 || in.sched[3 * s + 1] < 0 || in.sched[3 * s + 1] > 64 || in.sched[3 * s + 2] < 1 || in.sched[3 * s + 2] > 64) {
            fprintf(stderr, "%s/sched.in: a knob outside the range cr_create accepts\n", dir.c_str());
            return 2;
        }
    if (in.mode != CR_BVH_REFERENCE) { fprintf(stderr, "%s: CR_BVH_REFERENCE\n", dir.c_str()); return 2; }
    if (!head[0]) { fprintf(stderr, "%s: an f64 scene\n", dir.c_str()); return 2; }
    return run_case(dir, in);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: walk_offset_check CASE_DIR...\n"); return 2; }
    for (int i = 1; i < argc; i++) {
        const int rc = run_dir(argv[i]);
        if (rc != 0) return rc;
    }
    return 0;
}
