// Device check for tests/test_gpu_walk_primitives.py: runs the walk's per-ray primitives of crucible_amd/csrc/pathtrace.hpp on
// the device -- the f64 screen and the f32 record test of walk_round, the box, sphere and triangle tests, the screened rejection
// samplers and the software trigonometry -- on inputs the test writes, and writes the results back for the test to compare
// with the CPU oracle and with exact references.
//
// usage: walk_check DIR.  Every input file is optional; a part runs when its file exists.
//   DIR/box.in      n x 13 f64: box planes x0 x1 y0 y1 z0 z1, origin, direction, tmax   -> DIR/box.out   n x BoxOut
//   DIR/prim.in     n x 17 f64: kind (0 sphere, 1 triangle), g[9], origin, direction, tmax -> DIR/prim.out n x PrimOut
//   DIR/trig.in     n x 2 f64: y, x                                 -> DIR/trig64.out n x 3 f64, DIR/trig32.out n x 3 f32
//   DIR/sampler.in  2 u64: number of stream keys, first key         -> DIR/sampler.out 8 u64 (see sampler_kernel)
// The f32 forms take the f32 roundings of the same inputs.  Exit code 0 when every part ran; 2 on an I/O or HIP error.
#include "pathtrace.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cr;

struct BoxOut {
    float d, th;      // f64 screen: hi32 - lo32 and its TH (meaningful when screened)
    uint32_t flags;   // see the BF_ bits
};
enum : uint32_t {
    BF_SCREENED = 1u << 0,      // f64: finite 1/dir and inside the screen's range
    BF_EXACT64 = 1u << 1,       // f64 walk_begin's exact_box
    BF_HIT64 = 1u << 2,         // box_hit<double>
    BF_FAST_HIT64 = 1u << 3,    // box_hit_fast<double>
    BF_FAST_MISS64 = 1u << 4,   // box_miss_fast<double>
    BF_EXACT32 = 1u << 5,       // f32 walk_begin's exact_box
    BF_HIT32 = 1u << 6,         // box_hit<float>
    BF_FAST_HIT32 = 1u << 7,    // box_hit_fast<float>
    BF_FAST_MISS32 = 1u << 8,   // box_miss_fast<float>
    BF_REC_MISS32 = 1u << 9,    // screen_box_miss_exact: the f32 kernels' test on the record
    BF_OVERFLOW = 1u << 10,     // screen_plane: a finite f64 plane beyond the f32 range (the tree is walked without the screen)
};

__global__ void box_kernel(const double* in, BoxOut* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* c = in + 13 * i;
    const double tmax = c[12];
    uint32_t flags = 0;
    BoxOut o;
    {   // f64: the screen of a SCREEN kernel, on the record screen_from_entries_kernel makes (screen_plane)
        const double b[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
        const V3<double> ro = mk<double>(c[6], c[7], c[8]), rd = mk<double>(c[9], c[10], c[11]);
        WalkState<double> w;
        walk_begin(w, rd);
        float b32[6];
        int32_t overflow = 0;
        for (int k = 0; k < 6; k++) screen_plane(b[k], b32[k], &overflow);
        if (overflow) flags |= BF_OVERFLOW;
        const float ofx = (float)ro.x, ofy = (float)ro.y, ofz = (float)ro.z;
        const float ifx = (float)w.inv.x, ify = (float)w.inv.y, ifz = (float)w.inv.z;
        float mo, pmax, pmin;
        screen_extents(ofx, ofy, ofz, ifx, ify, ifz, mo, pmax, pmin);
        if (screen_in_range(w.exact_box, mo, pmax, pmin)) flags |= BF_SCREENED;
        if (w.exact_box) flags |= BF_EXACT64;
        const float th0 = screen_th0(screen_q(ofx, ifx), screen_q(ofy, ify), screen_q(ofz, ifz), pmax);
        o.d = screen_box_d(b32, Pair<float>{ofx, ofx}, Pair<float>{ofy, ofy}, Pair<float>{ofz, ofz}, Pair<float>{ifx, ifx},
                           Pair<float>{ify, ify}, Pair<float>{ifz, ifz}, 0.001f, (float)tmax, th0, o.th);
        if (box_hit<double>(b, ro, w.inv, 0.001, tmax)) flags |= BF_HIT64;
        const Pair<double> ox = {ro.x, ro.x}, oy = {ro.y, ro.y}, oz = {ro.z, ro.z};
        const Pair<double> ix = {w.inv.x, w.inv.x}, iy = {w.inv.y, w.inv.y}, iz = {w.inv.z, w.inv.z};
        if (box_hit_fast<double>(b, ox, oy, oz, ix, iy, iz, 0.001, tmax)) flags |= BF_FAST_HIT64;
        if (box_miss_fast<double>(b, ox, oy, oz, ix, iy, iz, 0.001, tmax)) flags |= BF_FAST_MISS64;
    }
    {   // f32: the same ray and box rounded to f32, as an f32 scene holds them
        float b[6];
        for (int k = 0; k < 6; k++) b[k] = (float)c[k];
        const V3<float> ro = mk<float>((float)c[6], (float)c[7], (float)c[8]), rd = mk<float>((float)c[9], (float)c[10], (float)c[11]);
        const float tmaxf = (float)tmax;
        WalkState<float> w;
        walk_begin(w, rd);
        if (w.exact_box) flags |= BF_EXACT32;
        if (box_hit<float>(b, ro, w.inv, 0.001f, tmaxf)) flags |= BF_HIT32;
        const Pair<float> ox = {ro.x, ro.x}, oy = {ro.y, ro.y}, oz = {ro.z, ro.z};
        const Pair<float> ix = {w.inv.x, w.inv.x}, iy = {w.inv.y, w.inv.y}, iz = {w.inv.z, w.inv.z};
        if (box_hit_fast<float>(b, ox, oy, oz, ix, iy, iz, 0.001f, tmaxf)) flags |= BF_FAST_HIT32;
        if (box_miss_fast<float>(b, ox, oy, oz, ix, iy, iz, 0.001f, tmaxf)) flags |= BF_FAST_MISS32;
        if (screen_box_miss_exact(b, ox, oy, oz, ix, iy, iz, 0.001f, tmaxf)) flags |= BF_REC_MISS32;
    }
    o.flags = flags;
    out[i] = o;
}

struct PrimOut {
    double t64;
    float t32;
    uint32_t flags;   // bit 0: hit in f64, bit 1: hit in f32
};

template <typename real> __device__ bool prim_t(const double* c, real& t) {
    real g[9];
    for (int k = 0; k < 9; k++) g[k] = (real)c[1 + k];
    const V3<real> ro = mk<real>((real)c[10], (real)c[11], (real)c[12]), rd = mk<real>((real)c[13], (real)c[14], (real)c[15]);
    const real tmax = (real)c[16];
    WalkState<real> w;
    walk_begin(w, rd);
    if (c[0] == 0.0) return sphere_t(g[0], g[1], g[2], g[3], ro, rd, w.dd, real(0.001), tmax, t);
    return triangle_t(mk<real>(g[0], g[1], g[2]), mk<real>(g[3], g[4], g[5]), mk<real>(g[6], g[7], g[8]), ro, rd, real(0.001), tmax, t);
}

__global__ void prim_kernel(const double* in, PrimOut* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PrimOut o;
    o.t64 = 0.0; o.t32 = 0.0f; o.flags = 0;
    double t64;
    float t32;
    if (prim_t<double>(in + 17 * i, t64)) { o.t64 = t64; o.flags |= 1u; }
    if (prim_t<float>(in + 17 * i, t32)) { o.t32 = t32; o.flags |= 2u; }
    out[i] = o;
}

__global__ void trig_kernel(const double* in, double* out64, float* out32, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double y = in[2 * i], x = in[2 * i + 1];
    out64[3 * i] = soft_atan2<double>(y, x);
    out64[3 * i + 1] = soft_asin<double>(y);
    out64[3 * i + 2] = soft_acos<double>(y);
    const float yf = (float)y, xf = (float)x;
    out32[3 * i] = soft_atan2<float>(yf, xf);
    out32[3 * i + 1] = soft_asin<float>(yf);
    out32[3 * i + 2] = soft_acos<float>(yf);
}

// The f32 screen value of a candidate and whether the screened samplers must decide it in f64: the band (written out here,
// independently of the samplers, so that a narrowed band in pathtrace.hpp still counts the candidates it should have caught).
__device__ bool unit_vector_in_band(uint64_t ux, uint64_t uy, uint64_t uz) {
    const float fx = screen_coord(ux), fy = screen_coord(uy), fz = screen_coord(uz);
    const float lf = fx * fx + fy * fy + fz * fz;
    return !(lf > 1.0f + 1e-5f) && !(lf > 1e-5f && lf < 1.0f - 1e-5f);
}
__device__ bool disk_in_band(uint64_t ux, uint64_t uy) {
    const float fx = screen_coord(ux), fy = screen_coord(uy);
    const float lf = fx * fx + fy * fy;
    return !(lf > 1.0f + 1e-5f) && !(lf < 1.0f - 1e-5f);
}

__device__ uint64_t stream_key(uint64_t i) {   // splitmix64: well spread stream states
    uint64_t z = i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// res[0]: unit vector mismatches (result bits or RNG state), res[1]: disk mismatches, res[2]: unit vector candidates in the
// f64 band, res[3]: disk candidates in the band, res[4]/res[5]: smallest mismatching key index (unit vector / disk), res[6]:
// unit vector rounds, res[7]: disk rounds
__global__ void sampler_kernel(uint64_t n, uint64_t first, unsigned long long* res) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = stream_key(first + i);
    unsigned long long band_uv = 0, band_disk = 0, rounds_uv = 0, rounds_disk = 0;
    {
        uint64_t s1 = key, s2 = key, s3 = key;
        const V3<double> a = random_unit_vector_dev<double>(s1);
        const V3<double> b = random_unit_vector<double>(s2);   // the plain loop (utils.rs:127-136)
        for (;;) {   // the rounds of the plain loop again, counted
            const uint64_t ux = rng_next(s3), uy = rng_next(s3), uz = rng_next(s3);
            rounds_uv++;
            if (unit_vector_in_band(ux, uy, uz)) band_uv++;
            const double x = -1.0 + 2.0 * u01(ux, 0.0), y = -1.0 + 2.0 * u01(uy, 0.0), z = -1.0 + 2.0 * u01(uz, 0.0);
            const double lensq = x * x + y * y + z * z;
            if (RealTraits<double>::tiny < lensq && lensq <= 1.0) break;
        }
        const bool same = __double_as_longlong(a.x) == __double_as_longlong(b.x) && __double_as_longlong(a.y) == __double_as_longlong(b.y) &&
                          __double_as_longlong(a.z) == __double_as_longlong(b.z) && s1 == s2;
        if (!same) { atomicAdd(&res[0], 1ull); atomicMin(&res[4], (unsigned long long)i); }
    }
    {
        uint64_t s1 = key, s2 = key;
        double ax, ay, px, py;
        random_in_unit_disk_dev<double>(s1, ax, ay);
        for (;;) {   // random_in_unit_disk (utils.rs:110-124) written out: rng_range(-1, 1) twice, then the test with z = 0
            const uint64_t ux = rng_next(s2);
            px = -1.0 + (1.0 - -1.0) * u01(ux, 0.0);
            const uint64_t uy = rng_next(s2);
            py = -1.0 + (1.0 - -1.0) * u01(uy, 0.0);
            rounds_disk++;
            if (disk_in_band(ux, uy)) band_disk++;
            if (px * px + py * py + 0.0 * 0.0 < 1.0) break;
        }
        const bool same = __double_as_longlong(ax) == __double_as_longlong(px) && __double_as_longlong(ay) == __double_as_longlong(py) && s1 == s2;
        if (!same) { atomicAdd(&res[1], 1ull); atomicMin(&res[5], (unsigned long long)i); }
    }
    if (band_uv) atomicAdd(&res[2], band_uv);
    if (band_disk) atomicAdd(&res[3], band_disk);
    atomicAdd(&res[6], rounds_uv);
    atomicAdd(&res[7], rounds_disk);
}

static bool read_file(const std::string& path, std::vector<char>& buf) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t)(len > 0 ? len : 0));
    const size_t got = buf.empty() ? 0 : fread(buf.data(), 1, buf.size(), f);
    fclose(f);
    return got == buf.size();
}
static bool write_file(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = fwrite(p, 1, bytes, f);
    return fclose(f) == 0 && put == bytes;
}

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)

// Copies `in` to the device, runs `launch(device_in, n)` and copies `out_bytes` of each output back.
template <typename Launch>
static int run_part(const std::vector<char>& in, size_t n, std::vector<std::vector<char>*> outs, std::vector<size_t> out_bytes, Launch launch) {
    void* din = nullptr;
    std::vector<void*> douts(outs.size(), nullptr);
    CHECK(hipMalloc(&din, in.size()));
    CHECK(hipMemcpy(din, in.data(), in.size(), hipMemcpyHostToDevice));
    for (size_t k = 0; k < outs.size(); k++) CHECK(hipMalloc(&douts[k], out_bytes[k]));
    launch(din, douts, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    for (size_t k = 0; k < outs.size(); k++) {
        outs[k]->resize(out_bytes[k]);
        CHECK(hipMemcpy(outs[k]->data(), douts[k], out_bytes[k], hipMemcpyDeviceToHost));
        CHECK(hipFree(douts[k]));
    }
    CHECK(hipFree(din));
    return 0;
}

static dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: walk_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::vector<char> in, o1, o2;
    if (read_file(dir + "/box.in", in) && !in.empty()) {
        if (in.size() % (13 * 8)) { fprintf(stderr, "box.in: bad size\n"); return 2; }
        const size_t n = in.size() / (13 * 8);
        if (run_part(in, n, {&o1}, {n * sizeof(BoxOut)}, [](void* d, std::vector<void*>& o, size_t m) {
                hipLaunchKernelGGL(box_kernel, grid_for(m), dim3(256), 0, 0, (const double*)d, (BoxOut*)o[0], m); }))
            return 2;
        if (!write_file(dir + "/box.out", o1.data(), o1.size())) return 2;
        printf("box: %zu cases\n", n);
    }
    if (read_file(dir + "/prim.in", in) && !in.empty()) {
        if (in.size() % (17 * 8)) { fprintf(stderr, "prim.in: bad size\n"); return 2; }
        const size_t n = in.size() / (17 * 8);
        if (run_part(in, n, {&o1}, {n * sizeof(PrimOut)}, [](void* d, std::vector<void*>& o, size_t m) {
                hipLaunchKernelGGL(prim_kernel, grid_for(m), dim3(256), 0, 0, (const double*)d, (PrimOut*)o[0], m); }))
            return 2;
        if (!write_file(dir + "/prim.out", o1.data(), o1.size())) return 2;
        printf("prim: %zu cases\n", n);
    }
    if (read_file(dir + "/trig.in", in) && !in.empty()) {
        if (in.size() % 16) { fprintf(stderr, "trig.in: bad size\n"); return 2; }
        const size_t n = in.size() / 16;
        if (run_part(in, n, {&o1, &o2}, {n * 24, n * 12}, [](void* d, std::vector<void*>& o, size_t m) {
                hipLaunchKernelGGL(trig_kernel, grid_for(m), dim3(256), 0, 0, (const double*)d, (double*)o[0], (float*)o[1], m); }))
            return 2;
        if (!write_file(dir + "/trig64.out", o1.data(), o1.size()) || !write_file(dir + "/trig32.out", o2.data(), o2.size())) return 2;
        printf("trig: %zu cases\n", n);
    }
    if (read_file(dir + "/sampler.in", in) && !in.empty()) {
        if (in.size() != 16) { fprintf(stderr, "sampler.in: bad size\n"); return 2; }
        uint64_t hdr[2];
        memcpy(hdr, in.data(), 16);
        unsigned long long init[8] = {0, 0, 0, 0, ~0ull, ~0ull, 0, 0}, *dres = nullptr;
        CHECK(hipMalloc(&dres, sizeof init));
        CHECK(hipMemcpy(dres, init, sizeof init, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(sampler_kernel, grid_for(hdr[0]), dim3(256), 0, 0, hdr[0], hdr[1], dres);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(init, dres, sizeof init, hipMemcpyDeviceToHost));
        CHECK(hipFree(dres));
        if (!write_file(dir + "/sampler.out", init, sizeof init)) return 2;
        printf("sampler: %llu keys\n", (unsigned long long)hdr[0]);
    }
    return 0;
}
