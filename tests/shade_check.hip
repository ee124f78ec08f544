// Device check for tests/test_gpu_shade_primitives.py: runs what a path does around the walk -- shade() after a closest hit
// and after a miss, the texture lookup, camera_ray, the timeline and the refit rule of crucible_amd/csrc/refit.hpp -- on
// inputs the test writes, and writes the results back for the test to compare with the CPU oracle and exact references.
// The scene records are packed from the C-ABI descriptors by crucible_amd/csrc/pack.hpp, the library's own packing.
//
// usage: shade_check DIR [--host].  Every input file except DIR/scene.bin is optional; a part runs when its file exists.
//   DIR/scene.bin     int32 n_prims n_mats n_texs n_images n_keys sky_kind sky_image, then CrPrimitive[n_prims],
//                     CrMaterial[n_mats], CrTexture[n_texs], CrKeyframe[n_keys], then per image int32 w, h and w*h*3 bytes
//   DIR/hit.in        n x 12 f64: prim, best_t (f64), best_t (f32), ro[3], rd[3], rtime, pixel, sample (the RNG key of
//                     (seed, pixel, sample), the seed in DIR/seed.in); best_t < 0: no hit in that precision, the case is skipped
//                     -> DIR/hit{64,32}.out: n x HIT_VARIANTS x HIT_WORDS f64
//   DIR/sky.in        n x 3 f64 directions -> DIR/sky{64,32}.out: n x 2 sky kinds x 4 x 4 f64 (colour, texel reads) for: the
//                     reference order with an empty stack, relaxed with thr = 1, the reference order unwinding the
//                     STACK_LEVELS records of DIR/stack.in, relaxed with thr = their product in path order
//   DIR/stack.in      STACK_LEVELS x 3 f64 attenuations (default 1): the stacked misses; the first is also a hit's
//                     starting thr in the relaxed variants
//   DIR/texture.in    n x 6 f64: texture (scene index), u, v, p[3] -> DIR/texture{64,32}.out: n x 4 f64 (colour, texel reads)
//   DIR/camera.in     records (see read_cameras) -> DIR/camera{64,32}.out: per sample 8 f64 (origin, direction, time, draws)
//   DIR/timeline.in   n x 2 f64: prim, t -> DIR/timeline{64,32}.out: n x 9 f64 (sphere: centre, radius; triangle: a, b, c)
//   DIR/refit.in      n x 5 f64: prim, ta64, tb64, ta32, tb32 -> DIR/refit{64,32}.out: n x 6 f64 (lo xyz, hi xyz)
// Every result is written as f64 (an f32 result converts exactly).  --host: only the timeline and refit parts, run on the
// CPU through the same __host__ __device__ functions (no GPU needed).  Exit code 0 when every part ran; 2 on an I/O or HIP error.
#include "pathtrace.hpp"
#include "pack.hpp"
#include "refit.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cr;

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

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); exit(2); } } while (0)

// ------------------------------------------------------------------ the scene, as the descriptors the C ABI receives
struct SceneIn {
    int32_t sky_kind = 0, sky_image = -1;
    std::vector<CrPrimitive> prims;
    std::vector<CrMaterial> mats;
    std::vector<CrTexture> texs;
    std::vector<CrKeyframe> keys;
    std::vector<CrImage> images;
    std::vector<std::vector<uint8_t>> rgb;
};

static bool read_scene(const std::string& path, SceneIn& s) {
    std::vector<char> b;
    if (!read_file(path, b) || b.size() < 28) return false;
    size_t at = 0;
    auto take = [&](void* dst, size_t bytes) { if (at + bytes > b.size()) return false; memcpy(dst, b.data() + at, bytes); at += bytes; return true; };
    int32_t h[7];
    if (!take(h, sizeof h)) return false;
    for (int k = 0; k < 5; k++) if (h[k] < 0 || h[k] > (1 << 20)) return false;
    s.prims.resize(h[0]); s.mats.resize(h[1]); s.texs.resize(h[2]); s.keys.resize(h[4]);
    s.sky_kind = h[5]; s.sky_image = h[6];
    if (!take(s.prims.data(), h[0] * sizeof(CrPrimitive)) || !take(s.mats.data(), h[1] * sizeof(CrMaterial)) ||
        !take(s.texs.data(), h[2] * sizeof(CrTexture)) || !take(s.keys.data(), h[4] * sizeof(CrKeyframe))) return false;
    s.rgb.resize(h[3]);
    s.images.resize(h[3]);
    for (int i = 0; i < h[3]; i++) {
        int32_t wh[2];
        if (!take(wh, sizeof wh) || wh[0] < 1 || wh[1] < 1 || (size_t)wh[0] * wh[1] > ((size_t)1 << 26)) return false;
        s.rgb[i].resize((size_t)wh[0] * wh[1] * 3);
        if (!take(s.rgb[i].data(), s.rgb[i].size())) return false;
        s.images[i].width = wh[0]; s.images[i].height = wh[1]; s.images[i].rgb8 = s.rgb[i].data();
    }
    // indices the device follows must stay in range
    for (const CrPrimitive& p : s.prims)
        if (p.material < 0 || p.material >= h[1] || p.key_first < 0 || p.key_count < 0 || p.key_first + p.key_count > h[4]) return false;
    for (const CrMaterial& m : s.mats) if (m.kind == CR_MAT_LAMBERTIAN && (m.texture < 0 || m.texture >= h[2])) return false;
    for (const CrTexture& t : s.texs) {
        if (t.kind == CR_TEX_CHECKER && (t.even < 0 || t.even >= h[2] || t.odd < 0 || t.odd >= h[2])) return false;
        if (t.kind == CR_TEX_IMAGE && (t.image < 0 || t.image >= h[3])) return false;
    }
    if (s.sky_kind == CR_SKY_SPHERICAL && (s.sky_image < 0 || s.sky_image >= h[3])) return false;
    return at == b.size();
}

// The scene in `real`, packed by pack.hpp.  Primitives keep the descriptor's order (index = descriptor index); every
// texture is kept (the remap of an all-live table), so a texture's device index is its descriptor index.
template <typename real> struct Packed {
    std::vector<Prim<real>> prims;
    std::vector<Mat<real>> mats;
    std::vector<Tex<real>> texs;
    std::vector<Key<real>> keys;
    std::vector<ImageRef> refs;
    std::vector<uint32_t> texels;
    std::vector<int32_t> remap;
};
template <typename real> static bool pack(const SceneIn& s, Packed<real>& P) {
    for (const CrPrimitive& p : s.prims) P.prims.push_back(pack_prim<real>(p));
    P.remap = live_texture_remap(s.mats.data(), s.mats.size(), s.texs.data(), s.texs.size());
    for (const CrMaterial& m : s.mats) P.mats.push_back(pack_mat<real>(m, s.texs.data(), P.remap.data()));
    for (size_t i = 0; i < s.texs.size(); i++) if (P.remap[i] >= 0) P.texs.push_back(pack_tex<real>(s.texs[i], P.remap.data()));
    P.keys.resize(s.keys.size());
    for (size_t i = 0; i < s.keys.size(); i++) key_to_real(s.keys[i], P.keys[i]);
    return pack_images(s.images.data(), (int32_t)s.images.size(), P.refs, P.texels);
}

// Every table gets 64 KiB of zeroed slack behind it: an index one row past a table's end reads zeros rather than faulting.
constexpr size_t kSlack = 1 << 16;
template <typename T> static T* to_dev(const std::vector<T>& v) {
    T* d = nullptr;
    CHECK(hipMalloc(&d, v.size() * sizeof(T) + kSlack));
    CHECK(hipMemset(d, 0, v.size() * sizeof(T) + kSlack));
    if (!v.empty()) CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> static std::vector<T> from_dev(const T* d, size_t n) {
    std::vector<T> v(n);
    CHECK(hipDeviceSynchronize());
    if (n) CHECK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

// The device copy of a packed scene, as KernelArgs sees it.
template <typename real> struct DevScene {
    KernelArgs<real> A;
    std::vector<void*> bufs;
    DevScene(const SceneIn& s, const Packed<real>& P, uint64_t seed) {
        memset(&A, 0, sizeof A);
        A.prims = to_dev(P.prims); A.mats = to_dev(P.mats); A.texs = to_dev(P.texs); A.keys = to_dev(P.keys);
        A.images = to_dev(P.refs); A.texels = to_dev(P.texels);
        A.n_prims = (int32_t)P.prims.size(); A.n_mats = (int32_t)P.mats.size(); A.n_texs = (int32_t)P.texs.size();
        A.sky_kind = s.sky_kind; A.sky_image = s.sky_image;
        A.seed_mixed = mix64(seed + RNG_GAMMA);
        bufs = {(void*)A.prims, (void*)A.mats, (void*)A.texs, (void*)A.keys, (void*)A.images, (void*)A.texels};
    }
    ~DevScene() { for (void* p : bufs) (void)hipFree(p); }
};

// Draws taken between the key and the final state: a copy of the key stepped until it equals the final state (-1: more than 64).
CR_HD double draws_between(uint64_t key, uint64_t final_state) {
    for (int k = 0; k <= 64; k++) {
        if (key == final_state) return (double)k;
        (void)rng_next(key);
    }
    return -1.0;
}

// ------------------------------------------------------------------ hit: shade() after a closest hit
// Per case and variant: finished, col[3], ro[3], rd[3], depth_left, att[3] (the pushed record, or thr), records pushed, c_tex,
// draws, 0.
constexpr int HIT_WORDS = 18;
constexpr int HIT_VARIANTS = 4;   // (ANIM, RELAX): (1,0) (1,1) (0,0) (0,1)

template <typename real, bool ANIM, bool RELAX>
__device__ void shade_hit_one(const KernelArgs<real>& A, const double* c, real* att_rec, const double* A_fac, double* o) {
    V3<real> ro = mk<real>((real)c[3], (real)c[4], (real)c[5]), rd = mk<real>((real)c[6], (real)c[7], (real)c[8]);
    const real best_t = (real)(sizeof(real) == 8 ? c[1] : c[2]), rtime = (real)c[9];
    const uint64_t key = rng_key(A.seed_mixed, (uint32_t)c[10], (uint32_t)c[11]);
    uint64_t rng = key;
    int32_t depth_left = 10, stack_n = 0;
    uint32_t c_tex = 0;
    V3<real> col = mk<real>(-7, -7, -7), thr = mk<real>((real)A_fac[0], (real)A_fac[1], (real)A_fac[2]);
    att_rec[0] = real(-7); att_rec[1] = real(-7); att_rec[2] = real(-7);
    const bool fin = shade<real, ANIM, false, RELAX>(A, A.prims, A.mats, A.texs, ro, rd, rtime, rng, depth_left, stack_n, best_t, (int32_t)c[0],
                                                     1, 0, c_tex, col, nullptr, &thr);
    o[0] = fin; o[1] = col.x; o[2] = col.y; o[3] = col.z;
    o[4] = ro.x; o[5] = ro.y; o[6] = ro.z; o[7] = rd.x; o[8] = rd.y; o[9] = rd.z; o[10] = depth_left;
    if (RELAX) { o[11] = thr.x; o[12] = thr.y; o[13] = thr.z; o[14] = 0; }
    else { o[11] = att_rec[0]; o[12] = att_rec[1]; o[13] = att_rec[2]; o[14] = stack_n; }
    o[15] = c_tex; o[16] = draws_between(key, rng); o[17] = 0;
}

template <typename real>
__global__ void hit_kernel(KernelArgs<real> A, const double* in, double* out, real* att, const double* fac, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* c = in + 12 * i;
    double* o = out + (size_t)HIT_VARIANTS * HIT_WORDS * i;
    if (!((sizeof(real) == 8 ? c[1] : c[2]) >= 0)) { for (int k = 0; k < HIT_VARIANTS * HIT_WORDS; k++) o[k] = 0; return; }
    KernelArgs<real> B = A;
    B.att_stack = att + 3 * i;   // one record: level 0 of a stack with stride 1 at this case's own slot
    const bool keyed = A.prims[(int32_t)c[0]].key_count > 0;
    shade_hit_one<real, true, false>(B, c, att + 3 * i, fac, o);
    shade_hit_one<real, true, true>(B, c, att + 3 * i, fac, o + HIT_WORDS);
    if (!keyed) {   // the static kernels never see a keyed primitive
        shade_hit_one<real, false, false>(B, c, att + 3 * i, fac, o + 2 * HIT_WORDS);
        shade_hit_one<real, false, true>(B, c, att + 3 * i, fac, o + 3 * HIT_WORDS);
    } else for (int k = 2 * HIT_WORDS; k < 4 * HIT_WORDS; k++) o[k] = 0;
}

// ------------------------------------------------------------------ sky: shade() after a miss
constexpr int STACK_LEVELS = 5;   // more than one round of the unwind's four-level loop, and its remainder loop

template <typename real, bool RELAX>
__device__ void shade_miss_one(const KernelArgs<real>& A, const double* d, int32_t stack_n, uint32_t stride, uint32_t slot, V3<real> thr, double* o) {
    V3<real> ro = mk<real>(0, 0, 0), rd = mk<real>((real)d[0], (real)d[1], (real)d[2]), col = mk<real>(-7, -7, -7);
    uint64_t rng = 1;
    int32_t depth_left = 10;
    uint32_t c_tex = 0;
    shade<real, false, false, RELAX>(A, A.prims, A.mats, A.texs, ro, rd, real(0), rng, depth_left, stack_n, real(-1), -1, stride, slot, c_tex, col,
                                     nullptr, &thr);
    o[0] = col.x; o[1] = col.y; o[2] = col.z; o[3] = c_tex;
}
// att: STACK_LEVELS records per case, level-major (level k of case i at (k * n + i) * 3), as the kernels lay out the stack.
template <typename real> __global__ void sky_kernel(KernelArgs<real> A, const double* in, double* out, real* att, const double* fac, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3<real> prod = mk<real>((real)fac[0], (real)fac[1], (real)fac[2]);   // a_1 * a_2 * ... in path order, as shade() forms thr
    for (int k = 0; k < STACK_LEVELS; k++) {
        real* rec = att + ((size_t)k * n + i) * 3;
        for (int c = 0; c < 3; c++) rec[c] = (real)fac[3 * k + c];
        if (k > 0) prod = mk<real>(prod.x * rec[0], prod.y * rec[1], prod.z * rec[2]);
    }
    for (int kind = 0; kind < 2; kind++) {
        KernelArgs<real> B = A;
        B.sky_kind = kind;
        B.att_stack = att;
        double* o = out + 32 * i + 16 * kind;
        shade_miss_one<real, false>(B, in + 3 * i, 0, 1, 0, mk<real>(1, 1, 1), o);
        shade_miss_one<real, true>(B, in + 3 * i, 0, 1, 0, mk<real>(1, 1, 1), o + 4);
        shade_miss_one<real, false>(B, in + 3 * i, STACK_LEVELS, (uint32_t)n, (uint32_t)i, mk<real>(1, 1, 1), o + 8);
        shade_miss_one<real, true>(B, in + 3 * i, 0, 1, 0, prod, o + 12);
    }
}

// ------------------------------------------------------------------ texture: CR_CHECKER_LEAF + image_lookup, as shade() reads a texture
template <typename real> __global__ void texture_kernel(KernelArgs<real> A, const int32_t* remap, const double* in, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* c = in + 6 * i;
    int ti = remap[(int32_t)c[0]];
    Tex<real> tx = A.texs[ti];
    auto tex_at = [&](int32_t k) { return A.texs[k]; };
    const V3<real> p = mk<real>((real)c[3], (real)c[4], (real)c[5]);
    CR_CHECKER_LEAF(tex_at, ti, tx, p)
    uint32_t c_tex = 0;
    V3<real> col;
    if (tx.kind == 2) col = image_lookup(A.images, A.texels, tx.image, (real)c[1], (real)c[2], c_tex);
    else col = mk<real>(tx.color[0], tx.color[1], tx.color[2]);
    double* o = out + 4 * i;
    o[0] = col.x; o[1] = col.y; o[2] = col.z; o[3] = c_tex;
}

// ------------------------------------------------------------------ camera: camera_ray
// camera.in: repeated records of CrCameraDesc, CrRenderParams, int32 n_samples, then n_samples x 3 uint32 (i, j, sample) and
// the camera's keys (from_key_count + at_key_count CrKeyframe).  The descriptors' key pointers are ignored.
struct CamCase { CrCameraDesc cd; CrRenderParams p; std::vector<CrKeyframe> keys; std::vector<uint32_t> ijs; };
static bool read_cameras(const std::vector<char>& b, std::vector<CamCase>& out) {
    size_t at = 0;
    auto take = [&](void* dst, size_t bytes) { if (at + bytes > b.size()) return false; memcpy(dst, b.data() + at, bytes); at += bytes; return true; };
    while (at < b.size()) {
        CamCase c;
        int32_t ns;
        if (!take(&c.cd, sizeof c.cd) || !take(&c.p, sizeof c.p) || !take(&ns, 4) || ns < 0 || ns > (1 << 20)) return false;
        if (c.cd.from_key_count < 0 || c.cd.at_key_count < 0 || c.cd.from_key_count + c.cd.at_key_count > 512) return false;
        if (c.cd.image_width < 1 || c.cd.image_height < 1) return false;
        c.ijs.resize(3 * (size_t)ns);
        c.keys.resize(c.cd.from_key_count + c.cd.at_key_count);
        if (!take(c.ijs.data(), c.ijs.size() * 4) || !take(c.keys.data(), c.keys.size() * sizeof(CrKeyframe))) return false;
        out.push_back(std::move(c));
    }
    return true;
}
template <typename real, bool ANIM, bool CAMK> __device__ void camera_one(const KernelArgs<real>& A, const uint32_t* ijs, double* o) {
    uint64_t rng = 0;
    V3<real> ro, rd;
    real rtime;
    camera_ray<real, ANIM, CAMK>(A, ijs[0], ijs[1], (int32_t)ijs[2], rng, ro, rd, rtime);
    const uint64_t key = rng_key(A.seed_mixed, ijs[1] * (uint32_t)A.cam.W + ijs[0], ijs[2]);
    o[0] = ro.x; o[1] = ro.y; o[2] = ro.z; o[3] = rd.x; o[4] = rd.y; o[5] = rd.z; o[6] = rtime; o[7] = draws_between(key, rng);
}
// Out: per sample the ANIM kernels' ray, then the CAMK kernels' ray, then (static cameras only) the plain kernels' ray.
template <typename real> __global__ void camera_kernel(KernelArgs<real> A, const uint32_t* ijs, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (ijs[3 * i] >= (uint32_t)A.cam.W || ijs[3 * i + 1] >= (uint32_t)A.cam.H) return;
    camera_one<real, true, false>(A, ijs + 3 * i, out + 24 * i);
    camera_one<real, false, true>(A, ijs + 3 * i, out + 24 * i + 8);
    if (!A.cam.animated) camera_one<real, false, false>(A, ijs + 3 * i, out + 24 * i + 16);
    else for (int k = 16; k < 24; k++) out[24 * i + k] = 0;
}

// ------------------------------------------------------------------ timeline and refit (__host__ __device__)
template <typename real> CR_HD void timeline_one(const Prim<real>* prims, const Key<real>* keys, const double* c, double* o) {
    const Prim<real>& p = prims[(int32_t)c[0]];
    const real t = (real)c[1];
    const Key<real>* k = keys + p.key_first;
    for (int a = 0; a < 9; a++) o[a] = 0;
    if (p.kind() == 0) {   // as shade() and the walk evaluate a keyed sphere
        real g0 = p.g[0], g1 = p.g[1], g2 = p.g[2], g3 = p.g[3];
        timeline_eval(k, p.key_count, t, g0, g1, g2, g3);
        o[0] = g0; o[1] = g1; o[2] = g2; o[3] = g3;
    } else for (int j = 0; j < 3; j++) {
        const V3<real> v = timeline_vertex(k, p.key_count, t, mk<real>(p.g[3 * j], p.g[3 * j + 1], p.g[3 * j + 2]));
        o[3 * j] = v.x; o[3 * j + 1] = v.y; o[3 * j + 2] = v.z;
    }
}
template <typename real> CR_HD void refit_one(const Prim<real>* prims, const Key<real>* keys, const double* c, double* o) {
    const Prim<real>& p = prims[(int32_t)c[0]];
    const bool f64 = sizeof(real) == 8;
    const real ta = (real)(f64 ? c[1] : c[3]), tb = (real)(f64 ? c[2] : c[4]);
    real lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = r_inf(real(0)); hi[a] = -r_inf(real(0)); }
    prim_box_over(p, keys, ta, tb, lo, hi);
    for (int a = 0; a < 3; a++) { o[a] = lo[a]; o[3 + a] = hi[a]; }
}
template <typename real> __global__ void timeline_kernel(const Prim<real>* prims, const Key<real>* keys, const double* in, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) timeline_one(prims, keys, in + 2 * i, out + 9 * i);
}
template <typename real> __global__ void refit_kernel(const Prim<real>* prims, const Key<real>* keys, const double* in, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) refit_one(prims, keys, in + 5 * i, out + 6 * i);
}

static dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// Reads DIR/name.in as rows of `cols` f64 whose first column is a primitive / texture index below `limit`.
static bool read_rows(const std::string& path, size_t cols, int64_t limit, std::vector<double>& rows) {
    std::vector<char> b;
    if (!read_file(path, b) || b.empty()) return false;
    if (b.size() % (cols * 8)) { fprintf(stderr, "%s: bad size\n", path.c_str()); exit(2); }
    rows.resize(b.size() / 8);
    memcpy(rows.data(), b.data(), b.size());
    for (size_t r = 0; r < rows.size() / cols; r++)
        if (!(rows[r * cols] >= 0 && rows[r * cols] < (double)limit)) { fprintf(stderr, "%s: row %zu: bad index\n", path.c_str(), r); exit(2); }
    return true;
}

template <typename real> static void run(const std::string& dir, const SceneIn& s, uint64_t seed, bool host) {
    const char* sfx = sizeof(real) == 8 ? "64" : "32";
    Packed<real> P;
    if (!pack(s, P)) { fprintf(stderr, "too many texels\n"); exit(2); }
    std::vector<double> rows;
    auto put = [&](const char* part, const std::vector<double>& o) {
        if (!write_file(dir + "/" + part + sfx + ".out", o.data(), o.size() * 8)) { fprintf(stderr, "cannot write %s\n", part); exit(2); }
    };
    if (host) {
        if (read_rows(dir + "/timeline.in", 2, (int64_t)P.prims.size(), rows)) {
            std::vector<double> o(rows.size() / 2 * 9);
            for (size_t i = 0; i < rows.size() / 2; i++) timeline_one(P.prims.data(), P.keys.data(), &rows[2 * i], &o[9 * i]);
            put("timeline", o);
        }
        if (read_rows(dir + "/refit.in", 5, (int64_t)P.prims.size(), rows)) {
            std::vector<double> o(rows.size() / 5 * 6);
            for (size_t i = 0; i < rows.size() / 5; i++) refit_one(P.prims.data(), P.keys.data(), &rows[5 * i], &o[6 * i]);
            put("refit", o);
        }
        return;
    }
    DevScene<real> D(s, P, seed);
    auto dev_rows = [&](size_t cols, size_t out_words, auto launch, const char* part) {
        const size_t n = rows.size() / cols;
        double* din = to_dev(rows);
        double* dout = nullptr;
        CHECK(hipMalloc(&dout, n * out_words * 8 + 16));
        launch(din, dout, n);
        CHECK(hipGetLastError());
        put(part, from_dev(dout, n * out_words));
        CHECK(hipFree(din)); CHECK(hipFree(dout));
        printf("%s%s: %zu cases\n", part, sfx, n);
    };
    const int64_t np = (int64_t)P.prims.size();
    if (read_rows(dir + "/timeline.in", 2, np, rows))
        dev_rows(2, 9, [&](double* i, double* o, size_t n) { hipLaunchKernelGGL(timeline_kernel<real>, grid_for(n), dim3(256), 0, 0, D.A.prims, D.A.keys, i, o, n); }, "timeline");
    if (read_rows(dir + "/refit.in", 5, np, rows))
        dev_rows(5, 6, [&](double* i, double* o, size_t n) { hipLaunchKernelGGL(refit_kernel<real>, grid_for(n), dim3(256), 0, 0, D.A.prims, D.A.keys, i, o, n); }, "refit");
    std::vector<char> b;
    std::vector<double> fac(3 * STACK_LEVELS, 1.0);
    if (read_file(dir + "/stack.in", b) && !b.empty()) {
        if (b.size() != fac.size() * 8) { fprintf(stderr, "stack.in: bad size\n"); exit(2); }
        memcpy(fac.data(), b.data(), b.size());
    }
    double* dfac = to_dev(fac);
    if (read_rows(dir + "/hit.in", 12, np, rows)) {
        real* att = nullptr;
        CHECK(hipMalloc(&att, rows.size() / 12 * 3 * sizeof(real) + 16));
        dev_rows(12, HIT_VARIANTS * HIT_WORDS, [&](double* i, double* o, size_t n) { hipLaunchKernelGGL(hit_kernel<real>, grid_for(n), dim3(256), 0, 0, D.A, i, o, att, dfac, n); }, "hit");
        CHECK(hipFree(att));
    }
    if (read_file(dir + "/sky.in", b) && !b.empty()) {
        if (b.size() % 24) { fprintf(stderr, "sky.in: bad size\n"); exit(2); }
        rows.resize(b.size() / 8);
        memcpy(rows.data(), b.data(), b.size());
        if (s.sky_image < 0 || s.sky_image >= (int32_t)s.images.size()) { fprintf(stderr, "sky.in needs a sky image\n"); exit(2); }
        real* att = nullptr;
        CHECK(hipMalloc(&att, rows.size() / 3 * STACK_LEVELS * 3 * sizeof(real) + 16));
        dev_rows(3, 32, [&](double* i, double* o, size_t n) { hipLaunchKernelGGL(sky_kernel<real>, grid_for(n), dim3(256), 0, 0, D.A, i, o, att, dfac, n); }, "sky");
        CHECK(hipFree(att));
    }
    if (read_rows(dir + "/texture.in", 6, (int64_t)s.texs.size(), rows)) {
        for (size_t r = 0; r < rows.size() / 6; r++)
            if (P.remap[(int32_t)rows[6 * r]] < 0) { fprintf(stderr, "texture.in: texture %d is not on the device\n", (int)rows[6 * r]); exit(2); }
        int32_t* remap = to_dev(P.remap);
        dev_rows(6, 4, [&](double* i, double* o, size_t n) { hipLaunchKernelGGL(texture_kernel<real>, grid_for(n), dim3(256), 0, 0, D.A, remap, i, o, n); }, "texture");
        CHECK(hipFree(remap));
    }
    if (read_file(dir + "/camera.in", b) && !b.empty()) {
        std::vector<CamCase> cams;
        if (!read_cameras(b, cams)) { fprintf(stderr, "camera.in: bad records\n"); exit(2); }
        std::vector<double> all;
        for (const CamCase& c : cams) {
            KernelArgs<real> A = D.A;
            pack_camera(&c.cd, A.cam);
            pack_camera_frame(A.cam);
            frame_times(&c.p, A.current_time, A.shutter_length);
            A.seed_mixed = mix64(c.p.seed + RNG_GAMMA);
            std::vector<Key<real>> ck(c.keys.size());
            for (size_t k = 0; k < ck.size(); k++) key_to_real(c.keys[k], ck[k]);
            Key<real>* dk = to_dev(ck);
            A.cam_keys = dk;
            const size_t n = c.ijs.size() / 3;
            uint32_t* dij = to_dev(c.ijs);
            double* dout = nullptr;
            CHECK(hipMalloc(&dout, n * 24 * 8 + 16));
            CHECK(hipMemset(dout, 0, n * 24 * 8));
            hipLaunchKernelGGL(camera_kernel<real>, grid_for(n), dim3(256), 0, 0, A, dij, dout, n);
            CHECK(hipGetLastError());
            const std::vector<double> o = from_dev(dout, n * 24);
            all.insert(all.end(), o.begin(), o.end());
            CHECK(hipFree(dij)); CHECK(hipFree(dout)); CHECK(hipFree(dk));
        }
        put("camera", all);
        printf("camera%s: %zu cameras\n", sfx, cams.size());
    }
    CHECK(hipFree(dfac));
}

int main(int argc, char** argv) {
    if (argc < 2 || argc > 3 || (argc == 3 && strcmp(argv[2], "--host") != 0)) { fprintf(stderr, "usage: shade_check DIR [--host]\n"); return 2; }
    const std::string dir = argv[1];
    const bool host = argc == 3;
    SceneIn s;
    if (!read_scene(dir + "/scene.bin", s)) { fprintf(stderr, "scene.bin: missing or malformed\n"); return 2; }
    uint64_t seed = 0;
    std::vector<char> b;
    if (read_file(dir + "/seed.in", b) && b.size() == 8) memcpy(&seed, b.data(), 8);
    run<double>(dir, s, seed, host);
    run<float>(dir, s, seed, host);
    return 0;
}
