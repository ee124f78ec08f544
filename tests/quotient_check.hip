// Device check for tests/test_gpu_quotient.py: sphere_quot<true>(n, a, shared_rcp(a)) of crucible_amd/csrc/pathtrace.hpp -- Sphere::hit's
// quotient with the reciprocal of a made once -- against n / a, on pairs the test writes.  Consecutive groups of 64 pairs are one
// wave (blocks of 256 threads, one pair per thread), so the test decides which pairs share the helper's wave-uniform guard.
// Built with the diagnostic counters (CR_DIAG): the helper counts, per lane, the quotients it made and those it divided, and
// that is the path this program reports -- what ran, not what the operands imply.
//
// usage: quotient_check DIR
//   DIR/quot.in  n x 2 f64: numerator, divisor   -> DIR/quot.out  n x QuotOut
// Exit code 0 when it ran; 2 on an I/O or HIP error.
#define CR_DIAG 1
#include "pathtrace.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace cr;

struct QuotOut {
    double q, ref;       // the helper's quotient and n / a
    uint32_t path;       // Q_SHORT or Q_DIVIDED
    uint32_t pad;
};
enum : uint32_t { Q_SHORT = 1, Q_DIVIDED = 2 };

__global__ void quot_kernel(const double* in, QuotOut* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;   // (the test sends whole waves: no wave is partly active)
    const double num = in[2 * i], a = in[2 * i + 1];
    Diag dg;
    for (int k = 0; k < DG_N; k++) dg.v[k] = 0;
    QuotOut o;
    o.q = sphere_quot<true>(num, a, shared_rcp(a), &dg);
    o.ref = num / a;
    o.path = dg.v[DG_QUOT_LANE] != 1u ? 0u : (dg.v[DG_QUOTDIV_LANE] ? Q_DIVIDED : Q_SHORT);
    o.pad = 0;
    out[i] = o;
}

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: quotient_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    FILE* f = fopen((dir + "/quot.in").c_str(), "rb");
    if (!f) { fprintf(stderr, "quot.in: cannot open\n"); return 2; }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (len <= 0 || len % (64 * 2 * 8)) { fprintf(stderr, "quot.in: bad size (whole waves of 64 pairs)\n"); fclose(f); return 2; }
    std::vector<char> in((size_t)len);
    const size_t got = fread(in.data(), 1, in.size(), f);
    fclose(f);
    if (got != in.size()) return 2;
    const size_t n = in.size() / (2 * 8);
    void *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, in.size()));
    CHECK(hipMalloc(&dout, n * sizeof(QuotOut)));
    CHECK(hipMemcpy(din, in.data(), in.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(quot_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double*)din, (QuotOut*)dout, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<QuotOut> out(n);
    CHECK(hipMemcpy(out.data(), dout, n * sizeof(QuotOut), hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    FILE* g = fopen((dir + "/quot.out").c_str(), "wb");
    if (!g) return 2;
    const size_t put = fwrite(out.data(), sizeof(QuotOut), n, g);
    if (fclose(g) != 0 || put != n) return 2;
    printf("quotient: %zu pairs\n", n);
    return 0;
}
