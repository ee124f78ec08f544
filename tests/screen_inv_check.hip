// Device check for tests/test_gpu_screen_inv.py: the screen's f32 1/direction as walk_begin_screened makes it
// (crucible_amd/csrc/pathtrace.hpp: screen_rcp1, screen_inv, screen_in_range_lazy) beside the one walk_begin's division gives.
//
// usage: screen_inv_check DIR
//   DIR/inv.in  n f64: direction components   -> DIR/inv.out  n x InvOut
// Exit code 0 when it ran; 2 on an I/O or HIP error.
#include "pathtrace.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace cr;

struct InvOut {
    double r1;           // v_rcp_f64 and one Newton step
    float if_new;        // (float)r1: walk_begin_screened's
    float if_old;        // (float)(1.0 / d): walk_begin's, as walk_round converts it
    uint32_t in_range;   // screen_in_range_lazy with the value on all three axes and the origin at 0
    uint32_t pad;
};

__global__ void inv_kernel(const double* in, InvOut* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = in[i];
    InvOut o;
    o.r1 = screen_rcp1(d);
    o.if_new = screen_inv(d);
    o.if_old = (float)(1.0 / d);
    o.in_range = screen_in_range_lazy(0.0f, o.if_new, o.if_new, o.if_new) ? 1u : 0u;
    o.pad = 0;
    out[i] = o;
}

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: screen_inv_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    FILE* f = fopen((dir + "/inv.in").c_str(), "rb");
    if (!f) { fprintf(stderr, "inv.in: cannot open\n"); return 2; }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (len <= 0 || len % 8) { fprintf(stderr, "inv.in: bad size\n"); fclose(f); return 2; }
    std::vector<char> in((size_t)len);
    const size_t got = fread(in.data(), 1, in.size(), f);
    fclose(f);
    if (got != in.size()) return 2;
    const size_t n = in.size() / 8;
    void *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, in.size()));
    CHECK(hipMalloc(&dout, n * sizeof(InvOut)));
    CHECK(hipMemcpy(din, in.data(), in.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(inv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double*)din, (InvOut*)dout, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<InvOut> out(n);
    CHECK(hipMemcpy(out.data(), dout, n * sizeof(InvOut), hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    FILE* g = fopen((dir + "/inv.out").c_str(), "wb");
    if (!g) return 2;
    const size_t put = fwrite(out.data(), sizeof(InvOut), n, g);
    if (fclose(g) != 0 || put != n) return 2;
    printf("screen_inv: %zu values\n", n);
    return 0;
}
