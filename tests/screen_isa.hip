// ISA probe for tests/test_gpu_screen_fma.py: instantiates f64 SCREEN kernels of crucible_amd/csrc/pathtrace.hpp on their
// own, so that a device-only compile (-S) shows the screened box loop without the rest of the library.
// SCREEN_ISA_KERNEL selects the instantiation's template arguments; the default is the headline kernel
// (book1, f64, scene in LDS, relaxed sums): pathtrace_kernel<double, RES_LDS, false, false, false, true, true>.
#include "pathtrace.hpp"

#ifndef SCREEN_ISA_KERNEL
#define SCREEN_ISA_KERNEL double, RES_LDS, false, false, false, true, true
#endif

namespace cr {
template __global__ void pathtrace_kernel<SCREEN_ISA_KERNEL>(const KernelArgs<double>);
}
