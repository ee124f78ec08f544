// ISA probe for tests/test_quiet_isa.py: the headline kernel of crucible_amd/csrc/pathtrace.hpp on its own, with its work
// counters (pathtrace_kernel<double, RES_LDS, false, false, false, true, true>) or without them (-DQUIET_ISA:
// pathtrace_kernel_quiet<RES_LDS>), so that a device-only compile (-S) shows the screened box loop of either.
#include "pathtrace.hpp"

namespace cr {
#ifdef QUIET_ISA
template __global__ void pathtrace_kernel_quiet<RES_LDS>(const KernelArgs<double>);
#else
template __global__ void pathtrace_kernel<double, RES_LDS, false, false, false, true, true>(const KernelArgs<double>);
#endif
}
