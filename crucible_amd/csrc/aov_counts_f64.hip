// aov_counts_f64.hip -- the f64 guide kernels at a count plane (aov_kernel.hpp, COUNTS): both tree orders, every residency
#include "aov_kernel.hpp"

template int32_t cr::aov_counts_ladder<double>(CrHandle*, cr::AovArgs<double>&, const cr::DevScene<double>&, const cr::WalkChoice&, int*);
