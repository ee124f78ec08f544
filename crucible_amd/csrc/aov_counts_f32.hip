// aov_counts_f32.hip -- the f32 guide kernels at a count plane (aov_kernel.hpp, COUNTS): both tree orders, every residency
#include "aov_kernel.hpp"

template int32_t cr::aov_counts_ladder<float>(CrHandle*, cr::AovArgs<float>&, const cr::DevScene<float>&, const cr::WalkChoice&, int*);
