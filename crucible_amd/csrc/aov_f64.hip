// aov_f64.hip -- the f64 guide kernels (aov_kernel.hpp): both tree orders, every residency, the f32 screen where a render uses it
#include "aov_kernel.hpp"

template int32_t cr::aov_ladder<double>(CrHandle*, cr::AovArgs<double>&, const cr::DevScene<double>&, const cr::WalkChoice&, int*);
