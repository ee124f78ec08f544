// aov_f32.hip -- the f32 guide kernels (aov_kernel.hpp): both tree orders, every residency
#include "aov_kernel.hpp"

template int32_t cr::aov_ladder<float>(CrHandle*, cr::AovArgs<float>&, const cr::DevScene<float>&, const cr::WalkChoice&, int*);
