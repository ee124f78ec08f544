// aov_views_f32.hip -- the f32 guide kernels of several cameras in one launch (aov_kernel.hpp, VIEWS): both tree orders, every residency
#include "aov_kernel.hpp"

template int32_t cr::aov_views_ladder<float>(CrHandle*, cr::AovArgs<float>&, const cr::DevScene<float>&, const cr::WalkChoice&, int*);
