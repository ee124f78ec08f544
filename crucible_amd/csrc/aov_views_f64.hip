// aov_views_f64.hip -- the f64 guide kernels of several cameras in one launch (aov_kernel.hpp, VIEWS): both tree orders, every residency
#include "aov_kernel.hpp"

template int32_t cr::aov_views_ladder<double>(CrHandle*, cr::AovArgs<double>&, const cr::DevScene<double>&, const cr::WalkChoice&, int*);
