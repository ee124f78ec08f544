// render_f64_relaxed.hip -- the f64 megakernels of relaxed sums (CR_SUM_RELAXED) (render.hpp) and the sums' finalize kernel.
#include "render.hpp"

CR_RENDER_UNIT(double, true)
template int32_t cr::fx_finalize<double>(CrHandle*, const unsigned long long*, double*, size_t, double, double, int32_t);
