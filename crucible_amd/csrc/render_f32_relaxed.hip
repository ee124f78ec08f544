// render_f32_relaxed.hip -- the f32 megakernels of relaxed sums (CR_SUM_RELAXED) (render.hpp) and the sums' finalize kernel.
#include "render.hpp"

CR_RENDER_UNIT(float, true)
template int32_t cr::fx_finalize<float>(CrHandle*, const unsigned long long*, float*, size_t, double, double, int32_t);
