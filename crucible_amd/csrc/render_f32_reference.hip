// render_f32_reference.hip -- the f32 megakernels of the reference's summation order (render.hpp).
#include "render.hpp"

CR_RENDER_UNIT(float, false)
