// render_f64_reference.hip -- the f64 megakernels of the reference's summation order (render.hpp).
#include "render.hpp"

CR_RENDER_UNIT(double, false)
