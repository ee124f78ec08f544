// render_views_f64.hip -- the f64 megakernels of several cameras in one launch, cr_render_views_* (render_views.hpp)
#include "render_views.hpp"

CR_RENDER_VIEWS_UNIT(double)
