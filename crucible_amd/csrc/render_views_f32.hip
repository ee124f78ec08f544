// render_views_f32.hip -- the f32 megakernels of several cameras in one launch, cr_render_views_* (render_views.hpp)
#include "render_views.hpp"

CR_RENDER_VIEWS_UNIT(float)
