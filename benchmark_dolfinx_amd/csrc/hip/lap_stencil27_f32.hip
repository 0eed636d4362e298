// Streaming 27-point stencil kernels, float32 instantiations.
#include "lap_stencil27.h"
BDX_STENCIL27_API(float, f32)
