// Streaming 27-point stencil kernels, float64 instantiations.
#include "lap_stencil27.h"
BDX_STENCIL27_API(double, f64)
