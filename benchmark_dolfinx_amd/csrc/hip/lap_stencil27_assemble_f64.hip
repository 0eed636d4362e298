// Device assembly of the 27-point stencil, float64 instantiation.
#include "lap_stencil27_assemble.h"
BDX_STENCIL27_ASSEMBLE_API(double, f64)
