// Device assembly of the 27-point stencil, float32 instantiation.
#include "lap_stencil27_assemble.h"
BDX_STENCIL27_ASSEMBLE_API(float, f32)
