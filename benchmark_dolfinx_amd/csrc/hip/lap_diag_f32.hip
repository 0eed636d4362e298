// Matrix-free operator diagonal, float32 instantiations.
#include "lap_diag.h"
BDX_DIAG_API(float, f32)
