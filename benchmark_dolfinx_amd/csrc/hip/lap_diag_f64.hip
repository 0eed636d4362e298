// Matrix-free operator diagonal, float64 instantiations.
#include "lap_diag.h"
BDX_DIAG_API(double, f64)
