// h-multigrid transfer kernels, float64 instantiations.
#include "lap_htransfer.h"
BDX_HTRANSFER_API(double, f64)
