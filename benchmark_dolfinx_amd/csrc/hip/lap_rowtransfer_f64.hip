// Row-streaming p-multigrid transfer kernels, float64 instantiations.
#include "lap_rowtransfer.h"
BDX_ROWTRANSFER_API(double, f64)
