// p-multigrid transfer kernels, float64 instantiations.
#include "lap_transfer.h"
BDX_TRANSFER_API(double, f64)
