// Row-streaming p-multigrid transfer kernels, float32 instantiations.
#include "lap_rowtransfer.h"
BDX_ROWTRANSFER_API(float, f32)
