// h-multigrid transfer kernels, float32 instantiations.
#include "lap_htransfer.h"
BDX_HTRANSFER_API(float, f32)
