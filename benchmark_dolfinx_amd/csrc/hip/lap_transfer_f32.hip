// p-multigrid transfer kernels, float32 instantiations.
#include "lap_transfer.h"
BDX_TRANSFER_API(float, f32)
