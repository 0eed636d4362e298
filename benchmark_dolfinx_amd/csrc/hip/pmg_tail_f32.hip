// V-cycle tail kernel, float32 instantiation.
#include "pmg_tail.h"
BDX_PMG_TAIL_API(float, f32)
