// V-cycle tail kernel, float64 instantiation.
#include "pmg_tail.h"
BDX_PMG_TAIL_API(double, f64)
