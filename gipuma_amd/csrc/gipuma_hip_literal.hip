// gipuma_hip_literal.hip -- the reference-order flavour of the library (GIPUMA_HIP_FLAG_LITERAL): gipuma_hip.hip compiled a
// third time with the per-sample arithmetic in the literal operation order of the reference's source (PM_LITERAL = 1, pm_core.h /
// pm_cost.h: view_cost_loop), device code in namespace pm_lit.  Of its host code the exact flavour, which owns the C-ABI, sees
// gipuma_hipl_api() alone (hidden): the table through which it reaches a literal session.
#include <hip/hip_runtime.h>

#define PM_LITERAL 1
#define pm pm_lit
#define GIPUMA_HIP_FLAVOUR_API gipuma_hipl_api
#include "gipuma_hip.hip"
