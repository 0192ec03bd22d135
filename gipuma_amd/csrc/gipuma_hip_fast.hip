// gipuma_hip_fast.hip -- the tolerance-judged flavour of the library (GIPUMA_HIP_FLAG_FAST): gipuma_hip.hip compiled a second
// time with the approx arithmetic of pm_core.h (PM_APPROX = 1), device code in namespace pm_fast.  Of its host code the exact
// flavour, which owns the C-ABI, sees gipuma_hipf_api() alone (hidden): the table through which it reaches a fast session.
#include <hip/hip_runtime.h>

#define PM_APPROX 1
#define pm pm_fast
#define GIPUMA_HIP_FLAVOUR_API gipuma_hipf_api
#include "gipuma_hip.hip"
