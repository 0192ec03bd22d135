// pm_hash.h -- mix32, the 32-bit integer hash behind the solver's counter-based random numbers (pm_core.h, M4) and the
// hashed visiting order of the cloud thinning (gipuma_cloud.hip, whose host code needs it too).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pm {

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x7feb352dU;
    h ^= h >> 15;
    h *= 0x846ca68bU;
    h ^= h >> 16;
    return h;
}

}  // namespace pm
