// Wave-uniform broadcasts of a 64-bit value from one lane (two v_readlane) — gfx950 / MI355X.  Used by the kernels
// that walk 64 loaded entries one at a time: the CSR row kernels of kmeans_sparse.hip and evalcluster.hip, and the
// dense accumulate kernel of kmeans_dense64.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lane {

__device__ __forceinline__ double bcast_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int64_t bcast_i64(int64_t v, int lane) {
    const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(v >> 32), lane);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

}  // namespace lane
