// Cross-lane helpers of a wave — gfx950 / MI355X.
// * bcast_f64 / bcast_i64: the wave-uniform broadcast of a 64-bit value from one lane (two v_readlane).  Used by the
//   kernels that walk 64 loaded entries one at a time: the CSR row walk of csr_rows.h, the CSC accumulate kernel of
//   kmeans_sparse.hip and the dense accumulate kernel of kmeans_dense64.hip.
// * group_sum<G> / group_sum_int<G>: the xor butterfly over aligned groups of G lanes.  Used by the kernels that
//   split a row or a pair over G lanes: bisecting.hip (both descents) and lsh.hip (the pair distances).
//   d64::group_sum (dense64_mfma.h) is another function: the fixed xor-16 / xor-32 sum over a row's four lane groups.
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

// the sum of the G lanes' values (G a power of two, groups aligned to G): both partners of a step add the same two
// values, so every lane of the group ends with the same bits
template <int G>
__device__ __forceinline__ double group_sum(double a) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

template <int G>
__device__ __forceinline__ int group_sum_int(int a) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

}  // namespace lane
