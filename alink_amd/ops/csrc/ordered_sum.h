// The ordered sums of the fused fp64 passes — glm.hip, moments.hip, gmm_em.hip, softmax_fused.hip, softmax_csr.hip,
// mlp_fused.hip and newton.hip — gfx950 / MI355X.
//
// Those passes promise the same bits for every grid and every run, with no float atomics.  What keeps the promise
// behind their row kernels is written once, here:
//   chunk merge   part [nchunk, P] -> out [P]: one lane per output element adds its chunk partials in chunk order.
//                 Which element of a partial an output element reads is the caller's Map (the identity, the mirror of
//                 a Gram matrix's lower triangle, or a layout that one file alone knows and keeps).
//   batch sums    part [S, nb] -> out [S]: one workgroup per series; a thread adds every SUM_THREADS-th partial in
//                 ascending order, then a fixed tree over the threads.  A rule of nb alone.
//   wave sums     the two xor butterflies over a wave's 64 lanes.  They are NOT interchangeable (below).
// The fold of a workgroup's four waves in wave order belongs to the tile deal, WaveDeal of gram64_mfma.h.
//
// No contraction: every function here that adds says `#pragma clang fp contract(off)` at the head of its body, which
// covers that body whatever the including file says and reaches no line of the including file (a file-scope pragma
// would hold to the end of gmm_em.hip, which is compiled with the compiler's default).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace osum {

// The sum of v over the wave's 64 lanes, on every lane.  wave_sum_asc adds the xor partners 1, 2, .., 32 and
// wave_sum_desc 32, 16, .., 1: two different orders of the same 63 additions, which round differently and so give
// DIFFERENT BITS.  A call site keeps the order it was written and tested with; taking the other one changes results
// without failing anything but a bit-for-bit comparison.
__device__ __forceinline__ double wave_sum_asc(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_desc(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Maps of the chunk merge: output element e reads element map(e) of every chunk's partial.
struct Identity {
    __device__ int64_t operator()(int64_t e) const { return e; }
};
// [head | dim x dim]: the lower triangle of the matrix behind the `head` leading entries is read from the upper, so
// the merged matrix is exactly symmetric
struct GramMirror {
    int head, dim;
    __device__ int64_t operator()(int64_t e) const {
        if (e < head) return e;
        const int a = (int)((e - head) / dim), b = (int)((e - head) - (int64_t)a * dim);
        return head + (a <= b ? (int64_t)a * dim + b : (int64_t)b * dim + a);
    }
};

constexpr int SUM_THREADS = 1024;       // threads of the batch sums (the default of the template parameter below)

namespace {         // a kernel of its own in every file that includes this header

// out[e] = the sum over c, in chunk order, of part[c P + map(e)]
template <class Map>
__global__ __launch_bounds__(256) void chunk_merge_kernel(Map map, int64_t P, int64_t nchunk,
                                                          const double* __restrict__ part, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= P) return;
    const int64_t src = map(e);
    double s = part[src];
    int64_t c = 1;
    // Eight loads in flight, added in chunk order.  Each load keeps a uniform offset of its own, stepped by 8 P a
    // round, so its address is one add of scalar and src; written as part[(c + u) * P + src] with P an argument the
    // eight addresses compile to a chain of dependent adds, which a merge of many chunks pays once a round.
    int64_t off[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) off[u] = (1 + u) * P;
    for (; c + 8 <= nchunk; c += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            t[u] = part[off[u] + src];
            off[u] += 8 * P;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; c < nchunk; ++c) s += part[c * P + src];
    out[e] = s;
}

// host side: its launch on stream st
template <class Map>
inline void chunk_merge(Map map, int64_t P, int64_t nchunk, const double* part, double* out, hipStream_t st) {
    hipLaunchKernelGGL(chunk_merge_kernel<Map>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, map, P, nchunk,
                       part, out);
}

// out[blockIdx.x] = the sum of the nb partials of series blockIdx.x: a thread adds p[i], p[i + SUM_THREADS], .. in
// ascending order (eight loads in flight), then the fixed tree over the threads.  A template, so that a file that
// never launches it carries no copy.
template <int THREADS = SUM_THREADS>
__global__ __launch_bounds__(THREADS) void batch_sums_kernel(const double* __restrict__ part, int64_t nb,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sh[THREADS];
    const double* __restrict__ p = part + (int64_t)blockIdx.x * nb;
    double a = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 7 * THREADS < nb; i += 8 * THREADS) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[i + u * THREADS];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += t[u];
    }
    for (; i < nb; i += THREADS) a += p[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// host side: the sums of `series` series, part [series, nb] -> out [series] (a template for the same reason)
template <int THREADS = SUM_THREADS>
inline void batch_sums(const double* part, int64_t nb, int series, double* out, hipStream_t st) {
    hipLaunchKernelGGL(batch_sums_kernel<THREADS>, dim3((unsigned)series), dim3(THREADS), 0, st, part, nb, out);
}

}  // namespace

}  // namespace osum
