// The fp64 MFMA tile loop shared by the dense fp64 kernels — kmeans_dense64.hip (nearest), evalcluster.hip (dense row
// pass), sos.hip (search, products) and, in part, gmm_em.hip (E pass) — gfx950 / MI355X.
//
// The problem they share: fp64 rows X [n, d] (any d, zero-padded in registers) against a table of fp64 "tile rows"
// T [kk, d] (centroids, cluster means, the streamed rows of SOS, the columns of GMM's W_j), all dots x_r . t_c on
// v_mfma_f64_16x16x4_f64 with no [n, kk] buffer.  A workgroup of WAVES = 4 waves owns ROWS = 64 data rows, a wave
// its 16, one per lane column m = lane & 15; the lane group g = lane >> 4 splits the dims.  The kernel walks the
// table in blocks of 16 NT tile rows (NT = 1, 2, 4 or 8 tiles of 16) and the dims in chunks of DCH = 32 (two
// 16-dim groups u = 0, 1), staging one (block, chunk) of the table in LDS at a time.
//
// MFMA operand and result maps (one v_mfma_f64_16x16x4_f64 = one step s of one 16-dim group u, k = 4):
//   A  the table tile:  row (tile row) = lane & 15 = m,  k = lane >> 4 = g;
//   B  the data rows:   k = lane >> 4 = g,               column (data row) = lane & 15 = m;
//   D  the four result slots q = 0..3 of a lane: tile row g + 4 q of the tile, data row m.
//   A lane therefore holds, for its own data row, the table rows (blk * NT + t) * 16 + g + 4 q; an epilogue runs down
//   the lane's own 4 NT registers first (ascending t, then q) and across the four lane groups of the row last
//   (group_sum, or the kernel's own xor-16 / xor-32 merge).
//   The k order inside a 16-dim group is permuted the same way on both operands: lane group g owns the dims
//   4 g .. 4 g + 3 and step s multiplies dim 4 g + s.  A lane's four dims of X are then 32 contiguous bytes
//   (load_chunk), and the sum over k does not care about the order the products enter it as long as A and B agree.
//
// The image (``ops/kmeans_dense64.centroid_image``): the table zero-padded to whole blocks and whole chunks and
// written in exactly the order the lanes read it,
//     img [blk][dch][u = 2][tile = NT][g = 4][m = 16][step = 4],
//     element = T[(blk * NT + tile) * 16 + m, dch * 32 + 16 u + 4 g + step]   (0 outside T),
// so one (block, chunk) is NT * 512 contiguous doubles, `stage` is a straight copy, and `mfma_group` reads
// 32 bytes per lane at cent + (((u * NT + tile) * 4 + g) * 16 + m) * 4 — consecutive lanes 32 bytes apart, a
// conflict-free ds_read_b128 pair.  That index expression (mfma_group) and the permute of ``centroid_image`` are the
// two ends of the contract; tests/test_kmeans_dense64.py pins the Python end element by element.
// gmm_em.hip keeps a layout of its own on purpose: [tile][dch][u][g][m][step] (tile outermost, all dim chunks of a
// tile together), staged per group of tiles for the whole d, because it holds a row's d <= 128 dims in registers
// and walks tiles, not chunks.  It shares the maps above, load_chunk, mf64 and group_sum, not stage / mfma_group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d64 {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int WAVES = 4;             // waves per workgroup; a wave owns 16 rows of the workgroup's 64
constexpr int ROWS = 16 * WAVES;
constexpr int DCH = 32;              // dims per staged chunk (two 16-dim groups u = 0, 1)

__device__ __forceinline__ d4_t mf64(double a, double b, d4_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the four lanes (lane & 15 fixed) that share a data row: both partners add the same two values at each step, so
// every one of them ends with the same bits
__device__ __forceinline__ double group_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// The four dims j0 .. j0 + 3 of one row, zero outside [0, d) or when the row is not `ok`; no address is formed that
// is not loaded.  VEC: d is even and xr is 16-byte aligned, so the four dims are two aligned 16-byte loads (a pair
// never straddles d); otherwise four scalar loads.  Returned by value, not through a reference, so that the scalar
// guards stay flat selects (profiles/dense64_shared_loop.txt).
template <bool VEC>
__device__ __forceinline__ d4_t load_group(const double* __restrict__ xr, bool ok, int j0, int d) {
    d4_t r;
    if (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            d2_t v = {0.0, 0.0};
            if (ok && j0 + 2 * h < d) v = *reinterpret_cast<const d2_t*>(xr + j0 + 2 * h);
            r[2 * h] = v[0];
            r[2 * h + 1] = v[1];
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) r[s] = (ok && j0 + s < d) ? xr[j0 + s] : 0.0;
    }
    return r;
}

// Row-chunk load: xb[u][s] = xr[dc * 32 + 16 u + 4 g + s] for the lane group g, by the rules of load_group.
template <bool VEC>
__device__ __forceinline__ void load_chunk(double (&xb)[2][4], const double* __restrict__ xr, bool ok, int dc, int g,
                                           int d) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const d4_t v = load_group<VEC>(xr, ok, dc * DCH + 16 * u + 4 * g, d);
#pragma unroll
        for (int s = 0; s < 4; ++s) xb[u][s] = v[s];
    }
}

// Stage the image's (block cb, dim chunk dc) in LDS: a straight copy of NT * 4 KiB, 16 bytes per thread and round.
// Every thread of the 256-thread workgroup must call it (two barriers).
template <int NT>
__device__ __forceinline__ void stage(double* __restrict__ cent, const double* __restrict__ img, int cb, int ndch,
                                      int dc) {
    const int tid = threadIdx.x;
    const d2_t* __restrict__ src = reinterpret_cast<const d2_t*>(img + ((int64_t)cb * ndch + dc) * (NT * 512));
    __syncthreads();        // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < NT; ++i) reinterpret_cast<d2_t*>(cent)[i * 256 + tid] = src[i * 256 + tid];
    __syncthreads();
}

// The MFMAs of one 16-dim group u of the staged chunk: acc[t] += tile t . xu, the ds_read_b128 of up to four tiles
// first, then the four steps interleaved over those tiles.
template <int NT>
__device__ __forceinline__ void mfma_group(d4_t (&acc)[NT], const double* __restrict__ cent, const double (&xu)[4],
                                           int u, int g, int m) {
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += 4) {
        d4_t a[NT < 4 ? NT : 4];
#pragma unroll
        for (int t = 0; t < (NT < 4 ? NT : 4); ++t)
            a[t] = *reinterpret_cast<const d4_t*>(cent + (((u * NT + t0 + t) * 4 + g) * 16 + m) * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int t = 0; t < (NT < 4 ? NT : 4); ++t) acc[t0 + t] = mf64(a[t][s], xu[s], acc[t0 + t]);
        }
    }
}

// ---- host side of the extern "C" wrappers ----

inline bool nt_ok(int nt) { return nt == 1 || nt == 2 || nt == 4 || nt == 8; }

// the VEC rule: even d and every row table 16-byte aligned
inline bool vec_ok(int d, const void* p) { return d % 2 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// workgroups that stride over ceil(rows / 64) row batches: at most `grid` of them, or `dflt` when grid <= 0
// (dflt 0: as many as batches)
inline unsigned row_blocks(int64_t rows, int grid, int64_t dflt) {
    int64_t blocks = (rows + ROWS - 1) / ROWS;
    const int64_t cap = grid > 0 ? grid : dflt;
    if (cap > 0 && blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

}  // namespace d64

// The one launch of the extern "C" wrappers: KERNEL<P, VEC> with 256-thread workgroups, P = the one of the four
// compile-time values P0..P3 that the run-time p equals (the caller has checked that it is one of them; nt takes
// 1, 2, 4, 8, the GMM E pass its dim chunks 1, 2, 3, 4), VEC = vec.
#define ALINK_D64_LAUNCH_VEC(KERNEL, P, vec, blocks, st, ...)                                                      \
    do {                                                                                                           \
        if (vec)                                                                                                   \
            hipLaunchKernelGGL((KERNEL<P, true>), dim3(blocks), dim3(64 * d64::WAVES), 0, st, __VA_ARGS__);       \
        else                                                                                                       \
            hipLaunchKernelGGL((KERNEL<P, false>), dim3(blocks), dim3(64 * d64::WAVES), 0, st, __VA_ARGS__);      \
    } while (0)
#define ALINK_D64_LAUNCH(KERNEL, p, P0, P1, P2, P3, vec, blocks, st, ...)                                          \
    do {                                                                                                           \
        if ((p) == P0) ALINK_D64_LAUNCH_VEC(KERNEL, P0, vec, blocks, st, __VA_ARGS__);                            \
        else if ((p) == P1) ALINK_D64_LAUNCH_VEC(KERNEL, P1, vec, blocks, st, __VA_ARGS__);                       \
        else if ((p) == P2) ALINK_D64_LAUNCH_VEC(KERNEL, P2, vec, blocks, st, __VA_ARGS__);                       \
        else ALINK_D64_LAUNCH_VEC(KERNEL, P3, vec, blocks, st, __VA_ARGS__);                                      \
    } while (0)
