// The wave-per-row walk of CSR rows against a dense table, shared by the CSR row kernels — kmeans_sparse.hip (nearest
// centroid) and evalcluster.hip (CSR row pass) — gfx950 / MI355X.  bisecting.hip (CSR descent) takes the host side
// only: its kernel walks a row's entries lane-strided against one plane, which is not this walk.
//
// The problem they share: CSR rows (crow int64 [n+1]; col int32 / int64; val fp64) under d columns against a table of
// k fp64 vectors (centroids, cluster means), all dots x_r . t_c in fp64 with no [n, k] buffer and no dense row.  The
// table comes transposed and padded, T [d, kp] with kp a multiple of 64 (``ops/csr.py``: kp, padded_transpose), so a
// stored entry (j, v) reads the contiguous kp-double row T[j, :].
//
// Lane / cluster map: one wave owns a row (WAVES = 4 rows per 256-thread workgroup, the waves stride over the rows).
// The kernel walks the table in cluster blocks of 64 NB columns starting at cb = 0, 64 NB, ...; lane l holds the
// clusters cb + l + 64 b, b = 0 .. NB - 1, in registers (NB = 1, 2 or NBMAX = 4: up to 256 clusters per pass over the
// row).  row_dots loads the row's entries 64 at a time, entry p + l on lane l (coalesced), and walks a batch in
// stored order with wave-uniform broadcasts, U entries at a time in two phases: every broadcast and the U NB gathers
// T[c, cb + l + 64 b] are issued first, then the U NB FMAs run in ascending u, then b.  So every lane adds a row's
// entries in stored order, and a row's sums do not depend on the grid or on the row's wave.
//
// Guard rule: an entry whose column is outside [0, d), and a lane past the end of the row, becomes (column 0,
// value 0.0) before any address is formed (load_entry): it reads row 0 of T and adds nothing, to the dots and to
// |x|^2 alike.  kp >= 64 NB unless NB == NBMAX, where a block may end past kp: `NB < NBMAX || cb + 64 b < kp` guards its
// tail, in the gathers here and in the caller's epilogue.
//
// Values travel by value (entry_t, dots_t), never through references to the caller's arrays, so that the guards stay
// flat selects (profiles/dense64_shared_loop.txt, profiles/csr_shared_walk.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "lane_bcast.h"

namespace csr {

constexpr int WAVES = 4;             // waves (rows / work items) per 256-thread workgroup
constexpr int NBMAX = 4;             // cluster blocks of 64 a lane holds at most (256 clusters per pass)
constexpr int64_t WAVE_GRID = 16384; // workgroups of a wave-per-item launch at most, unless the caller sets a grid

// this wave's first item and the items between two of its turns
__device__ __forceinline__ int64_t first_item() {
    return (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}
__device__ __forceinline__ int64_t item_stride() { return (int64_t)gridDim.x * WAVES; }

struct entry_t { int64_t c; double v; };

// The guarded entry of this lane in the batch of m <= 64 entries that starts at p: (col, val)[p + lane], or (0, 0.0)
// for an out-of-range column and for a lane past the row.
template <typename I>
__device__ __forceinline__ entry_t load_entry(const I* __restrict__ col, const double* __restrict__ val, int64_t p,
                                              int m, int lane, int64_t d) {
    entry_t e = {0, 0.0};
    if (lane < m) {
        const int64_t c = (int64_t)col[p + lane];
        if (c >= 0 && c < d) {
            e.c = c;
            e.v = val[p + lane];
        }
    }
    return e;
}

// The per-entry hook of row_dots, for a kernel that needs one more wave-uniform value of the entry's table row:
// `gather(row)` runs in the gather phase (row = T + c * kp) and its value comes back, with the entry's value v, to
// `fold(v, g)` in the FMA phase, after the entry's |x|^2 term and before its dots.  This default does nothing.
struct no_hook {
    __device__ __forceinline__ double gather(const double* __restrict__) const { return 0.0; }
    __device__ __forceinline__ void fold(double, double) {}
};

// a row against one cluster block: the lane's NB dots, |x|^2 of the row, and the hook after its folds
template <int NB, typename H>
struct dots_t {
    double acc[NB];
    double xn;
    H hook;
};

// The walk of the entries [s, e) of one row against the cluster block at cb of T [d, kp]: acc[b] = x . T[:, cb +
// lane + 64 b] (0 where the tail guard fails) and xn = |x|^2, both by fma in stored order from 0.
template <int NB, int U, int NBMAX, typename I, typename H = no_hook>
__device__ __forceinline__ dots_t<NB, H> row_dots(const I* __restrict__ col, const double* __restrict__ val,
                                                   int64_t s, int64_t e, int64_t d, const double* __restrict__ T,
                                                   int kp, int cb, int lane, H hook = H()) {
    dots_t<NB, H> r = {};
    for (int64_t p = s; p < e; p += 64) {
        const int m = (int)((e - p) < 64 ? (e - p) : 64);
        const entry_t mine = load_entry(col, val, p, m, lane, d);
        for (int j0 = 0; j0 < m; j0 += U) {
            double v[U];
            double g[U];
            double t[U][NB];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // lanes j0 + u >= m hold (0, 0.0): they read row 0 of T and add nothing
                const int j = (j0 + u) & 63;
                const int64_t c = lane::bcast_i64(mine.c, j);
                v[u] = lane::bcast_f64(mine.v, j);
                const double* __restrict__ rowp = T + c * (int64_t)kp;
                g[u] = hook.gather(rowp);
                // Where a hook reads the row too, the lane's first cluster stays in the index; without one it goes
                // into the pointer.  The same addresses: the form decides whether the compiler keeps the row as a
                // scalar base, and these two keep each kernel's registers (profiles/csr_shared_walk.txt, section A).
                constexpr bool hooked = !std::is_empty<H>::value;
                const double* __restrict__ colp = hooked ? rowp : rowp + cb + lane;
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    t[u][b] = (NB < NBMAX || cb + 64 * b < kp) ? colp[(hooked ? cb + lane : 0) + 64 * b] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                r.xn = fma(v[u], v[u], r.xn);
                hook.fold(v[u], g[u]);
#pragma unroll
                for (int b = 0; b < NB; ++b) r.acc[b] = fma(v[u], t[u][b], r.acc[b]);
            }
        }
    }
    r.hook = hook;
    return r;
}

// ---- host side of the extern "C" wrappers ----

// workgroups of `waves` waves that stride over the items, a wave per item: at most `grid` of them, or `dflt` when
// grid <= 0
inline unsigned wave_blocks(int64_t items, int grid, int waves, int64_t dflt) {
    const int64_t blocks = (items + waves - 1) / waves, cap = grid > 0 ? grid : dflt;
    return (unsigned)(blocks > cap ? cap : blocks);
}

}  // namespace csr

// The launches of the extern "C" wrappers over CSR rows, 256-thread workgroups, the kernel's arguments starting
// (crow, col, ...).  ALINK_CSR_LAUNCH: KERNEL<NB, U, I> with (NB, U) from kp — one or two whole blocks with 8 entries'
// gathers in flight, else NBMAX blocks per pass with 4 — and I from idx64.  Its column-type half alone, for a kernel
// without (NB, U), is ALINK_CSR_LAUNCH_IDX: K64 / K32 are the kernel's int64_t / int32_t column instantiations (each
// in parentheses); idx64 picks one and types col for it.
#define ALINK_CSR_LAUNCH_IDX(K64, K32, idx64, blocks, st, crow, col, ...)                                          \
    do {                                                                                                           \
        if (idx64)                                                                                                 \
            hipLaunchKernelGGL(K64, dim3(blocks), dim3(64 * csr::WAVES), 0, st, crow,                              \
                               reinterpret_cast<const int64_t*>(col), __VA_ARGS__);                                \
        else                                                                                                       \
            hipLaunchKernelGGL(K32, dim3(blocks), dim3(64 * csr::WAVES), 0, st, crow,                              \
                               reinterpret_cast<const int32_t*>(col), __VA_ARGS__);                                \
    } while (0)
#define ALINK_CSR_LAUNCH(KERNEL, kp, ...)                                                                          \
    do {                                                                                                           \
        if ((kp) == 64)                                                                                            \
            ALINK_CSR_LAUNCH_IDX((KERNEL<1, 8, int64_t>), (KERNEL<1, 8, int32_t>), __VA_ARGS__);                   \
        else if ((kp) == 128)                                                                                      \
            ALINK_CSR_LAUNCH_IDX((KERNEL<2, 8, int64_t>), (KERNEL<2, 8, int32_t>), __VA_ARGS__);                   \
        else                                                                                                       \
            ALINK_CSR_LAUNCH_IDX((KERNEL<csr::NBMAX, 4, int64_t>), (KERNEL<csr::NBMAX, 4, int32_t>), __VA_ARGS__); \
    } while (0)
