// Bisecting k-means (``ops/bisecting.py``): every row is compared with the split plane of its own tree node.
//
// The tree table (built on the host, shared by training and prediction): nodes are slots 0 .. S - 1, left / right
// [S] int32 are the children's slots (-1: do not descend here), and the slots that descend hold a plane:
//   EUCLIDEAN  P0 = V [., d] = r - l, thr [.] = (r + l)/2 . (r - l): a row goes left iff x . V[s] < thr[s];
//   COSINE     P0 = A [., d] = l/|l|, P1 = B [., d] = r/|r|: left iff (1 - x . A[s]) < (1 - x . B[s]) on rows the
//              caller normalised (two dots, as the host code compares them; never folded into one).
// Equality and any NaN compare false and go right.
//
// * alink_bisect_descend_f64 — fp64 rows [n, d], 1 <= d <= 1024; slot [n] int32 is read and written in place.
//   Per row: s = slot[i]; while levels remain, 0 <= s < S and left[s] >= 0: evaluate the plane, step to the child.
//   A streaming dot product: G lanes per row, G a power of two chosen from d alone (lanes_for): a lane owns the
//   pairs g, g + G, ... of its row (elements 2 q, 2 q + 1), up to 8 of them, so one load instruction of a group
//   covers a contiguous segment of the row: 16-byte loads where d is even and the bases are 16-byte aligned, 8-byte
//   loads otherwise.  Rows of up to 4 pairs take one pair per lane; longer rows keep 4 lanes (64-byte segments) until
//   8 pairs per lane no longer cover them: measured on the MI355X, the butterfly and the per-row bookkeeping, not the
//   loads, bound the kernel when every lane holds a single pair (1.49 ms against 0.74 ms at 4e6 x 128, load floor
//   0.67 ms), and segments of 32, 64 and 128 bytes load equally fast.
//   A lane adds its elements in ascending j by fma, then a fixed xor butterfly (offsets 1, 2, .., G / 2) adds the
//   G partial sums: the order depends on d alone, never on the grid, the row's position or the load width, so a
//   row gets the same side in every launch.  The row stays in registers across the levels (16 doubles per lane at
//   d = 1024); a row whose slot does not descend is not read.  The planes come from the table through L2.
// * alink_bisect_descend_csr — the same for CSR rows (crow int64, col int32 / int64, val fp64) that are never
//   densified: one wave per row, lane l takes the entries l, l + 64, ... in ascending order, the same butterfly
//   (lane_bcast.h: group_sum).  Entries whose column is outside [0, d) are skipped.  The grid and the column-type
//   dispatch are those of the CSR row kernels (csr_rows.h, host side).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_rows.h"

namespace {

using lane::group_sum;

typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int BD_THREADS = 256;
#ifndef BD_PAIRS_IN_FLIGHT
#define BD_PAIRS_IN_FLIGHT 4
#endif
constexpr int BD_FLIGHT = BD_PAIRS_IN_FLIGHT;   // 16-byte loads of X a lane has in flight: R rows of NP pairs each

// the lane's NP pairs of the d-vector at p (pairs g, g + G, ...); elements at or past d are zero and not loaded
template <int G, int NP, bool VEC>
__device__ __forceinline__ void load_pairs(const double* __restrict__ p, int d, int g, double (&x)[2 * NP]) {
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int j0 = 2 * (g + G * q);
        if (VEC) {
            d2_t v = {0.0, 0.0};
            if (j0 < d) v = *reinterpret_cast<const d2_t*>(p + j0);
            x[2 * q] = v[0];
            x[2 * q + 1] = v[1];
        } else {
            x[2 * q] = j0 < d ? p[j0] : 0.0;
            x[2 * q + 1] = j0 + 1 < d ? p[j0 + 1] : 0.0;
        }
    }
}

// G lanes per row, NP pairs per lane (2 G NP >= d), R rows per group in flight.
template <int G, int NP, int R, bool VEC>
__global__ __launch_bounds__(BD_THREADS) void bisect_descend_f64_kernel(
        const double* __restrict__ X, int64_t n, int d, int* __restrict__ slot, int S,
        const int* __restrict__ left, const int* __restrict__ right, const double* __restrict__ P0,
        const double* __restrict__ P1, const double* __restrict__ thr, int cosine, int levels) {
    constexpr int RPB = BD_THREADS / G;         // rows of one pass of the workgroup
    const int g = threadIdx.x & (G - 1);
    const int rloc = threadIdx.x / G;
    const int64_t npass = (n + (int64_t)RPB * R - 1) / ((int64_t)RPB * R);
    for (int64_t b = blockIdx.x; b < npass; b += gridDim.x) {
        int64_t row[R];
        int s[R], s0[R], l[R];
        bool act[R];
        double x[R][2 * NP];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            row[r] = (b * R + r) * RPB + rloc;
            s[r] = row[r] < n ? slot[row[r]] : -1;
            s0[r] = s[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            l[r] = (s[r] >= 0 && s[r] < S) ? left[s[r]] : -1;
            act[r] = l[r] >= 0 && levels > 0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (act[r]) {
                load_pairs<G, NP, VEC>(X + row[r] * (int64_t)d, d, g, x[r]);
            } else {
#pragma unroll
                for (int i = 0; i < 2 * NP; ++i) x[r][i] = 0.0;
            }
        }
        for (int lv = 0; lv < levels; ++lv) {
            bool any = false;
#pragma unroll
            for (int r = 0; r < R; ++r) any = any || act[r];
            if (!__any(any)) break;             // wave-uniform: every lane takes the butterflies below
            double a0[R], a1[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a0[r] = 0.0;
                a1[r] = 0.0;
                if (act[r]) {
                    double v[2 * NP];
                    load_pairs<G, NP, VEC>(P0 + (int64_t)s[r] * d, d, g, v);
#pragma unroll
                    for (int i = 0; i < 2 * NP; ++i) a0[r] = fma(x[r][i], v[i], a0[r]);
                    if (cosine) {
                        load_pairs<G, NP, VEC>(P1 + (int64_t)s[r] * d, d, g, v);
#pragma unroll
                        for (int i = 0; i < 2 * NP; ++i) a1[r] = fma(x[r][i], v[i], a1[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a0[r] = group_sum<G>(a0[r]);
                if (cosine) a1[r] = group_sum<G>(a1[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (act[r]) {
                    // false on equality and on NaN: those rows go right
                    const bool go_left = cosine ? (1.0 - a0[r]) < (1.0 - a1[r]) : a0[r] < thr[s[r]];
                    s[r] = go_left ? l[r] : right[s[r]];
                    // the child's own children only where another level follows
                    l[r] = (lv + 1 < levels && s[r] >= 0 && s[r] < S) ? left[s[r]] : -1;
                    act[r] = l[r] >= 0;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g == 0 && row[r] < n && s[r] != s0[r]) slot[row[r]] = s[r];
    }
}

constexpr int BC_WAVES = csr::WAVES;       // the launch of csr_rows.h

template <typename I>
__global__ __launch_bounds__(64 * BC_WAVES) void bisect_descend_csr_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, int* __restrict__ slot, int S, const int* __restrict__ left, const int* __restrict__ right,
        const double* __restrict__ P0, const double* __restrict__ P1, const double* __restrict__ thr, int cosine,
        int levels) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * BC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * BC_WAVES;
    for (int64_t r = w0; r < n; r += nw) {
        const int s0 = __builtin_amdgcn_readfirstlane(slot[r]);
        int s = s0;
        int l = (s >= 0 && s < S) ? left[s] : -1;
        if (l < 0) continue;                    // the row's entries are not read
        const int64_t beg = crow[r], end = crow[r + 1];
        for (int lv = 0; lv < levels && l >= 0; ++lv) {
            const double* __restrict__ p0 = P0 + (int64_t)s * d;
            const double* __restrict__ p1 = cosine ? P1 + (int64_t)s * d : p0;
            double a0 = 0.0, a1 = 0.0;
            for (int64_t p = beg + lane; p < end; p += 64) {
                const int64_t c = (int64_t)col[p];
                if (c >= 0 && c < d) {
                    const double v = val[p];
                    a0 = fma(v, p0[c], a0);
                    if (cosine) a1 = fma(v, p1[c], a1);
                }
            }
            a0 = group_sum<64>(a0);
            if (cosine) a1 = group_sum<64>(a1);
            const bool go_left = cosine ? (1.0 - a0) < (1.0 - a1) : a0 < thr[s];
            s = __builtin_amdgcn_readfirstlane(go_left ? l : right[s]);
            l = (s >= 0 && s < S) ? left[s] : -1;
        }
        if (lane == 0 && s != s0) slot[r] = s;
    }
}

template <int G, int NP>
void launch_f64(bool vec, dim3 g, hipStream_t st, const double* X, int64_t n, int d, int* slot, int S,
               const int* left, const int* right, const double* P0, const double* P1, const double* thr,
               int cosine, int levels) {
    constexpr int R = NP >= BD_FLIGHT ? 1 : BD_FLIGHT / NP;
    if (vec)
        hipLaunchKernelGGL((bisect_descend_f64_kernel<G, NP, R, true>), g, dim3(BD_THREADS), 0, st, X, n, d, slot, S,
                           left, right, P0, P1, thr, cosine, levels);
    else
        hipLaunchKernelGGL((bisect_descend_f64_kernel<G, NP, R, false>), g, dim3(BD_THREADS), 0, st, X, n, d, slot,
                           S, left, right, P0, P1, thr, cosine, levels);
}

#ifndef BD_SEGMENT_LANES
#define BD_SEGMENT_LANES 4
#endif

inline int pow2_cover(int v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

// Lanes per row for vector size d, from d alone: a row of up to BD_SEGMENT_LANES pairs takes the power of two that
// covers its pairs (one 16-byte load per lane, the group's loads one contiguous segment); a longer row keeps
// BD_SEGMENT_LANES lanes with up to 8 pairs each (fewer butterfly steps per byte), and more lanes only where 8 pairs
// per lane do not cover it.
inline int lanes_for(int d) {
    const int pairs = (d + 1) / 2;
    const int seg = pow2_cover(pairs) < BD_SEGMENT_LANES ? pow2_cover(pairs) : BD_SEGMENT_LANES;
    const int need = pow2_cover((pairs + 7) / 8);
    const int G = seg > need ? seg : need;
    return G > 64 ? 64 : G;
}

}  // namespace

extern "C" {

// Descend the n fp64 rows X [n, d] (1 <= d <= 1024) up to `levels` levels from slot [n] (in place) through the tree
// table of S slots: left / right [S]; P0 (and P1 for COSINE) [., d] and thr [.] cover every slot with left >= 0.
int alink_bisect_descend_f64(const double* X, int64_t n, int d, int* slot, int S, const int* left, const int* right,
                             const double* P0, const double* P1, const double* thr, int cosine, int levels, int grid,
                             void* stream) {
    if (n <= 0 || levels <= 0 || S <= 0) return 0;
    if (d < 1 || d > 1024 || n >= (1ll << 31) || P0 == nullptr || (cosine ? P1 == nullptr : thr == nullptr)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int G = lanes_for(d);
    const int pairs = (d + 1) / 2;
    const int np = (pairs + G - 1) / G;
    const int NP = np <= 1 ? 1 : np <= 2 ? 2 : np <= 4 ? 4 : 8;
    const int R = NP >= BD_FLIGHT ? 1 : BD_FLIGHT / NP;
    const int64_t rows_per_pass = (int64_t)(BD_THREADS / G) * R;
    int64_t blocks = (n + rows_per_pass - 1) / rows_per_pass;
    const int64_t cap = grid > 0 ? grid : 4096;
    if (blocks > cap) blocks = cap;
    const dim3 g((unsigned)blocks);
    const bool vec = d % 2 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(P0) % 16 == 0 && reinterpret_cast<uintptr_t>(P1) % 16 == 0;
#define ALINK_BD(GG, PP) launch_f64<GG, PP>(vec, g, st, X, n, d, slot, S, left, right, P0, P1, thr, cosine, levels)
#define ALINK_BD_G(GG)                          \
    case GG:                                    \
        if (NP == 1) ALINK_BD(GG, 1);           \
        else if (NP == 2) ALINK_BD(GG, 2);      \
        else if (NP == 4) ALINK_BD(GG, 4);      \
        else ALINK_BD(GG, 8);                   \
        break
    switch (G) {
        ALINK_BD_G(1);
        ALINK_BD_G(2);
        ALINK_BD_G(4);
        ALINK_BD_G(8);
        ALINK_BD_G(16);
        ALINK_BD_G(32);
        default:
            ALINK_BD_G(64);
    }
#undef ALINK_BD_G
#undef ALINK_BD
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The same for n CSR rows (crow int64 [n+1]; col int32, or int64 with idx64; val fp64) under d >= 1 columns.
int alink_bisect_descend_csr(const int64_t* crow, const void* col, int idx64, const double* val, int64_t n, int64_t d,
                             int* slot, int S, const int* left, const int* right, const double* P0, const double* P1,
                             const double* thr, int cosine, int levels, int grid, void* stream) {
    if (n <= 0 || levels <= 0 || S <= 0) return 0;
    if (d < 1 || P0 == nullptr || (cosine ? P1 == nullptr : thr == nullptr)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ALINK_CSR_LAUNCH_IDX((bisect_descend_csr_kernel<int64_t>), (bisect_descend_csr_kernel<int32_t>), idx64,
                         csr::wave_blocks(n, grid, BC_WAVES, csr::WAVE_GRID), st, crow, col, val, n, d, slot, S, left,
                         right, P0, P1, thr, cosine, levels);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
