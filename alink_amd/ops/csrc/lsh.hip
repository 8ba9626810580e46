// Locality-sensitive hashing (``ops/lsh.py``): the table hashes of MinHash and of bucket random projection, and
// the exact distances of candidate pairs.  No float atomics; every result depends on the rows alone, never on the
// grid.  The host oracle is ``models/similarity/lsh.py``.
//
// * alink_lsh_minhash — CSR rows (crow int64, col int64, val fp64), coefficients A, B int32 [T * P]; out int32
//   [n, T].  Function f = t * P + p of a row: v = (1 + col) * (int64) A[f] + B[f], w = (int32) low 32 bits of v,
//   cur = w % 2038074743 (truncating, sign kept), mn = min over the entries with val != 0, starting from the prime
//   (an empty row keeps it).  Only the low 32 bits of v are used, so the product is taken in uint32.  The table
//   hash is Guava murmur3_32(0) over the P values written big-endian: block bswap32(mn), h ^= 4 P, fmix.
//   Lanes own hash functions, so the min needs no cross-lane reduction: L = the power of two that covers T * P
//   (at most 64) lanes serve a row, 64 / L rows share a wave (from T * P alone), and the row's entries are loaded
//   coalesced, L at a time, and broadcast.  With more functions than lanes, the tables are taken L / P at a time
//   (P > 64: one table in pieces of 64 projections, the murmur state carried by the table's lane).
// * alink_lsh_brp_hash — dots fp64 [n, T * P], offsets r [T * P], width w; out int32 [n, T]: the low 32 bits of
//   (int64) floor((dot + r) / w) (a true fp64 division) under the same murmur epilogue.  Non-finite projections
//   are not defined.
// * alink_lsh_pair_jaccard — two CSR index sets with strictly ascending rows, pairs pa, pb int64 [m]; out fp64 [m]
//   = 1 - (double) inter / (double) uni, 0 when both rows are empty.  G lanes per pair: a lane takes the entries
//   g, g + G, ... of the shorter row and binary-searches the longer one; a fixed xor butterfly adds the counts.
// * alink_lsh_pair_euclid_csr — sqrt(sum (a_j - b_j)^2) over the union of the two rows' entries, never densified:
//   a lane takes the entries g, g + G, ... of row a (the difference where b holds the column, found by binary
//   search), then those of row b that a does not hold, adds them in that order by fma, and the butterfly adds the
//   lanes.  G comes from the two matrices' mean row length, fixed for the call.
// * alink_lsh_pair_euclid_f64 — the same for dense rows [., d], any d >= 1: a lane owns the element pairs g,
//   g + G, ... of both rows (G from d alone), 16-byte loads where d is even and both bases are 16-byte aligned,
//   8-byte loads otherwise, the same elements in the same order either way.
//   So a pair's distance depends on the two rows only: equal rows give equal bits, identical rows exactly 0.
//   A pair whose index is outside its matrix reads nothing and gets NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_bcast.h"

namespace {

using lane::group_sum;
using lane::group_sum_int;

typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int LSH_THREADS = 256;
constexpr int LSH_PRIME = 2038074743;

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// one murmur3_32 block: the int32 value v written big-endian, read as a little-endian word
__device__ __forceinline__ uint32_t mm_block(uint32_t h, uint32_t v) {
    uint32_t k = __builtin_bswap32(v);
    k *= 0xCC9E2D51u;
    k = rotl32(k, 15);
    k *= 0x1B873593u;
    h ^= k;
    h = rotl32(h, 13);
    return h * 5u + 0xE6546B64u;
}

__device__ __forceinline__ uint32_t mm_fin(uint32_t h, int words) {
    h ^= 4u * (uint32_t)words;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// L lanes per row, 64 / L rows per wave.  Every loop around a cross-lane operation has a wave-uniform trip count.
template <int L>
__global__ __launch_bounds__(LSH_THREADS) void lsh_minhash_kernel(
        const int64_t* __restrict__ crow, const int64_t* __restrict__ col, const double* __restrict__ val, int64_t n,
        const int* __restrict__ A, const int* __restrict__ B, int T, int P, int* __restrict__ out) {
    constexpr int R = 64 / L;
    const int lane = threadIdx.x & 63;
    const int g = lane & (L - 1);
    const int gbase = lane - g;
    const int64_t wave = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * (LSH_THREADS / 64);
    const int PC = P < L ? P : L;               // projections of one piece
    const int TPC = L / PC;                     // tables of one piece (1 when P >= L)
    const int tl = g / PC, pl = g % PC;
    for (int64_t rb = wave * R; rb < n; rb += nwave * R) {
        const int64_t row = rb + lane / L;
        const bool valid = row < n;
        const int64_t beg = valid ? crow[row] : 0;
        const int64_t len = valid ? crow[row + 1] - beg : 0;
        for (int t0 = 0; t0 < T; t0 += TPC) {
            uint32_t h = 0;                     // lane g < TPC carries table t0 + g
            for (int p0 = 0; p0 < P; p0 += PC) {
                const int p = p0 + pl;
                const bool own = tl < TPC && t0 + tl < T && p < P;
                const int f = own ? (t0 + tl) * P + p : 0;
                const uint32_t a = (uint32_t)A[f], b = (uint32_t)B[f];
                int mn = LSH_PRIME;
                for (int64_t base = 0; __any(base < len); base += L) {
                    const int64_t i = base + g;
                    uint32_t c = 0;
                    bool ok = false;
                    if (i < len) {
                        c = (uint32_t)col[beg + i];
                        ok = val[beg + i] != 0.0;
                    }
                    const unsigned long long mask = __ballot(ok);
#pragma unroll
                    for (int j = 0; j < L; ++j) {
                        const uint32_t cj = (uint32_t)__shfl((int)c, j, L);
                        if ((mask >> (gbase + j)) & 1ull) {
                            const int w = (int)((1u + cj) * a + b);
                            const int cur = w % LSH_PRIME;
                            mn = cur < mn ? cur : mn;
                        }
                    }
                }
                const int cnt = P - p0 < PC ? P - p0 : PC;
                const bool head = g < TPC;
                for (int j = 0; j < PC; ++j) {
                    const int v = __shfl(mn, head ? g * PC + j : 0, L);
                    if (head && j < cnt) h = mm_block(h, (uint32_t)v);
                }
            }
            if (valid && g < TPC && t0 + g < T) out[row * T + t0 + g] = (int)mm_fin(h, P);
        }
    }
}

__global__ __launch_bounds__(LSH_THREADS) void lsh_brp_kernel(
        const double* __restrict__ dots, int64_t n, const double* __restrict__ r, double w, int T, int P,
        int* __restrict__ out) {
    const int64_t total = n * T;
    const int64_t F = (int64_t)T * P;
    for (int64_t i = (int64_t)blockIdx.x * LSH_THREADS + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * LSH_THREADS) {
        const int64_t row = i / T;
        const int t = (int)(i - row * T);
        const double* __restrict__ x = dots + row * F + (int64_t)t * P;
        const double* __restrict__ o = r + (int64_t)t * P;
        uint32_t h = 0;
        for (int p = 0; p < P; ++p) {
            const double q = floor((x[p] + o[p]) / w);
            h = mm_block(h, (uint32_t)(unsigned long long)(long long)q);
        }
        out[i] = (int)mm_fin(h, P);
    }
}

// the position of key in the strictly ascending col[beg .. beg + len), or -1
__device__ __forceinline__ int64_t find_col(const int64_t* __restrict__ col, int64_t beg, int64_t len, int64_t key) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[beg + mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < len && col[beg + lo] == key) ? beg + lo : -1;
}

struct PairRows {
    bool valid, ok;
    int64_t q, beg_a, len_a, beg_b, len_b;
};

// pair q of this pass for the lane's group; rows outside their matrix are not read (ok = false)
template <int G>
__device__ __forceinline__ PairRows pair_rows(int64_t base, const int64_t* __restrict__ pa,
                                              const int64_t* __restrict__ pb, int64_t m,
                                              const int64_t* __restrict__ crow_a, int64_t na,
                                              const int64_t* __restrict__ crow_b, int64_t nb) {
    PairRows r;
    r.q = base + threadIdx.x / G;
    r.valid = r.q < m;
    const int64_t a = r.valid ? pa[r.q] : -1, b = r.valid ? pb[r.q] : -1;
    r.ok = r.valid && a >= 0 && a < na && b >= 0 && b < nb;
    r.beg_a = r.ok ? crow_a[a] : 0;
    r.len_a = r.ok ? crow_a[a + 1] - r.beg_a : 0;
    r.beg_b = r.ok ? crow_b[b] : 0;
    r.len_b = r.ok ? crow_b[b + 1] - r.beg_b : 0;
    return r;
}

template <int G>
__global__ __launch_bounds__(LSH_THREADS) void lsh_pair_jaccard_kernel(
        const int64_t* __restrict__ crow_a, const int64_t* __restrict__ col_a, int64_t na,
        const int64_t* __restrict__ crow_b, const int64_t* __restrict__ col_b, int64_t nb,
        const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, int64_t m, double* __restrict__ out) {
    constexpr int PPB = LSH_THREADS / G;
    const int g = threadIdx.x & (G - 1);
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < m; base += (int64_t)gridDim.x * PPB) {
        const PairRows r = pair_rows<G>(base, pa, pb, m, crow_a, na, crow_b, nb);
        const bool a_short = r.len_a <= r.len_b;
        const int64_t* __restrict__ cs = a_short ? col_a : col_b;
        const int64_t* __restrict__ cl = a_short ? col_b : col_a;
        const int64_t bs = a_short ? r.beg_a : r.beg_b, ls = a_short ? r.len_a : r.len_b;
        const int64_t bl = a_short ? r.beg_b : r.beg_a, ll = a_short ? r.len_b : r.len_a;
        int cnt = 0;
        for (int64_t i = g; i < ls; i += G) cnt += find_col(cl, bl, ll, cs[bs + i]) >= 0 ? 1 : 0;
        cnt = group_sum_int<G>(cnt);
        if (g == 0 && r.valid) {
            const int64_t uni = r.len_a + r.len_b - cnt;
            out[r.q] = !r.ok ? __builtin_nan("") : uni == 0 ? 0.0 : 1.0 - (double)cnt / (double)uni;
        }
    }
}

template <int G>
__global__ __launch_bounds__(LSH_THREADS) void lsh_pair_euclid_csr_kernel(
        const int64_t* __restrict__ crow_a, const int64_t* __restrict__ col_a, const double* __restrict__ val_a,
        int64_t na, const int64_t* __restrict__ crow_b, const int64_t* __restrict__ col_b,
        const double* __restrict__ val_b, int64_t nb, const int64_t* __restrict__ pa,
        const int64_t* __restrict__ pb, int64_t m, double* __restrict__ out) {
    constexpr int PPB = LSH_THREADS / G;
    const int g = threadIdx.x & (G - 1);
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < m; base += (int64_t)gridDim.x * PPB) {
        const PairRows r = pair_rows<G>(base, pa, pb, m, crow_a, na, crow_b, nb);
        double acc = 0.0;
        for (int64_t i = g; i < r.len_a; i += G) {
            const int64_t k = find_col(col_b, r.beg_b, r.len_b, col_a[r.beg_a + i]);
            const double av = val_a[r.beg_a + i];
            const double df = k >= 0 ? av - val_b[k] : av;
            acc = fma(df, df, acc);
        }
        for (int64_t i = g; i < r.len_b; i += G) {
            if (find_col(col_a, r.beg_a, r.len_a, col_b[r.beg_b + i]) < 0) {
                const double bv = val_b[r.beg_b + i];
                acc = fma(bv, bv, acc);
            }
        }
        acc = group_sum<G>(acc);
        if (g == 0 && r.valid) out[r.q] = r.ok ? sqrt(acc) : __builtin_nan("");
    }
}

template <int G, bool VEC>
__global__ __launch_bounds__(LSH_THREADS) void lsh_pair_euclid_f64_kernel(
        const double* __restrict__ A, int64_t na, const double* __restrict__ B, int64_t nb, int d,
        const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, int64_t m, double* __restrict__ out) {
    constexpr int PPB = LSH_THREADS / G;
    const int g = threadIdx.x & (G - 1);
    const int pairs = (d + 1) / 2;
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < m; base += (int64_t)gridDim.x * PPB) {
        const int64_t q = base + threadIdx.x / G;
        const bool valid = q < m;
        const int64_t a = valid ? pa[q] : -1, b = valid ? pb[q] : -1;
        const bool ok = valid && a >= 0 && a < na && b >= 0 && b < nb;
        double acc = 0.0;
        if (ok) {
            const double* __restrict__ x = A + a * (int64_t)d;
            const double* __restrict__ y = B + b * (int64_t)d;
#pragma unroll 4
            for (int e = g; e < pairs; e += G) {
                const int j0 = 2 * e;
                double x0, x1, y0, y1;
                if (VEC) {
                    const d2_t xv = *reinterpret_cast<const d2_t*>(x + j0);
                    const d2_t yv = *reinterpret_cast<const d2_t*>(y + j0);
                    x0 = xv[0], x1 = xv[1], y0 = yv[0], y1 = yv[1];
                } else {
                    x0 = x[j0], y0 = y[j0];
                    x1 = j0 + 1 < d ? x[j0 + 1] : 0.0;
                    y1 = j0 + 1 < d ? y[j0 + 1] : 0.0;
                }
                const double d0 = x0 - y0, d1 = x1 - y1;
                acc = fma(d0, d0, acc);
                acc = fma(d1, d1, acc);
            }
        }
        acc = group_sum<G>(acc);
        if (g == 0 && valid) out[q] = ok ? sqrt(acc) : __builtin_nan("");
    }
}

inline int pow2_cover(int64_t v) {
    int p = 1;
    while (p < v && p < 64) p *= 2;
    return p;
}

// lanes per pair of CSR rows: a quarter of the two matrices' mean row length, a power of two in [1, 64]
inline int csr_lanes(int64_t na, int64_t nnz_a, int64_t nb, int64_t nnz_b) {
    const int64_t rows = na + nb > 0 ? na + nb : 1;
    const int64_t mean = (nnz_a + nnz_b + rows - 1) / rows;
    return pow2_cover((mean + 3) / 4);
}

// lanes per pair of dense rows, from d alone: up to 8 element pairs a lane, at least 4 lanes once a row has them
inline int dense_lanes(int d) {
    const int pairs = (d + 1) / 2;
    const int seg = pow2_cover(pairs) < 4 ? pow2_cover(pairs) : 4;
    const int need = pow2_cover((pairs + 7) / 8);
    return seg > need ? seg : need;
}

inline unsigned pass_blocks(int64_t items, int per_block, int grid, int64_t cap) {
    int64_t blocks = (items + per_block - 1) / per_block;
    const int64_t c = grid > 0 ? grid : cap;
    if (blocks > c) blocks = c;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

#define ALINK_LSH_SWITCH(G, CALL) \
    switch (G) {                  \
        case 1: CALL(1); break;   \
        case 2: CALL(2); break;   \
        case 4: CALL(4); break;   \
        case 8: CALL(8); break;   \
        case 16: CALL(16); break; \
        case 32: CALL(32); break; \
        default: CALL(64);        \
    }

}  // namespace

extern "C" {

// Table hashes out [n, T] of the n CSR rows under the MinHash coefficients A, B [T * P].
int alink_lsh_minhash(const int64_t* crow, const int64_t* col, const double* val, int64_t n, const int* A,
                      const int* B, int T, int P, int* out, int grid, void* stream) {
    if (n < 0 || T < 1 || P < 1 || (int64_t)T * P > (1 << 24)) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (crow == nullptr || A == nullptr || B == nullptr || out == nullptr) return hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int L = pow2_cover((int64_t)T * P);
    const int rows_per_block = (LSH_THREADS / 64) * (64 / L);
    const dim3 g(pass_blocks(n, rows_per_block, grid, 8192)), b(LSH_THREADS);
#define ALINK_LSH_MH(LL) \
    hipLaunchKernelGGL((lsh_minhash_kernel<LL>), g, b, 0, st, crow, col, val, n, A, B, T, P, out)
    ALINK_LSH_SWITCH(L, ALINK_LSH_MH)
#undef ALINK_LSH_MH
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Table hashes out [n, T] of the projections dots [n, T * P] with offsets r [T * P] and bucket width w.
int alink_lsh_brp_hash(const double* dots, int64_t n, const double* r, double w, int T, int P, int* out, int grid,
                       void* stream) {
    if (n < 0 || T < 1 || P < 1 || (int64_t)T * P > (1 << 24) || !(w > 0.0)) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (dots == nullptr || r == nullptr || out == nullptr) return hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(pass_blocks(n * T, LSH_THREADS, grid, 8192)), b(LSH_THREADS);
    hipLaunchKernelGGL(lsh_brp_kernel, g, b, 0, st, dots, n, r, w, T, P, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Jaccard distances out [m] of the pairs (pa, pb) of two CSR index sets (na / nb rows, nnz_a / nnz_b entries).
int alink_lsh_pair_jaccard(const int64_t* crow_a, const int64_t* col_a, int64_t na, int64_t nnz_a,
                           const int64_t* crow_b, const int64_t* col_b, int64_t nb, int64_t nnz_b,
                           const int64_t* pa, const int64_t* pb, int64_t m, double* out, int grid, void* stream) {
    if (m < 0 || na < 0 || nb < 0 || nnz_a < 0 || nnz_b < 0) return hipErrorInvalidValue;
    if (m == 0) return 0;
    if (crow_a == nullptr || crow_b == nullptr || pa == nullptr || pb == nullptr || out == nullptr)
        return hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int G = csr_lanes(na, nnz_a, nb, nnz_b);
    const dim3 g(pass_blocks(m, LSH_THREADS / G, grid, 8192)), b(LSH_THREADS);
#define ALINK_LSH_PJ(GG)                                                                                       \
    hipLaunchKernelGGL((lsh_pair_jaccard_kernel<GG>), g, b, 0, st, crow_a, col_a, na, crow_b, col_b, nb, pa, pb, \
                       m, out)
    ALINK_LSH_SWITCH(G, ALINK_LSH_PJ)
#undef ALINK_LSH_PJ
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Euclidean distances out [m] of the pairs (pa, pb) of two CSR matrices, over the union of the rows' entries.
int alink_lsh_pair_euclid_csr(const int64_t* crow_a, const int64_t* col_a, const double* val_a, int64_t na,
                              int64_t nnz_a, const int64_t* crow_b, const int64_t* col_b, const double* val_b,
                              int64_t nb, int64_t nnz_b, const int64_t* pa, const int64_t* pb, int64_t m,
                              double* out, int grid, void* stream) {
    if (m < 0 || na < 0 || nb < 0 || nnz_a < 0 || nnz_b < 0) return hipErrorInvalidValue;
    if (m == 0) return 0;
    if (crow_a == nullptr || crow_b == nullptr || pa == nullptr || pb == nullptr || out == nullptr)
        return hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int G = csr_lanes(na, nnz_a, nb, nnz_b);
    const dim3 g(pass_blocks(m, LSH_THREADS / G, grid, 8192)), b(LSH_THREADS);
#define ALINK_LSH_PE(GG)                                                                                          \
    hipLaunchKernelGGL((lsh_pair_euclid_csr_kernel<GG>), g, b, 0, st, crow_a, col_a, val_a, na, crow_b, col_b, val_b, \
                       nb, pa, pb, m, out)
    ALINK_LSH_SWITCH(G, ALINK_LSH_PE)
#undef ALINK_LSH_PE
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Euclidean distances out [m] of the pairs (pa, pb) of the dense fp64 rows A [na, d] and B [nb, d], d >= 1.
int alink_lsh_pair_euclid_f64(const double* A, int64_t na, const double* B, int64_t nb, int d, const int64_t* pa,
                              const int64_t* pb, int64_t m, double* out, int grid, void* stream) {
    if (m < 0 || na < 0 || nb < 0 || d < 1) return hipErrorInvalidValue;
    if (m == 0) return 0;
    if (pa == nullptr || pb == nullptr || out == nullptr || (na > 0 && A == nullptr) || (nb > 0 && B == nullptr))
        return hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int G = dense_lanes(d);
    const bool vec = d % 2 == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(B) % 16 == 0;
    const dim3 g(pass_blocks(m, LSH_THREADS / G, grid, 8192)), b(LSH_THREADS);
#define ALINK_LSH_PD(GG)                                                                                         \
    if (vec)                                                                                                     \
        hipLaunchKernelGGL((lsh_pair_euclid_f64_kernel<GG, true>), g, b, 0, st, A, na, B, nb, d, pa, pb, m, out); \
    else                                                                                                         \
        hipLaunchKernelGGL((lsh_pair_euclid_f64_kernel<GG, false>), g, b, 0, st, A, na, B, nb, d, pa, pb, m, out)
    ALINK_LSH_SWITCH(G, ALINK_LSH_PD)
#undef ALINK_LSH_PD
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
