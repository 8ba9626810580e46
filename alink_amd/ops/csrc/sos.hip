// Stochastic Outlier Selection (``ops/sos.py``): fp64 rows [n, d] of any d in [1, 1024], centred by the wrapper,
// against all n rows; all arithmetic fp64 and no [n, n] or [block, n] buffer anywhere.
//
// Both kernels are the loop of ``kmeans_dense64.hip``: a workgroup of 4 waves owns 64 rows (a wave its 16, one per
// lane column m = lane & 15) and streams every row of the matrix past them as the "centroids", 16 NT at a time,
// staged in LDS from the lane-ordered image of ``ops/kmeans_dense64._centroid_image``; the dots x_i . x_j run on
// v_mfma_f64_16x16x4_f64 from a zero accumulator, d zero-padded in the registers.  A lane then holds, for its own
// row i, the streamed rows j = (cb NT + t) 16 + (lane >> 4) + 4 q, and
//     D_ij = max(0, (q_i + q_j) - 2 dot_ij)
// with both norms from the one vector q, so both kernels see the same bits for a pair.  j == i is skipped by index.
//
// * alink_sos_search_f64 — ``solveForBeta`` per row: beta0 = 1, betaMin = 0, betaMax unbounded, tol 1e-2, at most 100
//   updates after the first evaluation.  One evaluation is one pass over all columns: a lane adds a = exp(-beta D)
//   and a D over its own slots in ascending column order, a fixed xor butterfly adds the four lane groups, and
//   logH = (sum a D) (beta / sum a) + log(sum a).  All lanes of a row hold the same sums and take the same branch; a
//   converged row freezes its state; the workgroup passes again while any of its rows is active (a workgroup vote,
//   since the staging has barriers).  Every scalar update is a correctly rounded IEEE operation.
// * alink_sos_products_f64 — the same loop with the roles swapped: the workgroup owns 64 columns j and streams the
//   rows i with their beta_i and s_i; a lane multiplies (1 - exp(-beta_i D_ij) / s_i) in ascending i in a register,
//   and a fixed butterfly multiplies the lane groups.
//
// No float atomics; which workgroup takes which batch changes no operation's order, so the bits are the same for
// every launch and every grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int SOS_WAVES = 4;          // waves per workgroup; a wave owns 16 rows of the workgroup's 64
constexpr int SOS_ROWS = 16 * SOS_WAVES;
constexpr int SOS_DCH = 32;           // dims per staged chunk (two 16-dim groups u = 0, 1)
constexpr int SOS_MAX_ITER = 100;
constexpr double SOS_TOL = 1.0e-2;

__device__ __forceinline__ d4_t mf64(double a, double b, d4_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// One pass of the workgroup's 64 rows over all n streamed rows.  PROD = false: r0 += a, r1 += a D with
// a = exp(-beta_own D) (this lane's slots only; the caller runs the butterfly).  PROD = true: r0 *= 1 - a / s_j with
// a = exp(-beta_j D).  img: per (block, dim chunk) NT * 512 doubles in [u][tile][g][m][step] order; qpad (and
// bpad, spad) hold nblk * 16 NT entries.  Every thread of the workgroup must call it (barriers).
template <int NT, bool VEC, bool PROD>
__device__ __forceinline__ void sos_pass(double* __restrict__ cent, const double* __restrict__ xr, bool row_ok,
                                         int64_t row, int64_t n, int d, const double* __restrict__ img,
                                         const double* __restrict__ qpad, const double* __restrict__ bpad,
                                         const double* __restrict__ spad, int nblk, int ndch, double qi,
                                         double beta_own, double& r0, double& r1) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int m = lane & 15, g = lane >> 4;
    for (int cb = 0; cb < nblk; ++cb) {
        d4_t acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int dc = 0; dc < ndch; ++dc) {
            // this lane's dims of its own row: dc * 32 + 16 u + 4 g + s; outside the row they are zero
            double xb[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j0 = dc * SOS_DCH + 16 * u + 4 * g;
                if (VEC) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        d2_t v = {0.0, 0.0};
                        if (row_ok && j0 + 2 * h < d) v = *reinterpret_cast<const d2_t*>(xr + j0 + 2 * h);
                        xb[u][2 * h] = v[0];
                        xb[u][2 * h + 1] = v[1];
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xb[u][s] = (row_ok && j0 + s < d) ? xr[j0 + s] : 0.0;
                }
            }
            // stage the streamed block of this dim chunk: a straight copy of NT * 4 KiB
            const d2_t* __restrict__ src =
                reinterpret_cast<const d2_t*>(img + ((int64_t)cb * ndch + dc) * (NT * 512));
            __syncthreads();        // the previous chunk's reads are done
#pragma unroll
            for (int i = 0; i < NT; ++i) reinterpret_cast<d2_t*>(cent)[i * 256 + tid] = src[i * 256 + tid];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int t0 = 0; t0 < NT; t0 += 4) {
                    d4_t a[NT < 4 ? NT : 4];
#pragma unroll
                    for (int t = 0; t < (NT < 4 ? NT : 4); ++t)
                        a[t] = *reinterpret_cast<const d4_t*>(cent + (((u * NT + t0 + t) * 4 + g) * 16 + m) * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
#pragma unroll
                        for (int t = 0; t < (NT < 4 ? NT : 4); ++t)
                            acc[t0 + t] = mf64(a[t][s], xb[u][s], acc[t0 + t]);
                    }
                }
            }
        }
        // ascending streamed index within the lane: tile, then register
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (cb * NT + t) * 16 + g + 4 * q;
                double D = (qi + qpad[c]) - 2.0 * acc[t][q];
                D = D < 0.0 ? 0.0 : D;          // a NaN stays NaN
                if (c < n && c != row) {
                    if (PROD) {
                        const double a = exp(-bpad[c] * D);
                        r0 *= 1.0 - a / spad[c];
                    } else {
                        const double a = exp(-beta_own * D);
                        r0 += a;
                        r1 += a * D;
                    }
                }
            }
        }
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(64 * SOS_WAVES) void sos_search_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ qpad, int nblk, int ndch, int64_t lo, int64_t hi, double logh,
        double* __restrict__ beta_out, double* __restrict__ s_out, int* __restrict__ iters_out) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (hi - lo + SOS_ROWS - 1) / SOS_ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = lo + b * SOS_ROWS + wave * 16 + m;
        const bool row_ok = row < hi;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)d;
        const double qi = row_ok ? qpad[row] : 0.0;
        double beta = 1.0, bmin = 0.0, bmax = __builtin_inf(), s_fin = 0.0;
        int iter = 0;
        bool active = row_ok;
        for (;;) {
            double sa = 0.0, sad = 0.0;
            sos_pass<NT, VEC, false>(cent, xr, row_ok, row, n, d, img, qpad, nullptr, nullptr, nblk, ndch, qi, beta,
                                     sa, sad);
            // the four lane groups of a row: both partners add the same two values, the same bits on either side
#pragma unroll
            for (int o = 16; o < 64; o <<= 1) {
                sa += __shfl_xor(sa, o, 64);
                sad += __shfl_xor(sad, o, 64);
            }
            if (active) {
                s_fin = sa;
                const double err = (sad * (beta / sa) + log(sa)) - logh;
                const bool nan = err != err;
                if (iter < SOS_MAX_ITER && (nan || fabs(err) > SOS_TOL)) {
                    if (nan) {
                        beta = beta / 10.0;
                    } else if (err > 0.0) {         // beta has to grow
                        bmin = beta;
                        beta = bmax == __builtin_inf() ? beta * 2.0 : 0.5 * (bmin + bmax);
                    } else {                        // beta has to shrink
                        bmax = beta;
                        beta = 0.5 * (bmin + beta);
                    }
                    ++iter;
                } else {
                    active = false;
                }
            }
            if (!__syncthreads_or(active ? 1 : 0)) break;
        }
        if (g == 0 && row_ok) {
            beta_out[row - lo] = beta;
            s_out[row - lo] = s_fin;
            iters_out[row - lo] = iter;
        }
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(64 * SOS_WAVES) void sos_products_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ qpad, const double* __restrict__ bpad, const double* __restrict__ spad, int nblk,
        int ndch, int64_t lo, int64_t hi, double* __restrict__ p_out) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (hi - lo + SOS_ROWS - 1) / SOS_ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t col = lo + b * SOS_ROWS + wave * 16 + m;
        const bool col_ok = col < hi;
        const double* __restrict__ xr = X + (col_ok ? col : 0) * (int64_t)d;
        const double qj = col_ok ? qpad[col] : 0.0;
        double p = 1.0, unused = 0.0;
        sos_pass<NT, VEC, true>(cent, xr, col_ok, col, n, d, img, qpad, bpad, spad, nblk, ndch, qj, 0.0, p, unused);
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) p *= __shfl_xor(p, o, 64);
        if (g == 0 && col_ok) p_out[col - lo] = p;
    }
}

bool sos_args_ok(int64_t n, int d, int nt, int nblk, int64_t lo, int64_t hi) {
    if (n < 2 || n >= (1ll << 31) || d < 1 || d > 1024 || nblk < 1 || (int64_t)nblk * nt * 16 < n) return false;
    if (nt != 1 && nt != 2 && nt != 4 && nt != 8) return false;
    return 0 <= lo && lo <= hi && hi <= n;
}

unsigned sos_blocks(int64_t rows, int grid) {
    int64_t blocks = (rows + SOS_ROWS - 1) / SOS_ROWS;
    if (grid > 0 && blocks > grid) blocks = grid;
    return (unsigned)blocks;
}

}  // namespace

extern "C" {

// solveForBeta of the rows [lo, hi) of the centred fp64 rows X [n, d] against all n rows.  img: the image of
// ``ops/kmeans_dense64._centroid_image`` of all n rows for tiles-per-block nt (nblk blocks of 16 nt slots, zero rows
// behind n); qpad [nblk * 16 nt]: the squared row norms, zero behind n.  Outputs [hi - lo]: beta, s = sum a at the
// final beta, iters int32.
int alink_sos_search_f64(const double* X, int64_t n, int d, const double* img, const double* qpad, int nt, int nblk,
                         int64_t lo, int64_t hi, double logh, double* beta, double* s, int* iters, int grid,
                         void* stream) {
    if (!sos_args_ok(n, d, nt, nblk, lo, hi)) return 1;
    if (hi == lo) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + SOS_DCH - 1) / SOS_DCH;
    const dim3 g(sos_blocks(hi - lo, grid)), b(64 * SOS_WAVES);
    const bool vec = d % 2 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
#define ALINK_SOS_SEARCH(NT)                                                                                       \
    do {                                                                                                           \
        if (vec)                                                                                                   \
            hipLaunchKernelGGL((sos_search_kernel<NT, true>), g, b, 0, st, X, n, d, img, qpad, nblk, ndch, lo, hi, \
                               logh, beta, s, iters);                                                              \
        else                                                                                                       \
            hipLaunchKernelGGL((sos_search_kernel<NT, false>), g, b, 0, st, X, n, d, img, qpad, nblk, ndch, lo,    \
                               hi, logh, beta, s, iters);                                                          \
    } while (0)
    if (nt == 1) ALINK_SOS_SEARCH(1);
    else if (nt == 2) ALINK_SOS_SEARCH(2);
    else if (nt == 4) ALINK_SOS_SEARCH(4);
    else ALINK_SOS_SEARCH(8);
#undef ALINK_SOS_SEARCH
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// p_j = prod over i != j of (1 - exp(-beta_i D_ij) / s_i) for the columns j in [lo, hi).  bpad / spad
// [nblk * 16 nt]: the rows' beta and s (any finite value behind n; those slots are skipped by index).
int alink_sos_products_f64(const double* X, int64_t n, int d, const double* img, const double* qpad,
                           const double* bpad, const double* spad, int nt, int nblk, int64_t lo, int64_t hi,
                           double* p, int grid, void* stream) {
    if (!sos_args_ok(n, d, nt, nblk, lo, hi)) return 1;
    if (hi == lo) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + SOS_DCH - 1) / SOS_DCH;
    const dim3 g(sos_blocks(hi - lo, grid)), b(64 * SOS_WAVES);
    const bool vec = d % 2 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
#define ALINK_SOS_PRODUCTS(NT)                                                                                     \
    do {                                                                                                           \
        if (vec)                                                                                                   \
            hipLaunchKernelGGL((sos_products_kernel<NT, true>), g, b, 0, st, X, n, d, img, qpad, bpad, spad, nblk, \
                               ndch, lo, hi, p);                                                                   \
        else                                                                                                       \
            hipLaunchKernelGGL((sos_products_kernel<NT, false>), g, b, 0, st, X, n, d, img, qpad, bpad, spad,      \
                               nblk, ndch, lo, hi, p);                                                             \
    } while (0)
    if (nt == 1) ALINK_SOS_PRODUCTS(1);
    else if (nt == 2) ALINK_SOS_PRODUCTS(2);
    else if (nt == 4) ALINK_SOS_PRODUCTS(4);
    else ALINK_SOS_PRODUCTS(8);
#undef ALINK_SOS_PRODUCTS
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
