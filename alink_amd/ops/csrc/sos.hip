// Stochastic Outlier Selection (``ops/sos.py``): fp64 rows [n, d] of any d in [1, 1024], centred by the wrapper,
// against all n rows; all arithmetic fp64 and no [n, n] or [block, n] buffer anywhere.
//
// Both kernels run the tile loop of dense64_mfma.h (operand maps and image layout are described there): a workgroup
// owns 64 rows and streams every row of the matrix past them as the table, 16 NT at a time, from the image
// ``ops/kmeans_dense64.centroid_image`` makes of the rows themselves; the dots x_i . x_j start from a zero
// accumulator, d zero-padded in the registers.  A lane then holds, for its own row i, the streamed rows
// j = (cb NT + t) 16 + (lane >> 4) + 4 q, and
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

#include "dense64_mfma.h"

namespace {

using namespace d64;

constexpr int SOS_MAX_ITER = 100;
constexpr double SOS_TOL = 1.0e-2;

// One pass of the workgroup's 64 rows over all n streamed rows.  PROD = false: r0 += a, r1 += a D with
// a = exp(-beta_own D) (this lane's slots only; the caller runs the butterfly).  PROD = true: r0 *= 1 - a / s_j with
// a = exp(-beta_j D).  img: the image of all rows (dense64_mfma.h); qpad (and bpad, spad) hold nblk * 16 NT
// entries.  Every thread of the workgroup must call it (barriers).
template <int NT, bool VEC, bool PROD>
__device__ __forceinline__ void sos_pass(double* __restrict__ cent, const double* __restrict__ xr, bool row_ok,
                                         int64_t row, int64_t n, int d, const double* __restrict__ img,
                                         const double* __restrict__ qpad, const double* __restrict__ bpad,
                                         const double* __restrict__ spad, int nblk, int ndch, double qi,
                                         double beta_own, double& r0, double& r1) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, g = lane >> 4;
    for (int cb = 0; cb < nblk; ++cb) {
        d4_t acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int dc = 0; dc < ndch; ++dc) {
            // this lane's dims of its own row (zero outside it), then the streamed block of this dim chunk
            double xb[2][4];
            load_chunk<VEC>(xb, xr, row_ok, dc, g, d);
            stage<NT>(cent, img, cb, ndch, dc);
#pragma unroll
            for (int u = 0; u < 2; ++u) mfma_group<NT>(acc, cent, xb[u], u, g, m);
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
__global__ __launch_bounds__(64 * WAVES) void sos_search_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ qpad, int nblk, int ndch, int64_t lo, int64_t hi, double logh,
        double* __restrict__ beta_out, double* __restrict__ s_out, int* __restrict__ iters_out) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (hi - lo + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = lo + b * ROWS + wave * 16 + m;
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
            // the four lane groups of a row
            sa = group_sum(sa);
            sad = group_sum(sad);
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
__global__ __launch_bounds__(64 * WAVES) void sos_products_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ qpad, const double* __restrict__ bpad, const double* __restrict__ spad, int nblk,
        int ndch, int64_t lo, int64_t hi, double* __restrict__ p_out) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (hi - lo + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t col = lo + b * ROWS + wave * 16 + m;
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
    if (!nt_ok(nt)) return false;
    return 0 <= lo && lo <= hi && hi <= n;
}

}  // namespace

extern "C" {

// solveForBeta of the rows [lo, hi) of the centred fp64 rows X [n, d] against all n rows.  img: the image of
// ``ops/kmeans_dense64.centroid_image`` of all n rows for tiles-per-block nt (nblk blocks of 16 nt slots, zero rows
// behind n); qpad [nblk * 16 nt]: the squared row norms, zero behind n.  Outputs [hi - lo]: beta, s = sum a at the
// final beta, iters int32.
int alink_sos_search_f64(const double* X, int64_t n, int d, const double* img, const double* qpad, int nt, int nblk,
                         int64_t lo, int64_t hi, double logh, double* beta, double* s, int* iters, int grid,
                         void* stream) {
    if (!sos_args_ok(n, d, nt, nblk, lo, hi)) return 1;
    if (hi == lo) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + DCH - 1) / DCH;
    ALINK_D64_LAUNCH(sos_search_kernel, nt, 1, 2, 4, 8, vec_ok(d, X), row_blocks(hi - lo, grid, 0), st, X, n, d, img,
                     qpad, nblk, ndch, lo, hi, logh, beta, s, iters);
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
    const int ndch = (d + DCH - 1) / DCH;
    ALINK_D64_LAUNCH(sos_products_kernel, nt, 1, 2, 4, 8, vec_ok(d, X), row_blocks(hi - lo, grid, 0), st, X, n, d,
                     img, qpad, bpad, spad, nblk, ndch, lo, hi, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
