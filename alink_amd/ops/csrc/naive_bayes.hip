// Naive Bayes text prediction (``ops/naive_bayes.py``): every row against the L class rows of the model table in one
// pass over the rows, all arithmetic fp64, no [nnz, L] buffer and no dense copy of a CSR row.
//
// The model operand is a table M [L, d] (Multinomial: theta; Bernoulli: minMat = theta - log(1 - e^theta)) and an
// offset vector off [L] (Multinomial: pi; Bernoulli: pi + phi).  The score of class c is s_c = off[c] + x . M[c, :].
// Outputs per row, each pointer may be null:
//
//   pred  int32 [n]     the reference's findMaxProbLabel: ascending class index with a strict `<` from -inf, so
//                       bit-equal scores go to the lowest index, a NaN score never wins, and a row with no score above
//                       -inf gets -1;
//   prob  fp64 [n, L]   generateDetail's numbers exp(s_c - (m + log sum_c exp(s_c - m))), m the row maximum.  The
//                       row's slice of prob holds the scores between the passes over the classes: a lane writes s_c
//                       to slot c, and reads back only the slots it wrote itself;
//   bad   one int32     Bernoulli only: set (an integer atomic or) when a value inside [0, d) is neither 0 nor 1, by
//                       Java's `value == 0. || value == 1.`: -0.0 passes, NaN does not.  Guarded and padded
//                       positions hold 0.0 and never trip it.
//
// * alink_nb_rows_csr — CSR rows (int32 / int64 columns), one wave per row, on the row walk of csr_rows.h (the table
//   is M transposed and padded, Mt [d, kp]; the lane / class map and the entry guard are described there; padded
//   classes carry off = -inf).  More than 256 classes loop over class blocks with a running maximum, as the nearest
//   kernel of kmeans_sparse.hip does.  The 0 / 1 check is the walk's per-entry hook, in the first class block.  Each
//   lane adds its classes' exp terms in ascending class order and a fixed xor butterfly adds the lanes.
//   Choices: no LDS (a table row is read once per entry, coalesced over the lanes); 4 rows per 256-thread workgroup;
//   up to 16384 workgroups striding over the rows.
// * alink_nb_rows_f64 — dense fp64 rows [n, d], 1 <= d <= 1024, any L, on the tile loop of dense64_mfma.h (the table
//   is M; operand maps and the image layout are described there): 64 rows per workgroup, blocks of 16 NT classes, dim
//   chunks of 32, the image of ``kmeans_dense64.centroid_image``.  The accumulators start at off[c].  Class slots at
//   or past L are skipped by index in the argmax and add nothing to the sum.  The epilogue takes the maximum and the
//   argmax over the lane's own accumulators first (ascending class), then over the four lane groups of the row, the
//   order of kmeans_dense64.hip; the exp terms the same way, each lane in ascending class order, then the fixed
//   xor-16 / xor-32 sum.  The 0 / 1 check runs on the row chunk in registers, in the first class block.
//   Choices: LDS 4 NT KiB per workgroup (<= 32 KiB); the grid is capped at 1024 workgroups striding over the batches.
//
// A row's outputs depend on the row alone: no float atomics, the same bits for every grid and every run.
// Non-finite inputs are not guaranteed beyond the rules above.  Plain C++ and vector stores only.
#include "csr_rows.h"
#include "dense64_mfma.h"

namespace {

// Java's `value == 0. || value == 1.`
__device__ __forceinline__ bool nb_is01(double v) { return v == 0.0 || v == 1.0; }

// The hook of the CSR walk (csr_rows.h) that checks the entries' values; a guarded entry is (0, 0.0) and passes.
struct check01 {
    bool on;            // the first class block's walk alone
    int bad;
    __device__ __forceinline__ double gather(const double* __restrict__) const { return 0.0; }
    __device__ __forceinline__ void fold(double v, double) {
        if (on && !nb_is01(v)) bad = 1;
    }
};

// Mt [d, kp]; off [kp], -inf past L.  NB, U: class blocks of 64 per pass and entries whose gathers are issued
// together (csr_rows.h).
template <int NB, int U, typename I, bool BERN>
__device__ __forceinline__ void nb_rows_csr_body(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, const double* __restrict__ Mt, const double* __restrict__ off, int L, int kp,
        int* __restrict__ pred, double* __restrict__ prob, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = csr::item_stride();
    int badw = 0;
    for (int64_t r = csr::first_item(); r < n; r += nw) {
        const int64_t s = crow[r], e = crow[r + 1];
        double* __restrict__ pr = prob != nullptr ? prob + r * (int64_t)L : nullptr;
        double best = -__builtin_inf();
        int besti = -1;
        for (int cb = 0; cb < kp; cb += 64 * NB) {
            double acc[NB];
            if (BERN) {
                const auto w = csr::row_dots<NB, U, csr::NBMAX>(col, val, s, e, d, Mt, kp, cb, lane,
                                                                check01{cb == 0, badw});
                badw = w.hook.bad;
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = w.acc[b];
            } else {
                const auto w = csr::row_dots<NB, U, csr::NBMAX>(col, val, s, e, d, Mt, kp, cb, lane);
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = w.acc[b];
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = cb + 64 * b + lane;
                if ((NB < csr::NBMAX || cb + 64 * b < kp) && c < L) {
                    const double sc = off[c] + acc[b];
                    if (pr != nullptr) pr[c] = sc;
                    if (best < sc) {          // ascending c within a lane: strict < keeps the lowest index
                        best = sc;
                        besti = c;
                    }
                }
            }
        }
        // wave argmax over (score, index): the lower index wins equal scores; -1 goes with -inf on every lane
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (best < ob || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        if (lane == 0 && pred != nullptr) pred[r] = besti;
        if (pr != nullptr) {
            // the lane's own slots, ascending class; then the fixed butterfly over the lanes
            double sum = 0.0;
            for (int c = lane; c < L; c += 64) sum += exp(pr[c] - best);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            const double lse = best + log(sum);
            for (int c = lane; c < L; c += 64) pr[c] = exp(pr[c] - lse);
        }
    }
    if (BERN && badw != 0 && lane == 0) atomicOr(bad, 1);
}

template <int NB, int U, typename I>
__global__ __launch_bounds__(64 * csr::WAVES) void nb_rows_csr_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, const double* __restrict__ Mt, const double* __restrict__ off, int L, int kp,
        int* __restrict__ pred, double* __restrict__ prob, int* __restrict__ bad) {
    nb_rows_csr_body<NB, U, I, false>(crow, col, val, n, d, Mt, off, L, kp, pred, prob, bad);
}

template <int NB, int U, typename I>
__global__ __launch_bounds__(64 * csr::WAVES) void nb_rows_csr_check_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, const double* __restrict__ Mt, const double* __restrict__ off, int L, int kp,
        int* __restrict__ pred, double* __restrict__ prob, int* __restrict__ bad) {
    nb_rows_csr_body<NB, U, I, true>(crow, col, val, n, d, Mt, off, L, kp, pred, prob, bad);
}

using namespace d64;

// img: the image of M (dense64_mfma.h); init [nblk * 16 NT] = off, 0 on the padded slots.  VEC: even d and 16-byte
// aligned X (load_chunk).  check: the 0 / 1 rule of Bernoulli, bad non-null.
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void nb_rows_f64_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ init, int L, int nblk, int ndch, int check, int* __restrict__ pred,
        double* __restrict__ prob, int* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    int badl = 0;
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + m;
        const bool row_ok = row < n;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)d;
        double* __restrict__ pr = (prob != nullptr && row_ok) ? prob + row * (int64_t)L : nullptr;
        double best = -__builtin_inf();
        int besti = -1;
        for (int cb = 0; cb < nblk; ++cb) {
            d4_t acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[t][q] = init[(cb * NT + t) * 16 + g + 4 * q];
            }
            for (int dc = 0; dc < ndch; ++dc) {
                // this lane's dims of the row (zero outside it), then the table block of this dim chunk
                double xb[2][4];
                load_chunk<VEC>(xb, xr, row_ok, dc, g, d);
                if (check && cb == 0) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            if (!nb_is01(xb[u][s])) badl = 1;
                    }
                }
                stage<NT>(cent, img, cb, ndch, dc);
#pragma unroll
                for (int u = 0; u < 2; ++u) mfma_group<NT>(acc, cent, xb[u], u, g, m);
            }
            // ascending class index within the lane: tile, then register
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = (cb * NT + t) * 16 + g + 4 * q;
                    const double sc = acc[t][q];
                    if (c < L) {
                        if (pr != nullptr) pr[c] = sc;
                        if (best < sc) {
                            best = sc;
                            besti = c;
                        }
                    }
                }
            }
        }
        // across the four lane groups of a row: the higher score, the lower index on equal scores
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (best < ob || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        if (g == 0 && row_ok && pred != nullptr) pred[row] = besti;
        if (prob != nullptr) {
            // the lane's own slots (classes g + 4 q of every tile), ascending; then the four lane groups
            double sum = 0.0;
            if (pr != nullptr) {
                for (int c0 = 0; c0 < L; c0 += 16) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = c0 + g + 4 * q;
                        if (c < L) sum += exp(pr[c] - best);
                    }
                }
            }
            sum = group_sum(sum);
            if (pr != nullptr) {
                const double lse = best + log(sum);
                for (int c0 = 0; c0 < L; c0 += 16) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = c0 + g + 4 * q;
                        if (c < L) pr[c] = exp(pr[c] - lse);
                    }
                }
            }
        }
    }
    if (check && __any(badl) && lane == 0) atomicOr(bad, 1);
}

}  // namespace

extern "C" {

// n CSR rows (crow int64 [n+1]; col int32, or int64 with idx64; val fp64) under the d columns of the model against
// Mt [d, kp], the table transposed and padded (kp a multiple of 64, L <= kp), off [kp] with -inf past L.  pred int32
// [n], prob fp64 [n, L] and bad (one int32, or-ed into: zero it) may each be null; bad is read only with bernoulli.
int alink_nb_rows_csr(const int64_t* crow, const void* col, int idx64, const double* val, int64_t n, int64_t d,
                      const double* Mt, const double* off, int L, int kp, int bernoulli, int* pred, double* prob,
                      int* bad, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || L < 1 || kp < 64 || kp % 64 != 0 || L > kp || n >= (1ll << 31)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = csr::wave_blocks(n, grid, csr::WAVES, csr::WAVE_GRID);
    if (bernoulli && bad != nullptr)
        ALINK_CSR_LAUNCH(nb_rows_csr_check_kernel, kp, idx64, blocks, st, crow, col, val, n, d, Mt, off, L, kp, pred,
                         prob, bad);
    else
        ALINK_CSR_LAUNCH(nb_rows_csr_kernel, kp, idx64, blocks, st, crow, col, val, n, d, Mt, off, L, kp, pred, prob,
                         bad);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// n fp64 rows X [n, d] (1 <= d <= 1024, 8-byte aligned).  img: the image of the table M [L, d] by
// ``ops/kmeans_dense64.centroid_image`` for tiles-per-block nt (1, 2, 4 or 8), nblk blocks of 16 nt class slots;
// init [nblk * 16 nt] = off, zero on the padded slots.  pred, prob and bad as above.
int alink_nb_rows_f64(const double* X, int64_t n, int d, const double* img, const double* init, int L, int nt,
                      int nblk, int bernoulli, int* pred, double* prob, int* bad, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 1024 || L < 1 || nblk < 1 || (int64_t)nblk * nt * 16 < L || n >= (1ll << 31)) return 1;
    if (!nt_ok(nt)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + DCH - 1) / DCH;
    const int check = bernoulli && bad != nullptr;
    ALINK_D64_LAUNCH(nb_rows_f64_kernel, nt, 1, 2, 4, 8, vec_ok(d, X), row_blocks(n, grid, 1024), st, X, n, d, img,
                     init, L, nblk, ndch, check, pred, prob, bad);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
