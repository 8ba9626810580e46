// Multinomial (softmax) regression on CSR rows, gfx950 / MI355X: the row pass and the gradient gather of
// models/linear/objfunc.py SoftmaxObjFunc for a sparse FeatureMatrix (crow int64 [n+1]; col int32 / int64; val fp64;
// m columns, the intercept column among them), coefficients W [k1, m] (pivot class k1 with logit 0, 1 <= k1 <= 64),
// fp64 class indices y in [0, k1] and weights w (ops/softmax_csr.py).  All arithmetic is fp64.  No [nnz, k1] block, no
// dense row, no float atomics.
//
// alink_softmax_csr_rows: one wave per row on the row walk of csr_rows.h (row_dots, its entry guard: an entry whose
// column is outside [0, m) adds nothing).  The table is W transposed and padded to 64 columns, T [m, 64], so lane l
// owns class l and a stored entry reads one contiguous line of T.  Search: the table is [W ; D], each padded to 64,
// T [m, 128] (NB = 2): class l keeps lane l in both halves, acc[0] = x . W_l and acc[1] = x . D_l.
//   softmax a lane holds one logit.  The maximum (the pivot's 0 included) and the sum of exp go over the 64 lanes by a
//           fixed xor butterfly (1, 2, ..., 32), the pivot's term is added last; lanes at or past k1 are left out by
//           index: they never enter the maximum and add exactly 0.  fmax drops a NaN logit from the maximum as in the
//           dense kernel, and the NaN then reaches the sum as in ops/softmax.py.  lse = max + log(sum),
//           loss = lse - eta[y] (0 for the pivot), r_c = w (exp(eta_c - lse) - [c == y]).  The label's logit comes by
//           one v_readlane (y is uniform over the wave).  A row's outputs depend on the row alone.
//   search  e_s = ec - s (beta ed) per lane, s < nsteps <= 64, and w (lse(e_s) - e_s[y]) from the two logit registers:
//           the row is read once.
//   sums    a wave's work item is a block of SMC_RB consecutive rows, walked in row order; lane s keeps the running sum
//           of step s (lane 0 the plain loss sum), so a block gives one partial per step, part [nsteps, nb].
//           The batch sums of ordered_sum.h add a step's partials by a rule of nb alone.  Nothing depends on the grid.
//   outputs by mask: R [n, k1]; the loss sum(s); the per-row loss without the weight.
//
// alink_softmax_csr_grad: Gt [m, k1], Gt[j, c] = sum over the entries (i, j, v) of v R[i, c], through the CSC view and
// the (column, chunk of at most 512 entries) work list of ops/kmeans_sparse.prepare.  A wave owns one work item.  With
// P = k1 rounded up to a power of two and E = 64 / P, lane (e, c) = e P + c owns class c and the chunk's entries e,
// e + E, e + 2 E, ...: the wave loads 64 (row, value) pairs coalesced, lane group e takes entry j + e by ds_bpermute,
// gathers R[row, c] (a contiguous k1-double line per entry, E lines per step) and fmas in ascending entry order; the
// gathers of GU steps are issued before their fmas.  A fixed xor butterfly over e (P, 2 P, ..., 32) finishes the chunk.
// So 4 classes take 16 entries per step, 64 classes one.  A single-chunk column writes Gt; a longer column writes its
// chunk partials to part [nslots, k1] and smc_merge_kernel, one wave per such column, adds them in chunk order with 16
// loads in flight.  A value depends on (column, k1) alone, never on the grid, the run or the wave.
#include <math.h>

#include "csr_rows.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using csr::WAVES;

constexpr int SMC_KMAX = 64, SMC_MAX_STEPS = 64;
constexpr int SMC_RB = 16;          // rows of one loss partial (a wave's work item)
constexpr int SMC_GU = 4;           // steps of the gather whose loads are issued together
constexpr int SMC_MU = 16;          // chunk partials the merge loads together
enum { M_R = 1, M_LOSS = 2, M_ROWLOSS = 4 };

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// log(1 + sum_{c < k1} exp(e_c)) of the row whose class `lane` has the logit e; the same on every lane
__device__ __forceinline__ double row_lse(double e, bool cls) {
    const double mx = wave_max(cls ? fmax(0.0, e) : 0.0);
    const double se = osum::wave_sum_asc(cls ? exp(e - mx) : 0.0) + exp(0.0 - mx);
    return mx + log(se);
}

template <bool SEARCH, typename I>
__global__ __launch_bounds__(64 * WAVES) void smc_rows_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t m, const double* __restrict__ y, const double* __restrict__ w, int k1, const double* __restrict__ T,
        double beta, int nsteps, int mask, double* __restrict__ R, double* __restrict__ rloss,
        double* __restrict__ part, int64_t nb) {
    constexpr int NB = SEARCH ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bool cls = lane < k1;
    const int64_t nw = csr::item_stride();
    for (int64_t b = csr::first_item(); b < nb; b += nw) {
        const int64_t r0 = b * SMC_RB, r1 = r0 + SMC_RB < n ? r0 + SMC_RB : n;
        double lsum = 0.0;          // lane s: the block's sum of step s
        for (int64_t r = r0; r < r1; ++r) {
            const auto d = csr::row_dots<NB, 8, csr::NBMAX>(col, val, crow[r], crow[r + 1], m, T, 64 * NB, 0, lane);
            const double wi = w[r];
            const int yi = __builtin_amdgcn_readfirstlane((int)y[r]);
            const bool lab = yi >= 0 && yi < k1;        // else the pivot: its logit is 0
            if constexpr (SEARCH) {
                const double ec = d.acc[0], dd = d.acc[1] * beta;
                const double ecy = lab ? lane::bcast_f64(ec, yi & 63) : 0.0;
                const double dy = (lab ? lane::bcast_f64(d.acc[1], yi & 63) : 0.0) * beta;
                for (int s = 0; s < nsteps; ++s) {
                    const double sd = (double)s;
                    const double lse = row_lse(ec - sd * dd, cls);
                    const double v = (lse - (ecy - sd * dy)) * wi;
                    if (lane == s) lsum += v;
                }
            } else {
                const double e = d.acc[0];
                const double lse = row_lse(e, cls);
                const double ey = lab ? lane::bcast_f64(e, yi & 63) : 0.0;
                const double loss = lse - ey;
                if (lane == 0) {
                    lsum += loss * wi;
                    if (mask & M_ROWLOSS) rloss[r] = loss;
                }
                if ((mask & M_R) && cls) {
                    double rc = exp(e - lse);
                    if (lane == yi) rc -= 1.0;
                    R[r * (int64_t)k1 + lane] = rc * wi;
                }
            }
        }
        if ((SEARCH || (mask & M_LOSS)) && lane < nsteps) part[(int64_t)lane * nb + b] = lsum;
    }
}

// One wave per work item: entries [wstart, wstart + wlen) of the CSC arrays, all of column wcol.  P: k1 rounded up to
// a power of two; lane e P + c owns class c and every (64 / P)-th entry from e on.
template <int P>
__global__ __launch_bounds__(64 * WAVES) void smc_grad_kernel(
        const int32_t* __restrict__ rows, const double* __restrict__ vals, const double* __restrict__ R, int k1,
        int64_t nwork, const int64_t* __restrict__ wcol, const int64_t* __restrict__ wstart,
        const int32_t* __restrict__ wlen, const int64_t* __restrict__ wslot, double* __restrict__ Gt,
        double* __restrict__ part) {
    constexpr int E = 64 / P;
    constexpr int GU = E * SMC_GU > 64 ? 64 / E : SMC_GU;       // no step past the 64 loaded entries
    const int lane = threadIdx.x & 63;
    const int c = lane & (P - 1), e = lane / P;
    const bool cls = c < k1;
    const int cc = cls ? c : 0;         // every address formed below lies inside R, whatever the lane
    const int64_t nw = csr::item_stride();
    for (int64_t it = csr::first_item(); it < nwork; it += nw) {
        const int64_t s = wstart[it], slot = wslot[it];
        const int len = wlen[it];
        double acc = 0.0;
        for (int p = 0; p < len; p += 64) {
            const int cnt = (len - p) < 64 ? (len - p) : 64;
            int row = 0;
            double v = 0.0;
            if (lane < cnt) {
                row = rows[s + p + lane];
                v = vals[s + p + lane];
            }
            for (int j0 = 0; j0 < cnt; j0 += E * GU) {
                double vv[GU], rr[GU];
                bool ok[GU];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int j = j0 + u * E + e;       // the source lane is taken mod 64 (a loaded row or row 0)
                    ok[u] = cls && j < cnt;
                    const int ri = __shfl(row, j & 63, 64);
                    vv[u] = __shfl(v, j & 63, 64);
                    rr[u] = ok[u] ? R[(int64_t)ri * k1 + cc] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < GU; ++u)
                    if (ok[u]) acc = fma(vv[u], rr[u], acc);
            }
        }
#pragma unroll
        for (int o = P; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
        if (e == 0 && cls) (slot < 0 ? Gt + wcol[it] * (int64_t)k1 : part + slot * (int64_t)k1)[c] = acc;
    }
}

// The columns of several chunks: Gt[mcol[i], :] = part[mfirst[i]] + part[mfirst[i] + 1] + ... in chunk order, one wave
// per column, lane c its class c
__global__ __launch_bounds__(64 * WAVES) void smc_merge_kernel(
        int64_t nmulti, const int64_t* __restrict__ mcol, const int64_t* __restrict__ mfirst,
        const int64_t* __restrict__ mcount, int k1, const double* __restrict__ part, double* __restrict__ Gt) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = csr::item_stride();
    for (int64_t i = csr::first_item(); i < nmulti; i += nw) {
        if (lane >= k1) continue;
        const double* __restrict__ p = part + mfirst[i] * (int64_t)k1 + lane;
        const int64_t cnt = mcount[i];
        double a = p[0];
        int64_t q = 1;
        for (; q + SMC_MU <= cnt; q += SMC_MU) {
            double t[SMC_MU];
#pragma unroll
            for (int u = 0; u < SMC_MU; ++u) t[u] = p[(q + u) * (int64_t)k1];
#pragma unroll
            for (int u = 0; u < SMC_MU; ++u) a += t[u];
        }
        for (; q < cnt; ++q) a += p[q * (int64_t)k1];
        Gt[mcol[i] * (int64_t)k1 + lane] = a;
    }
}

}  // namespace

extern "C" {

// The row pass over n CSR rows (crow int64 [n+1]; col int32, or int64 with idx64; val fp64) under m columns, y and w
// [n].  Plain (search == 0): T [m, 64] is W transposed and padded; mask 1 writes R [n, k1], mask 2 gives out [1] =
// sum w loss, mask 4 writes rloss [n] = the rows' losses without the weight.  Search: T [m, 128] is [W ; D], each
// padded to 64 columns, and out [nsteps] = the weighted losses at W - s beta D, s < nsteps <= 64.
// part [nsteps, ceil(n / 16)] (nsteps = 1 for the plain pass) is needed with out.
int alink_softmax_csr_rows(const int64_t* crow, const void* col, int idx64, const double* val, int64_t n, int64_t m,
                           const double* y, const double* w, int k1, const double* T, int search, double beta,
                           int nsteps, int mask, double* R, double* rloss, double* part, double* out, int grid,
                           void* stream) {
    if (n <= 0) return 0;
    if (m < 1 || k1 < 1 || k1 > SMC_KMAX || n >= (1ll << 31)) return 1;
    if (crow == nullptr || y == nullptr || w == nullptr || T == nullptr) return 1;
    if (search) {
        if (nsteps < 1 || nsteps > SMC_MAX_STEPS || part == nullptr || out == nullptr) return 1;
        mask = 0;
    } else {
        if (mask <= 0 || mask > (M_R | M_LOSS | M_ROWLOSS)) return 1;
        if ((mask & M_R) && R == nullptr) return 1;
        if ((mask & M_LOSS) && (part == nullptr || out == nullptr)) return 1;
        if ((mask & M_ROWLOSS) && rloss == nullptr) return 1;
        nsteps = 1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nb = (n + SMC_RB - 1) / SMC_RB;
    const unsigned blocks = csr::wave_blocks(nb, grid, WAVES, csr::WAVE_GRID);
    if (search)
        ALINK_CSR_LAUNCH_IDX((smc_rows_kernel<true, int64_t>), (smc_rows_kernel<true, int32_t>), idx64, blocks, st,
                             crow, col, val, n, m, y, w, k1, T, beta, nsteps, mask, R, rloss, part, nb);
    else
        ALINK_CSR_LAUNCH_IDX((smc_rows_kernel<false, int64_t>), (smc_rows_kernel<false, int32_t>), idx64, blocks, st,
                             crow, col, val, n, m, y, w, k1, T, beta, nsteps, mask, R, rloss, part, nb);
    if (search || (mask & M_LOSS))
        osum::batch_sums(part, nb, nsteps, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Gt [m, k1]: Gt[j, :] = sum of v R[i, :] over the entries of column j, through the CSC view (rows int32 /
// vals fp64, sorted by column, rows ascending inside a column) and its work list (ops/kmeans_sparse.prepare): nwork
// items (wcol, wstart, wlen <= 512, wslot: -1 = the column's only chunk, else its row of part [nslots, k1]), then
// nmulti multi-chunk columns (mcol, mfirst, mcount) merged in chunk order.  R [n, k1].  Gt must be zeroed by the caller
// (columns without entries are not written).
int alink_softmax_csr_grad(const int32_t* rows, const double* vals, const double* R, int k1, int64_t nwork,
                           const int64_t* wcol, const int64_t* wstart, const int32_t* wlen, const int64_t* wslot,
                           int64_t nmulti, const int64_t* mcol, const int64_t* mfirst, const int64_t* mcount,
                           double* Gt, double* part, int grid, void* stream) {
    if (nwork <= 0) return 0;
    if (k1 < 1 || k1 > SMC_KMAX || R == nullptr || Gt == nullptr || (nmulti > 0 && part == nullptr)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(csr::wave_blocks(nwork, grid, WAVES, csr::WAVE_GRID)), b(64 * WAVES);
#define ALINK_SMC_GRAD(P)                                                                                          \
    hipLaunchKernelGGL((smc_grad_kernel<P>), g, b, 0, st, rows, vals, R, k1, nwork, wcol, wstart, wlen, wslot, Gt, \
                       part)
    if (k1 == 1) ALINK_SMC_GRAD(1);
    else if (k1 == 2) ALINK_SMC_GRAD(2);
    else if (k1 <= 4) ALINK_SMC_GRAD(4);
    else if (k1 <= 8) ALINK_SMC_GRAD(8);
    else if (k1 <= 16) ALINK_SMC_GRAD(16);
    else if (k1 <= 32) ALINK_SMC_GRAD(32);
    else ALINK_SMC_GRAD(64);
#undef ALINK_SMC_GRAD
    if (nmulti > 0)
        hipLaunchKernelGGL(smc_merge_kernel, dim3(csr::wave_blocks(nmulti, grid, WAVES, csr::WAVE_GRID)), b, 0, st,
                           nmulti, mcol, mfirst, mcount, k1, part, Gt);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
