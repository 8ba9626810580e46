// Sparse-vector KMeans (``ops/kmeans_sparse.py``): CSR rows against dense centroids, all arithmetic fp64.
//
// * alink_kmeans_sparse_nearest — one wave per CSR row, on the row walk of csr_rows.h (the table is the centroids,
//   transposed and padded, Ct [d, kp]; the lane / cluster map and the entry guard are described there): per cluster
//   block the walk gives the lane's dots and |x|^2, and this file keeps the score and the argmin.
//   score_c = cn[c] - mul * dot_c (EUCLIDEAN: cn = |c|^2, mul = 2; COSINE: cn = 0, mul = 1; padded clusters carry
//   cn = +inf), the wave argmin keeps the LOWEST index on equal scores (the reference's strict `<` scan).  k beyond
//   one register block loops over cluster blocks with a running best.  Entries whose column is outside [0, d)
//   contribute nothing, to the dot products and to |x|^2 alike.
//   Outputs (each optional): idx int32 [n]; best distance fp64 [n] (EUCLIDEAN max(0, |x|^2 + score), COSINE
//   1 + score); exact per-cluster int64 counts by integer atomics (the k-means|| weights pass).
// * alink_kmeans_sparse_accum — per-cluster column sums without float atomics, through the CSC view of the rows
//   (entries stably sorted by column, so rows ascend inside a column).  One wave per work item = (column, chunk of
//   at most ACCUM_CHUNK consecutive entries): it reads 64 (row, value) pairs at a time, gathers idx[row], and
//   walks them in order; only the lane that owns the entry's cluster adds, so a chunk is summed in ascending row
//   order in registers.  A single-chunk column's sums go straight to sumT [d, kp]; a longer column's chunk
//   partials go to a side buffer that alink_kmeans_sparse_accum (second launch) adds in chunk order.  The result
//   does not depend on the grid and is bitwise identical from run to run.
#include "csr_rows.h"

namespace {

using csr::NBMAX;
using csr::WAVES;

// NB, U: cluster blocks of 64 per pass and entries whose gathers are issued together (csr_rows.h).
template <int NB, int U, typename I>
__global__ __launch_bounds__(64 * WAVES) void sparse_nearest_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, const double* __restrict__ Ct, const double* __restrict__ cn, int kp, double mul, int cosine,
        int* __restrict__ idx_out, double* __restrict__ dist_out, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = csr::item_stride();
    for (int64_t r = csr::first_item(); r < n; r += nw) {
        const int64_t s = crow[r], e = crow[r + 1];
        double best = __builtin_inf();
        int besti = 0;
        double xn = 0.0;
        for (int cb = 0; cb < kp; cb += 64 * NB) {
            const auto w = csr::row_dots<NB, U, NBMAX>(col, val, s, e, d, Ct, kp, cb, lane);
            xn = w.xn;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = cb + 64 * b + lane;
                if (NB < NBMAX || cb + 64 * b < kp) {
                    const double sc = cn[c] - mul * w.acc[b];
                    if (sc < best) {          // ascending c within a lane: strict < keeps the lowest index
                        best = sc;
                        besti = c;
                    }
                }
            }
        }
        // wave argmin over (score, index): the lower index wins equal scores
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ob < best || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        if (lane == 0) {
            if (idx_out != nullptr) idx_out[r] = besti;
            if (dist_out != nullptr) {
                const double dd = cosine ? 1.0 + best : xn + best;
                dist_out[r] = cosine ? dd : (dd > 0.0 ? dd : 0.0);
            }
            if (counts != nullptr) atomicAdd(counts + besti, 1ull);
        }
    }
}

// One wave per work item w: entries [wstart[w], wstart[w] + wlen[w]) of the CSC arrays, all of column wcol[w].
// The sums of clusters [cb, cb + 64 NB) go to sumT[wcol[w], :] (wslot[w] < 0) or part[wslot[w], :].
template <int NB>
__global__ __launch_bounds__(64 * WAVES) void sparse_accum_kernel(
        const int32_t* __restrict__ rows, const double* __restrict__ vals, const int* __restrict__ idx,
        int64_t nwork, const int64_t* __restrict__ wcol, const int64_t* __restrict__ wstart,
        const int32_t* __restrict__ wlen, const int64_t* __restrict__ wslot, int kp, double* __restrict__ sumT,
        double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    for (int64_t w = w0; w < nwork; w += nw) {
        const int64_t s = wstart[w];
        const int len = wlen[w];
        const int64_t slot = wslot[w];
        double* __restrict__ dst = slot < 0 ? sumT + wcol[w] * (int64_t)kp : part + slot * (int64_t)kp;
        for (int cb = 0; cb < kp; cb += 64 * NB) {
            double acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = 0.0;
            for (int p = 0; p < len; p += 64) {
                const int m = (len - p) < 64 ? (len - p) : 64;
                int a = -1;
                double v = 0.0;
                if (lane < m) {
                    a = idx[rows[s + p + lane]] - cb;             // the entry's cluster, relative to this pass
                    v = vals[s + p + lane];
                }
                for (int j = 0; j < m; ++j) {
                    const int mine = __builtin_amdgcn_readlane(a, j) - lane;     // 64 b on the owning lane
                    const double vj = lane::bcast_f64(v, j);
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] += (mine == 64 * b) ? vj : 0.0;
                }
            }
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (NB < NBMAX || cb + 64 * b < kp) dst[cb + 64 * b + lane] = acc[b];
        }
    }
}

// The columns that span several chunks: sumT[mcol[i], :] = part[mfirst[i]] + part[mfirst[i] + 1] + ... in chunk
// order, one wave per column, one lane per cluster.
__global__ __launch_bounds__(64 * WAVES) void sparse_accum_merge_kernel(
        int64_t nmulti, const int64_t* __restrict__ mcol, const int64_t* __restrict__ mfirst,
        const int64_t* __restrict__ mcount, int kp, const double* __restrict__ part, double* __restrict__ sumT) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    for (int64_t i = w0; i < nmulti; i += nw) {
        const int64_t f = mfirst[i], cnt = mcount[i];
        double* __restrict__ dst = sumT + mcol[i] * (int64_t)kp;
        for (int c = lane; c < kp; c += 64) {
            double a = part[f * (int64_t)kp + c];
            for (int64_t q = 1; q < cnt; ++q) a += part[(f + q) * (int64_t)kp + c];
            dst[c] = a;
        }
    }
}

}  // namespace

extern "C" {

// Nearest centroid of n CSR rows (crow int64 [n+1]; col int32, or int64 with idx64; val fp64) among the kp padded
// columns of Ct [d, kp] (kp a multiple of 64, d >= 1); cn [kp] is the score offset (+inf on padded clusters), the
// score is cn[c] - mul * dot_c.  idx / dist / counts may each be null; counts [kp] int64 is added to (zero it).
int alink_kmeans_sparse_nearest(const int64_t* crow, const void* col, int idx64, const double* val, int64_t n,
                                int64_t d, const double* Ct, const double* cn, int kp, double mul, int cosine,
                                int* idx, double* dist, void* counts, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || kp < 64 || kp % 64 != 0) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ALINK_CSR_LAUNCH(sparse_nearest_kernel, kp, idx64, csr::wave_blocks(n, grid, WAVES, csr::WAVE_GRID), st, crow, col,
                     val, n, d, Ct, cn, kp, mul, cosine, idx, dist, reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Column sums per cluster through the CSC view (rows int32 / vals fp64, sorted by column, rows ascending inside a
// column) and the rows' clusters idx int32 [n]: nwork work items (wcol, wstart, wlen <= the chunk size, wslot:
// -1 = the column's only chunk, else its row of part), then nmulti multi-chunk columns (mcol, mfirst, mcount)
// merged in chunk order.  sumT [d, kp] must be zeroed by the caller (columns without entries are not written).
int alink_kmeans_sparse_accum(const int32_t* rows, const double* vals, const int* idx, int64_t nwork,
                              const int64_t* wcol, const int64_t* wstart, const int32_t* wlen, const int64_t* wslot,
                              int64_t nmulti, const int64_t* mcol, const int64_t* mfirst, const int64_t* mcount,
                              int kp, double* sumT, double* part, int grid, void* stream) {
    if (nwork <= 0) return 0;
    if (kp < 64 || kp % 64 != 0) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(csr::wave_blocks(nwork, grid, WAVES, csr::WAVE_GRID)), b(64 * WAVES);
    if (kp == 64)
        hipLaunchKernelGGL((sparse_accum_kernel<1>), g, b, 0, st, rows, vals, idx, nwork, wcol, wstart, wlen, wslot,
                           kp, sumT, part);
    else if (kp == 128)
        hipLaunchKernelGGL((sparse_accum_kernel<2>), g, b, 0, st, rows, vals, idx, nwork, wcol, wstart, wlen, wslot,
                           kp, sumT, part);
    else
        hipLaunchKernelGGL((sparse_accum_kernel<4>), g, b, 0, st, rows, vals, idx, nwork, wcol, wstart, wlen, wslot,
                           kp, sumT, part);
    if (nmulti > 0)
        hipLaunchKernelGGL(sparse_accum_merge_kernel, dim3(csr::wave_blocks(nmulti, grid, WAVES, csr::WAVE_GRID)), b, 0,
                           st, nmulti, mcol, mfirst, mcount, kp, part, sumT);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
