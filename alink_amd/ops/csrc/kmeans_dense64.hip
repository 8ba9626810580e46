// Dense fp64 KMeans (``ops/kmeans_dense64.py``): fp64 rows [n, d] of any d in [1, 1024] against fp64 centroids,
// all arithmetic fp64.
//
// * alink_kmeans_dense64_nearest — score s[r, c] = x_r . c_c - |c_c|^2 / 2 on v_mfma_f64_16x16x4_f64, argmax per row.
//   The tile loop, the operand maps and the lane-ordered centroid image are those of dense64_mfma.h (the table is
//   the centroids): 64 rows per workgroup, blocks of 16 NT centroids, dim chunks of 32.  A lane holds four centroids
//   (lane >> 4) + 4 q per tile for its own row: the argmax runs down the lane's own registers first and across the
//   four lane groups last.
//   Accumulators start at -|c|^2 / 2 (0 for COSINE).  d is padded to the chunk with zeros in the registers: a load
//   is issued only for a (row, dim) inside [0, n) x [0, d).  Centroid slots at or past k are skipped by index in the
//   argmax, so they cannot win whatever the real scores are.  The scan is in ascending centroid index with a
//   strict `>`, and the merge across lane groups prefers the lower index on equal scores: bit-equal scores go to the
//   lowest index.  A NaN row compares false everywhere and keeps index 0.
//   Outputs (each optional): idx int32 [n]; distance fp64 [n] (EUCLIDEAN max(0, |x|^2 - 2 s), COSINE 1 - s); exact
//   per-centroid int64 counts (LDS histogram per workgroup when k <= 2048, integer atomics otherwise).
// * alink_kmeans_dense64_accum — per-cluster sums without float atomics.  The wrapper sorts the rows stably by
//   cluster (perm) and lists the work: chunk w = rows perm[wstart[w] .. wstart[w] + wlen[w]) of one cluster, at most
//   ACCUM_ROWS of them.  One wave per (chunk, 64-dim slice): lanes run over dims and add the chunk's rows in
//   ascending row order in a register, result to part [nchunk, d].  The merge kernel then adds every cluster's chunk
//   partials in chunk order (one lane per (cluster, dim)) into buf [k, d + 1] and writes the count (the cluster's
//   segment length) in the last column.  Which wave sums which chunk never changes the order of any addition, so
//   the result is bitwise identical for every launch and every grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense64_mfma.h"
#include "lane_bcast.h"

namespace {

using namespace d64;
using lane::bcast_i64;

constexpr int DN_HIST = 2048;        // largest k whose counts go through the LDS histogram

// img: the centroid image (dense64_mfma.h); ninit [nblk * 16 NT].  VEC: even d and 16-byte aligned X (load_chunk).
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void dense64_nearest_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ ninit, int k, int nblk, int ndch, int cosine, int* __restrict__ idx_out,
        double* __restrict__ dist_out, unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    __shared__ unsigned int hist[DN_HIST];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    const bool use_hist = counts != nullptr && k <= DN_HIST;
    if (use_hist) {
        for (int i = tid; i < k; i += 64 * WAVES) hist[i] = 0u;
        // the first barrier of the staging loop orders these stores before any histogram add
    }
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + m;
        const bool row_ok = row < n;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)d;
        double best = -__builtin_inf();
        int besti = 0;
        double xn = 0.0;
        for (int cb = 0; cb < nblk; ++cb) {
            d4_t acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[t][q] = ninit[(cb * NT + t) * 16 + g + 4 * q];
            }
            xn = 0.0;
            for (int dc = 0; dc < ndch; ++dc) {
                // this lane's dims of the row (zero outside it), then the centroid block of this dim chunk
                double xb[2][4];
                load_chunk<VEC>(xb, xr, row_ok, dc, g, d);
                stage<NT>(cent, img, cb, ndch, dc);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xn = fma(xb[u][s], xb[u][s], xn);
                    mfma_group<NT>(acc, cent, xb[u], u, g, m);
                }
            }
            // ascending centroid index within the lane: tile, then register
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = (cb * NT + t) * 16 + g + 4 * q;
                    const double sc = acc[t][q];
                    if (c < k && sc > best) {
                        best = sc;
                        besti = c;
                    }
                }
            }
        }
        // across the four lane groups of a row: the higher score, the lower index on equal scores
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            const double ox = __shfl_xor(xn, o, 64);
            xn += ox;           // both partners add the same two values: the same bits on either side
            if (ob > best || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        if (g == 0 && row_ok) {
            if (idx_out != nullptr) idx_out[row] = besti;
            if (dist_out != nullptr) {
                const double dd = cosine ? 1.0 - best : xn - 2.0 * best;
                // a NaN distance stays NaN; a negative rounding residue becomes 0
                dist_out[row] = cosine ? dd : (dd < 0.0 ? 0.0 : dd);
            }
            if (counts != nullptr) {
                if (use_hist) atomicAdd(&hist[besti], 1u);
                else atomicAdd(counts + besti, 1ull);
            }
        }
    }
    if (use_hist) {
        __syncthreads();
        for (int i = tid; i < k; i += 64 * WAVES) {
            const unsigned int h = hist[i];
            if (h != 0u) atomicAdd(counts + i, (unsigned long long)h);
        }
    }
}

constexpr int AC_WAVES = 4;
constexpr int AC_U = 8;              // row loads in flight per lane

// One wave per (chunk w, 64-dim slice sl): part[w, sl * 64 + lane] = sum of X[perm[p], sl * 64 + lane] over the
// chunk's positions p in ascending order.
__global__ __launch_bounds__(64 * AC_WAVES) void dense64_accum_kernel(
        const double* __restrict__ X, int d, const int64_t* __restrict__ perm, int64_t nchunk,
        const int64_t* __restrict__ wstart, const int32_t* __restrict__ wlen, int nslice,
        double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * AC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * AC_WAVES;
    const int64_t items = nchunk * nslice;
    for (int64_t it = w0; it < items; it += nw) {
        const int64_t w = it / nslice;
        const int j = (int)(it - w * nslice) * 64 + lane;
        const bool j_ok = j < d;
        const int64_t s = wstart[w];
        const int len = wlen[w];
        double acc = 0.0;
        for (int p = 0; p < len; p += 64) {
            const int cnt = (len - p) < 64 ? (len - p) : 64;
            const int64_t mine = lane < cnt ? perm[s + p + lane] : 0;
            for (int q0 = 0; q0 < cnt; q0 += AC_U) {
                double v[AC_U];
#pragma unroll
                for (int u = 0; u < AC_U; ++u) {
                    const int q = q0 + u;
                    // q is wave-uniform; lanes past the chunk hold row 0 and are not loaded
                    const int64_t r = bcast_i64(mine, q & 63);
                    v[u] = (q < cnt && j_ok) ? X[r * (int64_t)d + j] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < AC_U; ++u)
                    if (q0 + u < cnt) acc += v[u];
            }
        }
        if (j_ok) part[w * (int64_t)d + j] = acc;
    }
}

// buf[c, j] = part[cfirst[c], j] + part[cfirst[c] + 1, j] + ... (cnch[c] chunks, in order; 0 when none);
// buf[c, d] = the cluster's row count.
__global__ __launch_bounds__(256) void dense64_merge_kernel(
        int k, int d, const int64_t* __restrict__ cfirst, const int64_t* __restrict__ cnch,
        const int64_t* __restrict__ ccount, const double* __restrict__ part, double* __restrict__ buf) {
    const int64_t total = (int64_t)k * (d + 1);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / (d + 1));
        const int j = (int)(i - (int64_t)c * (d + 1));
        if (j == d) {
            buf[i] = (double)ccount[c];
            continue;
        }
        const int64_t f = cfirst[c], nc = cnch[c];
        double a = 0.0;
        if (nc > 0) {
            a = part[f * (int64_t)d + j];
            for (int64_t q = 1; q < nc; ++q) a += part[(f + q) * (int64_t)d + j];
        }
        buf[i] = a;
    }
}

}  // namespace

extern "C" {

// Nearest centroid of the n fp64 rows X [n, d] (1 <= d <= 1024).  img / ninit: the centroid image of
// ``ops/kmeans_dense64.centroid_image`` for tiles-per-block nt (1, 2, 4 or 8): nblk blocks of 16 nt centroid
// slots, ndch = ceil(d / 32) dim chunks.  idx / dist / counts may each be null; counts [k] int64 is added to.
int alink_kmeans_dense64_nearest(const double* X, int64_t n, int d, const double* img, const double* ninit, int k,
                                 int nt, int nblk, int cosine, int* idx, double* dist, void* counts, int grid,
                                 void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 1024 || k < 1 || nblk < 1 || (int64_t)nblk * nt * 16 < k || n >= (1ll << 31)) return 1;
    if (!nt_ok(nt)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + DCH - 1) / DCH;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    ALINK_D64_LAUNCH(dense64_nearest_kernel, nt, 1, 2, 4, 8, vec_ok(d, X), row_blocks(n, grid, 1024), st, X, n, d,
                     img, ninit, k, nblk, ndch, cosine, idx, dist, cnt);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Per-cluster sums of X [n, d] through the cluster-sorted row list perm (every entry in [0, n)): nchunk chunks
// (wstart, wlen) summed into part [nchunk, d], then merged per cluster (cfirst, cnch, ccount: [k]) into
// buf [k, d + 1].  Every element of buf is written.
int alink_kmeans_dense64_accum(const double* X, int d, const int64_t* perm, int64_t nchunk, const int64_t* wstart,
                               const int32_t* wlen, int k, const int64_t* cfirst, const int64_t* cnch,
                               const int64_t* ccount, double* part, double* buf, int grid, void* stream) {
    if (d < 1 || d > 1024 || k < 1) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t cap = grid > 0 ? grid : 16384;
    if (nchunk > 0) {
        const int nslice = (d + 63) / 64;
        int64_t blocks = (nchunk * nslice + AC_WAVES - 1) / AC_WAVES;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(dense64_accum_kernel, dim3((unsigned)blocks), dim3(64 * AC_WAVES), 0, st, X, d, perm,
                           nchunk, wstart, wlen, nslice, part);
    }
    int64_t mblocks = ((int64_t)k * (d + 1) + 255) / 256;
    if (mblocks > cap) mblocks = cap;
    hipLaunchKernelGGL(dense64_merge_kernel, dim3((unsigned)mblocks), dim3(256), 0, st, k, d, cfirst, cnch, ccount,
                       part, buf);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
