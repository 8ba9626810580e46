// Dense fp64 KMeans (``ops/kmeans_dense64.py``): fp64 rows [n, d] of any d in [1, 1024] against fp64 centroids,
// all arithmetic fp64.
//
// * alink_kmeans_dense64_nearest — score s[r, c] = x_r . c_c - |c_c|^2 / 2 on v_mfma_f64_16x16x4_f64, argmax per row.
//   A workgroup of 4 waves takes 64 rows at a time (a wave its 16), and walks the centroids in blocks of 16 NT
//   (NT = 1, 2, 4 or 8 tiles) and the dims in chunks of 32.  The MFMA's A operand is the centroid tile (row = centroid
//   lane & 15, k = lane >> 4), its B operand the rows (k = lane >> 4, column = row lane & 15), so the result holds one
//   data row per lane column and four centroids (lane >> 4) + 4 q per lane: the argmax runs down the lane's own
//   registers first and across the four lane groups last.  The k order inside a 16-dim group is permuted the same way
//   on both operands (lane group g owns dims 4 g .. 4 g + 3, one per MFMA step), so a lane's loads of X are 32
//   contiguous bytes.  The centroid block of a dim chunk is staged in LDS from an image the wrapper laid out in
//   exactly the order the lanes read it ([u][tile][g][m][step], 32 bytes per lane, conflict-free ds_read_b128).
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

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int DN_WAVES = 4;          // waves per workgroup; a wave owns 16 rows of the workgroup's 64
constexpr int DN_ROWS = 16 * DN_WAVES;
constexpr int DN_DCH = 32;           // dims per staged chunk (two 16-dim groups u = 0, 1)
constexpr int DN_HIST = 2048;        // largest k whose counts go through the LDS histogram

__device__ __forceinline__ d4_t mf64(double a, double b, d4_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// img: per (centroid block, dim chunk) NT * 512 doubles in [u][tile][g][m][step] order; ninit [nblk * 16 NT].
// VEC: d is even and X is 16-byte aligned, so a lane's four dims are two aligned 16-byte loads.
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * DN_WAVES) void dense64_nearest_kernel(
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
        for (int i = tid; i < k; i += 64 * DN_WAVES) hist[i] = 0u;
        // the first barrier of the staging loop orders these stores before any histogram add
    }
    const int64_t nbatch = (n + DN_ROWS - 1) / DN_ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * DN_ROWS + wave * 16 + m;
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
                // this lane's rows of X: dims dc * 32 + 16 u + 4 g + s; outside the row they are zero
                double xb[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j0 = dc * DN_DCH + 16 * u + 4 * g;
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
                // stage the centroid block of this dim chunk: a straight copy of NT * 4 KiB
                const d2_t* __restrict__ src =
                    reinterpret_cast<const d2_t*>(img + ((int64_t)cb * ndch + dc) * (NT * 512));
                __syncthreads();        // the previous chunk's reads are done
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    reinterpret_cast<d2_t*>(cent)[i * 256 + tid] = src[i * 256 + tid];
                __syncthreads();
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xn = fma(xb[u][s], xb[u][s], xn);
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
        for (int i = tid; i < k; i += 64 * DN_WAVES) {
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
                    const int lo = __builtin_amdgcn_readlane((int)(mine & 0xffffffffll), q & 63);
                    const int hi = __builtin_amdgcn_readlane((int)(mine >> 32), q & 63);
                    const int64_t r = ((int64_t)hi << 32) | (uint32_t)lo;
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
// ``ops/kmeans_dense64._centroid_image`` for tiles-per-block nt (1, 2, 4 or 8): nblk blocks of 16 nt centroid
// slots, ndch = ceil(d / 32) dim chunks.  idx / dist / counts may each be null; counts [k] int64 is added to.
int alink_kmeans_dense64_nearest(const double* X, int64_t n, int d, const double* img, const double* ninit, int k,
                                 int nt, int nblk, int cosine, int* idx, double* dist, void* counts, int grid,
                                 void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 1024 || k < 1 || nblk < 1 || (int64_t)nblk * nt * 16 < k || n >= (1ll << 31)) return 1;
    if (nt != 1 && nt != 2 && nt != 4 && nt != 8) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + DN_DCH - 1) / DN_DCH;
    int64_t blocks = (n + DN_ROWS - 1) / DN_ROWS;
    const int64_t cap = grid > 0 ? grid : 1024;
    if (blocks > cap) blocks = cap;
    const dim3 g((unsigned)blocks), b(64 * DN_WAVES);
    const bool vec = d % 2 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define ALINK_DN_NEAREST(NT)                                                                                       \
    do {                                                                                                           \
        if (vec)                                                                                                   \
            hipLaunchKernelGGL((dense64_nearest_kernel<NT, true>), g, b, 0, st, X, n, d, img, ninit, k, nblk,      \
                               ndch, cosine, idx, dist, cnt);                                                      \
        else                                                                                                       \
            hipLaunchKernelGGL((dense64_nearest_kernel<NT, false>), g, b, 0, st, X, n, d, img, ninit, k, nblk,     \
                               ndch, cosine, idx, dist, cnt);                                                      \
    } while (0)
    if (nt == 1) ALINK_DN_NEAREST(1);
    else if (nt == 2) ALINK_DN_NEAREST(2);
    else if (nt == 4) ALINK_DN_NEAREST(4);
    else ALINK_DN_NEAREST(8);
#undef ALINK_DN_NEAREST
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
