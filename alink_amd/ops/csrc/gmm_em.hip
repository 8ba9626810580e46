// Fused GMM EM step on fp64 rows (``ops/gmm.py``): contiguous fp64 X0 [n, d] (rows centred by the global mean),
// 1 <= d <= 128, any k >= 1, n < 2^31, all arithmetic fp64.  No [n, k d] buffer anywhere.
//
// * alink_gmm_em_rows_f64 — the E pass.  Every projection z_j = X0 W_j - C_j (C_j = (mu_j - xbar) W_j) on
//   v_mfma_f64_16x16x4_f64 with the operand maps, the row-chunk load and the butterfly of dense64_mfma.h: the
//   columns of all W_j are the table, [k dpad, d] with dpad = d rounded up to 16, so a tile of 16 columns never
//   straddles two components; padded columns are zero in W and in C and add nothing.  A workgroup of 4 waves takes
//   64 rows at a time (a wave its 16) and keeps their dims in registers for the whole walk over the components; a
//   lane holds the four columns (lane >> 4) + 4 q of a tile for its own row.  The LDS layout is this kernel's own
//   (tile outermost; see the layout note of dense64_mfma.h), and so are its staging and its MFMA loop.
//   The image is staged in LDS in groups of GT tiles x all dim chunks (32 KiB at most): at
//   d = 128 a component's W_j (128 KiB) does not fit and is streamed in column blocks; |z|^2 separates over the
//   columns, so streaming is exact; an image of a single group is staged once per workgroup.  Accumulators start
//   at -C.
//   Epilogue per row and component: q_j = sum_c z_jc^2, the lane adding its own accumulators in ascending (tile,
//   register) order, then a fixed xor butterfly (16, 32) over the four lane groups that share the row;
//   lp_j = cst_j - q_j / 2 (cst_j folds -(rank_j log 2 pi + logdet_j) / 2 + log w_j).  Every lane of a row then
//   holds the same lp_j.  The argmax runs in ascending j with a strict `>`: bit-equal values go to the lowest j,
//   and a padded slot is never a candidate.  lp_j is parked in R[i, j] by the lane group j & 3, which alone reads
//   it back: the row's maximum is known by then, each lane group adds exp(lp_j - max) over its own j in ascending
//   order, the butterfly finishes the sum, lse_i = max + log(sum), and R[i, j] = exp(lp_j - lse_i).
//   sum_i lse_i: one partial per 64-row batch (rows in lane order, waves in wave order), and a single-workgroup
//   kernel adds the batch partials by a fixed rule (thread t takes batches t, t + 1024, ... in order, then a fixed
//   LDS tree).  Neither a row's outputs nor the sum depend on the grid.
// * alink_gmm_em_moments_f64 — the M pass: rs_j = sum_i r_ij, xs_j = sum_i r_ij x0_i, xxs_j = sum_i r_ij x0_i x0_i^T.
//   Work units are (row chunk, group of 2 or 4 components, tile row ta, block of at most 4 tiles tb >= ta): one wave
//   per unit (its components share every load of the rows) walks the chunk's rows four at a time (lane group
//   g = lane >> 4 takes row i0 + g; 16 rows of loads are in flight before their products) and computes its tiles
//   of (r . X0)^T X0 on the fp64 MFMA: A = r_i x_i[16 ta + m], B = x_i[16 tb + m].  The units of a chunk are
//   neighbours in the grid, so the re-reads of its rows meet in L2.
//   The running sums of A and r in the unit that holds the diagonal tile give xs and rs after the same
//   butterfly.  Only the upper tile triangle is computed; the merge kernel adds the chunk partials in chunk
//   order, one lane per output element, reading element (min(a, b), max(a, b)) for both (a, b) and (b, a).  No
//   float atomics; the chunk length comes from the caller and does not depend on the grid, so the result has the
//   same bits for every launch and every grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dense64_mfma.h"

namespace {

using namespace d64;

constexpr int EM_M_WAVES = 4;        // waves per workgroup of the M pass, one unit each
constexpr int EM_RED = 1024;         // threads of the log-likelihood reduction

constexpr int em_group_tiles(int ndch) { return ndch == 1 ? 8 : (ndch == 2 ? 4 : 2); }

// img: per tile and dim chunk 512 doubles in [u][g][m][step] order ([tile][dch] outside), ninit [ngroup * GT * 16].
// VEC: even d and 16-byte aligned X (load_chunk).
template <int NDCH, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void gmm_em_rows_kernel(
        const double* __restrict__ X, int64_t n, int d, const double* __restrict__ img,
        const double* __restrict__ ninit, const double* __restrict__ cst, int k, int tpc, int ngroup,
        double* R, int* __restrict__ arg_out, double* __restrict__ part) {
    constexpr int GT = em_group_tiles(NDCH);
    constexpr int TI = GT < 4 ? GT : 4;         // tiles interleaved in the MFMA stream
    __shared__ __attribute__((aligned(16))) double cent[GT * NDCH * 512];
    __shared__ double wsum[2][WAVES];        // by batch parity: see the end of the batch loop
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + m;
        const bool row_ok = row < n;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)d;
        // this lane's dims of its row: dc * 32 + 16 u + 4 g + s; outside the row they are zero
        double xb[NDCH][2][4];
#pragma unroll
        for (int dc = 0; dc < NDCH; ++dc) load_chunk<VEC>(xb[dc], xr, row_ok, dc, g, d);
        double* __restrict__ rrow = R != nullptr ? R + (row_ok ? row : 0) * (int64_t)k : nullptr;
        double best = -__builtin_inf();
        int besti = 0;
        double qs = 0.0;
        int j = 0, tin = 0;
        for (int grp = 0; grp < ngroup; ++grp) {
            const d2_t* __restrict__ src = reinterpret_cast<const d2_t*>(img + (int64_t)grp * (GT * NDCH * 512));
            // the real tiles of this group (the last group may end in zero tiles, which are neither staged nor
            // multiplied; their accumulators are never read)
            const int left = k * tpc - grp * GT;
            const int nt_here = left < GT ? left : GT;
            // an image of one group is staged once per workgroup and serves all its batches
            if (ngroup > 1 || b == (int64_t)blockIdx.x) {
                __syncthreads();        // the previous group's reads are done
#pragma unroll
                for (int i = 0; i < GT * NDCH; ++i)
                    if (i < nt_here * NDCH) reinterpret_cast<d2_t*>(cent)[i * 256 + tid] = src[i * 256 + tid];
                __syncthreads();
            }
            d4_t acc[GT];
#pragma unroll
            for (int t = 0; t < GT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[t][q] = ninit[((int64_t)grp * GT + t) * 16 + g + 4 * q];
            }
#pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (dc * 32 + 16 * u >= d) continue;        // a 16-dim group of zeros past d
#pragma unroll
                    for (int t0 = 0; t0 < GT; t0 += TI) {
                        if (t0 >= nt_here) continue;
                        d4_t a[TI];
#pragma unroll
                        for (int t = 0; t < TI; ++t)
                            a[t] = *reinterpret_cast<const d4_t*>(
                                cent + ((((t0 + t) * NDCH + dc) * 2 + u) * 4 + g) * 64 + m * 4);
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int t = 0; t < TI; ++t) acc[t0 + t] = mf64(a[t][s], xb[dc][u][s], acc[t0 + t]);
                        }
                    }
                }
            }
            // tiles in ascending order; j, tin and the branches are uniform over the workgroup
#pragma unroll
            for (int t = 0; t < GT; ++t) {
                if (j < k) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) qs += acc[t][q] * acc[t][q];
                    if (++tin == tpc) {
                        const double lp = cst[j] - 0.5 * group_sum(qs);
                        if (lp > best) {
                            best = lp;
                            besti = j;
                        }
                        if (rrow != nullptr && row_ok && (j & 3) == g) rrow[j] = lp;
                        qs = 0.0;
                        tin = 0;
                        ++j;
                    }
                }
            }
        }
        if (arg_out != nullptr && g == 0 && row_ok) arg_out[row] = besti;
        if (R != nullptr) {
            // lane group g owns the components j = g (mod 4): it wrote their lp and alone reads them back
            double se = 0.0;
            if (row_ok)
                for (int c = g; c < k; c += 4) se += exp(rrow[c] - best);
            se = group_sum(se);
            const double lse = row_ok ? best + log(se) : 0.0;
            if (row_ok)
                for (int c = g; c < k; c += 4) rrow[c] = exp(rrow[c] - lse);
            // the batch's sum of lse: the wave's 16 rows by a fixed butterfly, the waves in order
            double v = g == 0 ? lse : 0.0;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
            // the one barrier every batch has: a wave can be at most one batch ahead of thread 0's reads, so two
            // slots by batch parity are enough whether or not the staging barriers above are taken
            double* ws = wsum[((b - (int64_t)blockIdx.x) / gridDim.x) & 1];
            if (lane == 0) ws[wave] = v;
            __syncthreads();
            if (tid == 0) part[b] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
        }
    }
}

// out[0] = the sum of part [nb] by a rule that depends on nb alone
__global__ __launch_bounds__(EM_RED) void gmm_em_ll_kernel(const double* __restrict__ part, int64_t nb,
                                                           double* __restrict__ out) {
    __shared__ double sh[EM_RED];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += EM_RED) a += part[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = EM_RED / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// One unit: rows [r0, r1) of the components j0 .. j0 + JB - 1 (those below k), tile row ta, tiles
// tb = tb0 .. tb0 + NTB - 1 (tb0 >= ta).  The JB components share every load of X; only r differs.  pc: the chunk's
// partials [k][d d | d | 1]; the unit with tb0 == ta also writes the tile row's part of xs (and rs).
template <int NTB, int JB>
__device__ __forceinline__ void em_unit(const double* __restrict__ X, const double* __restrict__ R, int d, int k,
                                        int64_t r0, int64_t r1, int j0, int ta, int tb0, double* __restrict__ pc) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, g = lane >> 4;
    const int ca = 16 * ta + m;
    const int cb = 16 * tb0 + m;
    const bool aok = ca < d;
    const int nj = k - j0 < JB ? k - j0 : JB;
    d4_t acc[JB][NTB];
    double sx[JB], sr[JB];
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
        sx[jj] = 0.0;
        sr[jj] = 0.0;
#pragma unroll
        for (int t = 0; t < NTB; ++t) acc[jj][t] = d4_t{0.0, 0.0, 0.0, 0.0};
    }
    bool cok[NTB];
#pragma unroll
    for (int t = 0; t < NTB; ++t) cok[t] = cb + 16 * t < d;
    // whole blocks of 16 rows: every load is issued before the first product, rows in the same ascending order as
    // the tail loop below (four at a time, lane group g the row i0 + 4 s + g)
    int64_t i0 = r0;
    for (; i0 + 16 <= r1; i0 += 16) {
        double r[4][JB], xa[4], xv[4][NTB];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t i = i0 + 4 * s + g;
            const double* __restrict__ rr = R + i * (int64_t)k + j0;
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) r[s][jj] = jj < nj ? rr[jj] : 0.0;
            const double* __restrict__ xr = X + i * (int64_t)d;
            xa[s] = aok ? xr[ca] : 0.0;
#pragma unroll
            for (int t = 0; t < NTB; ++t) xv[s][t] = cok[t] ? xr[cb + 16 * t] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) {
                const double a = r[s][jj] * xa[s];
                sx[jj] += a;
                sr[jj] += r[s][jj];
#pragma unroll
                for (int t = 0; t < NTB; ++t) acc[jj][t] = mf64(a, xv[s][t], acc[jj][t]);
            }
        }
    }
    for (; i0 < r1; i0 += 4) {
        const int64_t i = i0 + g;
        const bool ok = i < r1;
        const double* __restrict__ rr = R + (ok ? i : r0) * (int64_t)k + j0;
        const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)d;
        const double xa = (ok && aok) ? xr[ca] : 0.0;
        double xv[NTB];
#pragma unroll
        for (int t = 0; t < NTB; ++t) xv[t] = (ok && cok[t]) ? xr[cb + 16 * t] : 0.0;
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const double r = (ok && jj < nj) ? rr[jj] : 0.0;
            const double a = r * xa;
            sx[jj] += a;
            sr[jj] += r;
#pragma unroll
            for (int t = 0; t < NTB; ++t) acc[jj][t] = mf64(a, xv[t], acc[jj][t]);
        }
    }
    const int64_t S = (int64_t)d * d + d + 1;
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
        if (jj >= nj) continue;
        double* __restrict__ out = pc + (int64_t)(j0 + jj) * S;
        // acc[jj][t][q] = xxs[16 ta + g + 4 q][16 (tb0 + t) + m]
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra = 16 * ta + g + 4 * q;
                if (ra < d && cok[t]) out[(int64_t)ra * d + cb + 16 * t] = acc[jj][t][q];
            }
        }
        if (tb0 == ta) {
            const double tx = group_sum(sx[jj]);
            const double tr = group_sum(sr[jj]);
            if (g == 0 && aok) out[(int64_t)d * d + ca] = tx;
            if (ta == 0 && lane == 0) out[(int64_t)d * d + d] = tr;
        }
    }
}

constexpr int EM_TB = 4;        // tiles of one unit at most: a wider tile row is split into blocks of EM_TB tiles

// units of one (chunk, component group): sum over ta of ceil((dt - ta) / EM_TB)
__host__ __device__ inline int em_units_per_group(int dt) {
    int u = 0;
    for (int ta = 0; ta < dt; ++ta) u += (dt - ta + EM_TB - 1) / EM_TB;
    return u;
}

// components per unit: 8 accumulator tiles at most
constexpr int em_group_components(int maxtb) { return maxtb <= 2 ? 4 : 2; }

// MAXTB = min(ceil(d / 16), EM_TB): a narrow d compiles (and pays the registers of) its own tile counts only
template <int MAXTB>
__global__ __launch_bounds__(64 * EM_M_WAVES) void gmm_em_moments_kernel(
        const double* __restrict__ X, const double* __restrict__ R, int64_t n, int d, int k, int64_t chunk_rows,
        int64_t nchunk, double* __restrict__ part) {
    constexpr int JB = em_group_components(MAXTB);
    const int dt = (d + 15) / 16;
    const int upg = em_units_per_group(dt);
    const int ng = (k + JB - 1) / JB;
    const int64_t S = (int64_t)d * d + d + 1;
    const int64_t units = nchunk * ng * upg;
    const int64_t w0 = (int64_t)blockIdx.x * EM_M_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * EM_M_WAVES;
    for (int64_t un = w0; un < units; un += nw) {
        const int64_t c = un / ((int64_t)ng * upg);
        const int rem = (int)(un - c * (int64_t)ng * upg);
        const int jg = rem / upg;
        int v = rem - jg * upg;         // the unit's place in the group's list: tile rows, then their blocks
        int ta = 0;
        for (;; ++ta) {
            const int nb = (dt - ta + EM_TB - 1) / EM_TB;
            if (v < nb) break;
            v -= nb;
        }
        const int tb0 = ta + v * EM_TB;
        const int ntb = dt - tb0 < EM_TB ? dt - tb0 : EM_TB;
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        double* __restrict__ pc = part + c * k * S;
        if (MAXTB >= 4 && ntb == 4) em_unit<4, JB>(X, R, d, k, r0, r1, jg * JB, ta, tb0, pc);
        else if (MAXTB >= 3 && ntb == 3) em_unit<3, JB>(X, R, d, k, r0, r1, jg * JB, ta, tb0, pc);
        else if (MAXTB >= 2 && ntb == 2) em_unit<2, JB>(X, R, d, k, r0, r1, jg * JB, ta, tb0, pc);
        else em_unit<1, JB>(X, R, d, k, r0, r1, jg * JB, ta, tb0, pc);
    }
}

// out = [rs k | xs k d | xxs k d d]: every element the sum of its chunk partials in chunk order
__global__ __launch_bounds__(256) void gmm_em_merge_kernel(int k, int d, int64_t nchunk,
                                                           const double* __restrict__ part,
                                                           double* __restrict__ out) {
    const int64_t S = (int64_t)d * d + d + 1;
    const int64_t total = (int64_t)k * S;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int j;
        int64_t off;
        if (e < k) {
            j = (int)e;
            off = (int64_t)d * d + d;
        } else if (e < (int64_t)k + (int64_t)k * d) {
            const int64_t f = e - k;
            j = (int)(f / d);
            off = (int64_t)d * d + (f - (int64_t)j * d);
        } else {
            const int64_t f = e - k - (int64_t)k * d;
            j = (int)(f / ((int64_t)d * d));
            const int ab = (int)(f - (int64_t)j * d * d);
            const int a = ab / d, b2 = ab - a * d;
            off = a <= b2 ? (int64_t)a * d + b2 : (int64_t)b2 * d + a;
        }
        double s = part[(int64_t)j * S + off];
        for (int64_t c = 1; c < nchunk; ++c) s += part[(c * k + j) * S + off];
        out[e] = s;
    }
}

}  // namespace

extern "C" {

// The E pass over the n fp64 rows X [n, d] (1 <= d <= 128).  img / ninit: the lane-ordered image of the
// [k tpc 16, d] column matrix and the accumulator start -C (``ops/gmm._em_image``), padded with zero tiles to
// ngroup groups of GT tiles (GT = 8, 4, 2, 2 for ceil(d / 32) = 1, 2, 3, 4); tpc = ceil(d / 16) tiles per component.
// R [n, k] (the responsibilities), arg int32 [n] (the argmax) may each be null; with R, part [ceil(n / 64)] is
// scratch and ll [1] receives sum_i lse_i.
int alink_gmm_em_rows_f64(const double* X, int64_t n, int d, const double* img, const double* ninit,
                          const double* cst, int k, int tpc, int ngroup, double* R, int* arg, double* part, double* ll,
                          int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 128 || k < 1 || n >= (1ll << 31) || tpc != (d + 15) / 16) return 1;
    const int ndch = (d + 31) / 32;
    if (ngroup < 1 || (int64_t)ngroup * em_group_tiles(ndch) < (int64_t)k * tpc) return 1;
    if (R != nullptr && (part == nullptr || ll == nullptr)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    ALINK_D64_LAUNCH(gmm_em_rows_kernel, ndch, 1, 2, 3, 4, vec_ok(d, X), row_blocks(n, grid, 2048), st, X, n, d, img,
                     ninit, cst, k, tpc, ngroup, R, arg, part);
    if (R != nullptr) hipLaunchKernelGGL(gmm_em_ll_kernel, dim3(1), dim3(EM_RED), 0, st, part, nbatch, ll);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The M pass: out [k (1 + d + d d)] = [rs | xs | xxs] of X [n, d] under R [n, k], through nchunk =
// ceil(n / chunk_rows) row chunks whose partials part [nchunk, k, d d + d + 1] are merged in chunk order.
int alink_gmm_em_moments_f64(const double* X, const double* R, int64_t n, int d, int k, int64_t chunk_rows,
                             int64_t nchunk, double* part, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 128 || k < 1 || n >= (1ll << 31) || chunk_rows < 1) return 1;
    if (nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int dt = (d + 15) / 16;
    const int64_t cap = grid > 0 ? grid : 16384;
    const int maxtb = dt < EM_TB ? dt : EM_TB;
    const int64_t groups = (k + em_group_components(maxtb) - 1) / em_group_components(maxtb);
    int64_t blocks = (nchunk * groups * em_units_per_group(dt) + EM_M_WAVES - 1) / EM_M_WAVES;
    if (blocks > cap) blocks = cap;
#define ALINK_EM_MOMENTS(MAXTB)                                                                                    \
    hipLaunchKernelGGL(gmm_em_moments_kernel<MAXTB>, dim3((unsigned)blocks), dim3(64 * EM_M_WAVES), 0, st, X, R,   \
                       n, d, k, chunk_rows, nchunk, part)
    if (dt == 1) ALINK_EM_MOMENTS(1);
    else if (dt == 2) ALINK_EM_MOMENTS(2);
    else if (dt == 3) ALINK_EM_MOMENTS(3);
    else ALINK_EM_MOMENTS(4);
#undef ALINK_EM_MOMENTS
    int64_t mblocks = ((int64_t)k * ((int64_t)d * d + d + 1) + 255) / 256;
    if (mblocks > cap) mblocks = cap;
    hipLaunchKernelGGL(gmm_em_merge_kernel, dim3((unsigned)mblocks), dim3(256), 0, st, k, d, nchunk, part, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
