// Pearson chi-square independence tests of many feature columns against one label (``ops/chisq.py``).  A block of
// columns arrives as a sorted entry stream: entry e holds the running category index g[e] (ascending; a category is
// one distinct value of one column) and the label code lab[e] in [0, L) of its row.  The contingency counts are
// integers, so cnt is the same for every grid, chunk size and split into row blocks or ranks; the statistic is a
// sum of non-negative fp64 terms added in one fixed order per column.  Integer vector atomics only; the host oracle
// is ``models/statistics/summary.chi_square_test``.
//
// * alink_chisq_counts — cnt uint32 [G, L] += the entries.  Work is split by entries: a wave owns chunks of
//   ``chunk`` consecutive entries (chunk w, w + waves, ...), whatever columns and categories they fall in, so one
//   value that fills millions of entries and a column of all-distinct values both stay balanced.  Per step of 64
//   entries: when the whole step lies in one category the lanes add into the wave's private LDS histogram of L
//   counters (integer ds_add); the histogram is flushed by lanes over labels with global integer atomic adds of its
//   non-zero counters when the category changes and at the chunk's end.  A step that holds a category border adds
//   its entries straight into cnt with one global atomic each: short runs have nothing to gain from the histogram
//   and a flush per category would cost L / 64 passes each.  ``variant`` 1 takes the per-entry atomics for every
//   step (the measured comparison of ops/chisq.py).  An entry outside [0, G) x [0, L) is skipped and counted in
//   ``bad`` (the wrapper raises).
// * alink_chisq_stat — per column c with categories gptr[c] .. gptr[c + 1] of cnt (int64 after the ranks' sum), its
//   label totals cs [c, L] and an optional extra category zero [c, L] (the implicit zeros of CSR rows; it comes
//   last): rows of the cross table are the categories with a row sum rs > 0, columns the labels with cs > 0, and
//   every such cell adds E = rs * cs / n, t = O - E, t * t / E, each step one correctly rounded fp64 operation
//   (the *_rn intrinsics, so nothing is contracted or reordered).  W lanes own a category (W a power of two chosen from L
//   alone, lanes_for), lane s the labels s, s + W, ... in ascending order; a fixed xor butterfly adds the W lanes;
//   the categories of a unit of CQ_UNIT = 256 add in ascending order; a second kernel adds a column's unit
//   partials in unit order.  A wave owns a unit, so a column's value depends on the column alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int CQ_THREADS = 256;
constexpr int CQ_WAVES = CQ_THREADS / 64;
constexpr int CQ_LMAX = 1024;           // labels the histogram and a lane's registers hold
constexpr int CQ_UNIT = 256;            // categories whose terms one wave adds in order
constexpr int CQ_PER_LANE = CQ_LMAX / 64;

__global__ __launch_bounds__(CQ_THREADS) void chisq_counts_kernel(
        const int* __restrict__ g, const int* __restrict__ lab, int64_t E, int64_t G, int L, int64_t chunk,
        int variant, uint32_t* __restrict__ cnt, int* __restrict__ bad) {
    __shared__ uint32_t hist_all[CQ_WAVES][CQ_LMAX];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    uint32_t* hist = hist_all[wv];
    for (int l = lane; l < L; l += 64) hist[l] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const int64_t waves = (int64_t)gridDim.x * CQ_WAVES;
    const int64_t chunks = (E + chunk - 1) / chunk;
    for (int64_t ch = (int64_t)blockIdx.x * CQ_WAVES + wv; ch < chunks; ch += waves) {
        const int64_t lo = ch * chunk;
        const int64_t hi = lo + chunk < E ? lo + chunk : E;
        int64_t open = -1;                                  // the category the histogram holds, wave-uniform
        for (int64_t e0 = lo; e0 < hi; e0 += 64) {
            const int64_t e = e0 + lane;
            const bool in = e < hi;
            int64_t ge = in ? (int64_t)g[e] : -1;
            int le = in ? lab[e] : 0;
            const bool ok = in && ge >= 0 && ge < G && le >= 0 && le < L;
            if (in && !ok) atomicAdd(bad, 1);
            const int64_t last = e0 + 63 < hi ? e0 + 63 : hi - 1;
            const int64_t g_first = (int64_t)g[e0], g_last = (int64_t)g[last];      // wave-uniform loads
            const bool whole = variant == 0 && g_first == g_last && g_first >= 0 && g_first < G;
            if (open >= 0 && !(whole && g_first == open)) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                for (int l = lane; l < L; l += 64) {
                    const uint32_t v = hist[l];
                    if (v) {
                        atomicAdd(cnt + open * L + l, v);
                        hist[l] = 0;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                open = -1;
            }
            if (whole) {
                // ascending g and equal ends: every entry of the step has this category
                if (ok && ge == g_first) atomicAdd(hist + le, 1u);
                else if (ok) atomicAdd(cnt + ge * L + le, 1u);          // only if g does not ascend
                open = g_first;
            } else if (ok) {
                atomicAdd(cnt + ge * L + le, 1u);
            }
        }
        if (open >= 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            for (int l = lane; l < L; l += 64) {
                const uint32_t v = hist[l];
                if (v) {
                    atomicAdd(cnt + open * L + l, v);
                    hist[l] = 0;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
}

// lanes per category: the smallest power of two that covers L, at most a wave
inline int lanes_for(int L) {
    int w = 1;
    while (w < L && w < 64) w <<= 1;
    return w;
}

__device__ __forceinline__ double butterfly_f64(double a, int W) {
    for (int o = 1; o < W; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

__device__ __forceinline__ int64_t butterfly_i64(int64_t a, int W) {
    for (int o = 1; o < W; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// one correctly rounded operation per step, in this order; no contraction of t * t with anything
__device__ __forceinline__ double chisq_term(double o, double rs, double cs, double n) {
#pragma clang fp contract(off)
    const double ex = __dmul_rn(rs, cs);
    const double ee = __ddiv_rn(ex, n);
    const double t = __dsub_rn(o, ee);
    const double tt = __dmul_rn(t, t);
    return __ddiv_rn(tt, ee);
}

// a wave owns a unit: up to CQ_UNIT consecutive categories of one column (the zero row, when there is one, is the
// column's last category).  part[u]: the unit's sum of terms; rcat[u]: its categories with rs > 0.
__global__ __launch_bounds__(CQ_THREADS) void chisq_unit_kernel(
        const int64_t* __restrict__ cnt, const int64_t* __restrict__ gptr, const int64_t* __restrict__ cs,
        const int64_t* __restrict__ zero, const int* __restrict__ ucol, const int64_t* __restrict__ uptr,
        int64_t U, int L, int W, double* __restrict__ part, int* __restrict__ rcat) {
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int sub = lane & (W - 1);                         // the lane's place among the W lanes of its category
    const int grp = lane / W;                               // which of the 64 / W categories of a pass
    const int per = 64 / W;
    const int nq = (L + W - 1) / W;                         // labels per lane
    const int64_t waves = (int64_t)gridDim.x * CQ_WAVES;
    for (int64_t u = (int64_t)blockIdx.x * CQ_WAVES + wv; u < U; u += waves) {
        const int c = ucol[u];
        const int64_t g0 = gptr[c], ncat = gptr[c + 1] - g0;
        const int64_t total = ncat + (zero != nullptr ? 1 : 0);
        const int64_t k0 = (u - uptr[c]) * CQ_UNIT;
        const int64_t k1 = k0 + CQ_UNIT < total ? k0 + CQ_UNIT : total;
        const int64_t* csr = cs + (int64_t)c * L;
        // the lane's label totals, and n = their sum over all labels (every W-lane group holds all of them)
        double csd[CQ_PER_LANE];
        int64_t nloc = 0;
#pragma unroll
        for (int q = 0; q < CQ_PER_LANE; ++q) {
            const int l = sub + q * W;
            if (q >= nq) {
                csd[q] = 0.0;
                continue;
            }
            const int64_t v = l < L ? csr[l] : 0;
            csd[q] = (double)v;
            nloc += v;
        }
        const double n = (double)butterfly_i64(nloc, W);
        double acc = 0.0;
        int rc = 0;
        for (int64_t kb = k0; kb < k1; kb += per) {
            const int64_t k = kb + grp;
            const bool live = k < k1;
            const int64_t* row = !live ? nullptr : (k < ncat ? cnt + (g0 + k) * L : zero + (int64_t)c * L);
            int64_t o[CQ_PER_LANE];
            int64_t rloc = 0;
#pragma unroll
            for (int q = 0; q < CQ_PER_LANE; ++q) {
                const int l = sub + q * W;
                o[q] = (q < nq && live && l < L) ? row[l] : 0;
                rloc += o[q];
            }
            const int64_t rsi = butterfly_i64(rloc, W);
            const double rs = (double)rsi;
            double s = 0.0;
            if (rsi > 0) {
#pragma unroll
                for (int q = 0; q < CQ_PER_LANE; ++q)
                    if (q < nq && sub + q * W < L && csd[q] > 0.0) s += chisq_term((double)o[q], rs, csd[q], n);
            }
            s = butterfly_f64(s, W);
            // the pass's categories in ascending order; a category with rs == 0 adds nothing
            for (int j = 0; j < per; ++j) {
                const double sj = __shfl(s, j * W, 64);
                const int64_t rj = __shfl(rsi, j * W, 64);
                if (kb + j < k1 && rj > 0) {
                    acc += sj;
                    ++rc;
                }
            }
        }
        if (lane == 0) {
            part[u] = acc;
            rcat[u] = rc;
        }
    }
}

__global__ __launch_bounds__(CQ_THREADS) void chisq_merge_kernel(
        const double* __restrict__ part, const int* __restrict__ rcat, const int64_t* __restrict__ uptr,
        const int64_t* __restrict__ cs, int C, int L, double* __restrict__ value, int* __restrict__ R,
        int* __restrict__ Lc) {
    for (int c = blockIdx.x * CQ_THREADS + threadIdx.x; c < C; c += gridDim.x * CQ_THREADS) {
        double v = 0.0;
        int r = 0;
        for (int64_t u = uptr[c]; u < uptr[c + 1]; ++u) {
            v += part[u];
            r += rcat[u];
        }
        int lc = 0;
        for (int l = 0; l < L; ++l) lc += cs[(int64_t)c * L + l] > 0 ? 1 : 0;
        value[c] = v;
        R[c] = r;
        Lc[c] = lc;
    }
}

}  // namespace

extern "C" {

// cnt uint32 [G, L] += the stream's entries.  chunk: entries a wave owns at a time (0: 2048; rounded up to 64);
// grid: workgroups (0: chosen from E); variant 0: LDS histogram for whole-step runs, 1: per-entry global atomics.
int alink_chisq_counts(const int* g, const int* lab, int64_t E, int64_t G, int L, void* cnt, int* bad, int64_t chunk,
                       int grid, int variant, void* stream) {
    if (E < 0 || G < 1 || L < 1 || L > CQ_LMAX || chunk < 0 || grid < 0 || variant < 0 || variant > 1) return 1;
    if (E == 0) return 0;
    if (chunk == 0) chunk = 2048;
    chunk = (chunk + 63) / 64 * 64;
    const int64_t chunks = (E + chunk - 1) / chunk;
    int64_t blocks = (chunks + CQ_WAVES - 1) / CQ_WAVES;
    if (blocks > 8192) blocks = 8192;
    if (grid > 0) blocks = grid;
    hipLaunchKernelGGL(chisq_counts_kernel, dim3((unsigned)blocks), dim3(CQ_THREADS), 0, (hipStream_t)stream, g, lab,
                       E, G, L, chunk, variant, (uint32_t*)cnt, bad);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// value double [C], R int32 [C], Lc int32 [C] of C columns.  ucol int32 [U] / uptr int64 [C + 1]: the units (256
// categories each, the zero row included) and the columns they belong to; part double [U] and rcat int32 [U] are
// scratch.  zero may be null.
int alink_chisq_stat(const int64_t* cnt, const int64_t* gptr, const int64_t* cs, const int64_t* zero,
                     const int* ucol, const int64_t* uptr, int64_t U, int C, int L, double* part, int* rcat,
                     double* value, int* R, int* Lc, int grid, void* stream) {
    if (C < 0 || U < 0 || L < 1 || L > CQ_LMAX || grid < 0) return 1;
    if (C == 0) return 0;
    const int W = lanes_for(L);
    if (U > 0) {
        int64_t blocks = (U + CQ_WAVES - 1) / CQ_WAVES;
        if (blocks > 8192) blocks = 8192;
        if (grid > 0) blocks = grid;
        hipLaunchKernelGGL(chisq_unit_kernel, dim3((unsigned)blocks), dim3(CQ_THREADS), 0, (hipStream_t)stream, cnt,
                           gptr, cs, zero, ucol, uptr, U, L, W, part, rcat);
        if (hipGetLastError() != hipSuccess) return 2;
    }
    int mblocks = (C + CQ_THREADS - 1) / CQ_THREADS;
    if (mblocks > 4096) mblocks = 4096;
    hipLaunchKernelGGL(chisq_merge_kernel, dim3((unsigned)mblocks), dim3(CQ_THREADS), 0, (hipStream_t)stream, part,
                       rcat, uptr, cs, C, L, value, R, Lc);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // extern "C"
