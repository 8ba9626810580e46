// Newton's method for the linear family on gfx950 / MI355X: the fused Hessian, gradient and loss pass of
// OptimObjFunc.calc_hessian_gradient_loss (models/linear/objfunc.py), for contiguous fp64 rows X [n, k] with
// 1 <= k <= 128 (ops/newton.py).
//
// alink_newton_unary_f64: one read of X gives
//     [ sum w | sum l | s2 | s3 | g (k) | H (k x k) ],   H = sum_i hc_i x_i x_i^T,   g = sum_i gc_i x_i,
// with eta_i = x_i . coef and, for the unary losses (codes 0..8, those of ops/linear.loss_code),
//     hc = l''(eta, y) w,   gc = w l'(eta, y),   the loss sum unweighted (as calc_hessian_gradient_loss has it),
// and for AFT (code 9; coef [k + 1], log sigma = coef[k], w the censor indicator), eps = (y - eta) / sigma,
//     hc = exp(eps) / sigma^2,   gc = (w - exp(eps)) / sigma,   l = w (log sigma - eps) + exp(eps),   sum w = the rows,
//     s2 = sum (w + (w - exp(eps)) eps),   s3 = sum eps (exp(eps) (1 + eps) - w)
// (the corner entries of g and H, which the host adds; s2 = s3 = 0 for the unary losses).  The sums stand in front of
// g and H, here and in the softmax pass, because the merge takes its leading entries as a head before the matrix.
// A workgroup of 4 waves owns one row chunk and walks it 64 rows at a time:
//   load    four lanes per row read it from HBM once (row_dot of gram64_mfma.h: 16-byte loads where k is even and X
//           aligned, scalar loads otherwise, nothing outside the row), dot it with coef (LDS) by fma in a fixed order
//           and stage it in LDS at the stride of GramTiles; the columns behind k are zero.
//   loss    lane sub = 0 of a row evaluates l, l' and l'' (a wave-uniform switch on the loss code) with every cut-off
//           and clamp of the torch classes in objfunc.py, and writes hc, gc and the row's four sum terms beside the
//           rows.
//   Gram    after one barrier, the weighted upper tile triangle of gram64_mfma.h with ww = hc, and behind it the NT
//           scalar-operand tiles with A = gc, whose result row 0 is g: at most 44 accumulator tiles (NT = 8), 11 per
//           wave, in registers for the whole chunk.  Wave 0 adds the four sum terms, the rows by xor steps, the batches
//           in order.
//   merge   part [nchunk, 4 + k + k k] holds each chunk's sums, g and the entries of its upper tiles, merged in chunk
//           order with the mirror map of ordered_sum.h: no float atomics, the same bits for every grid and run.  A
//           loss with l'' = 0 (hinge, perceptron, SVR) gives ww = 0 and H = 0 exactly.
//
// All arithmetic is fp64 and follows the torch formulas operation for operation (no contraction: the only fused
// operations are the explicit fma of the dot and the matrix instruction).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gram64_mfma.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using d64::d2_t;
using d64::d4_t;

constexpr int NW_KMAX = 128;
constexpr int NW_SUMS = 4;      // leading entries of a partial: sum w, sum l, s2, s3
constexpr double LN2 = 0.6931471805599453;      // math.log(2.0)
enum { LOG = 0, LOGISTIC, SQUARE, HINGE, SMOOTH_HINGE, PERCEPTRON, EXPONENTIAL, HUBER, SVR, AFT };

// one row's terms: the Gram weight, the gradient scalar and the four sum terms
struct RowTerms {
    double hc, gc, s[NW_SUMS];
};

// l, l' and l'' of the unary loss `code` at (eta, y); p is Huber's delta or SVR's epsilon.  The comparisons are written
// so that each takes the branch torch.where / clamp takes.
__device__ __forceinline__ void unary_loss(int code, double p, double eta, double y, double& l, double& d1,
                                           double& d2) {
    switch (code) {
        case LOG:
        case LOGISTIC: {
            const double d = eta * y;
            const double mid = d < -37.0 ? -d : (d > 34.0 ? 0.0 : log1p(exp(-d)));
            const double t = y / (1.0 + exp(d > 700.0 ? 700.0 : d));
            d2 = t * (y - t);
            if (code == LOG) {
                l = mid;
                d1 = d < -37.0 ? -y : (d > 34.0 ? 0.0 : -y / (exp(d) + 1.0));
            } else {
                l = mid / LN2;
                d1 = d < -37.0 ? -y / LN2 : -y / (exp(d > 700.0 ? 700.0 : d) + 1.0) / LN2;
                d2 = d2 / LN2;
            }
            break;
        }
        case SQUARE: {
            const double x = eta - y;
            l = 0.5 * (x * x);
            d1 = x;
            d2 = 1.0;
            break;
        }
        case HINGE: {
            const double d = eta * y, v = 1.0 - d;
            l = v < 0.0 ? 0.0 : v;
            d1 = d < 1.0 ? -y : 0.0;
            d2 = 0.0;
            break;
        }
        case SMOOTH_HINGE: {
            const double d = eta * y, u = 1.0 - d;
            l = d <= 0.0 ? 0.5 - d : (d >= 1.0 ? 0.0 : 0.5 * (u * u));
            d1 = d <= 0.0 ? -y : (d >= 1.0 ? 0.0 : u * (-y));
            d2 = (d >= 1.0 || d <= 0.0) ? 0.0 : y * y;
            break;
        }
        case PERCEPTRON: {
            const double v = (-eta) * y;
            l = v < 0.0 ? 0.0 : v;
            d1 = eta * y < 0.0 ? -y : 0.0;
            d2 = 0.0;
            break;
        }
        case EXPONENTIAL: {
            const double e = exp((-eta) * y);
            l = e;
            d1 = (-y) * e;
            d2 = (y * y) * e;
            break;
        }
        case HUBER: {
            const double x = eta - y, ax = fabs(x);
            l = ax > p ? p * (ax - p / 2.0) : (ax * ax) / 2.0;
            d1 = ax > p ? (x > 0.0 ? p : -p) : x;
            d2 = ax > p ? 0.0 : 1.0;
            break;
        }
        default: {      // SVR
            const double x = eta - y, v = fabs(x) - p;
            l = v < 0.0 ? 0.0 : v;
            d1 = fabs(x) > p ? (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0)) : 0.0;
            d2 = 0.0;
            break;
        }
    }
}

__device__ __forceinline__ RowTerms row_terms(int code, double p, double eta, double y, double w) {
    RowTerms r;
    if (code == AFT) {          // p = log sigma
        const double sigma = exp(p);
        const double eps = (y - eta) / sigma;
        const double ee = exp(eps), mult = w - ee;
        r.hc = ee / (sigma * sigma);
        r.gc = mult / sigma;
        r.s[0] = 1.0;
        r.s[1] = w * (p - eps) + ee;
        r.s[2] = w + mult * eps;
        r.s[3] = eps * (ee * (1.0 + eps) - w);
    } else {
        double l, d1, d2;
        unary_loss(code, p, eta, y, l, d1, d2);
        r.hc = d2 * w;
        r.gc = w * d1;
        r.s[0] = w;
        r.s[1] = l;
        r.s[2] = 0.0;
        r.s[3] = 0.0;
    }
    return r;
}

// pc = the chunk's [sums (4) | g [k] | H [k, k]]: acc[s][q] = H[16 ta + g + 4 q][16 tb + m] of an upper tile, and
// result row 0 (g = 0, q = 0) of scalar tile tb = g[16 tb + m]
template <int NT>
struct NewtonStore {
    using G = d64::GramTiles<NT, true, d64::SCALAR>;
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[G::MAXT], double* __restrict__ pc, int k, int g,
                                                 int m) {
        if constexpr (s < G::MAXT) {
            constexpr int t = G::tile(WAVE, s);
            if constexpr (t < G::TU) {
                constexpr int ta = d64::tile_a(NT, t), tb = d64::tile_b(NT, t);
                const int cb = 16 * tb + m;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ra = 16 * ta + g + 4 * q;
                    if (ra < k && cb < k) pc[NW_SUMS + k + (int64_t)ra * k + cb] = acc[s][q];
                }
            } else if constexpr (t < G::T) {
                const int cb = 16 * (t - G::TU) + m;
                if (g == 0 && cb < k) pc[NW_SUMS + cb] = acc[s][0];
            }
            store<WAVE, s + 1>(acc, pc, k, g, m);
        }
    }
};

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void newton_unary_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
        const double* __restrict__ coef, int64_t n, int k, int code, double param, int64_t chunk_rows, int64_t nchunk,
        double* __restrict__ part) {
    using G = d64::GramTiles<NT, true, d64::SCALAR>;
    constexpr int S = G::S;
    __shared__ __attribute__((aligned(16))) double rows[64 * S];
    __shared__ __attribute__((aligned(16))) double bet[128];
    __shared__ double wws[128];             // the rows' hc, then their gc
    __shared__ double terms[NW_SUMS][64];
    __shared__ __attribute__((aligned(32))) double red[G::RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid >> 2, sub = tid & 3;
    const int m = lane & 15, g = lane >> 4;
    const int64_t P = NW_SUMS + k + (int64_t)k * k;
    if (code == AFT) param = coef[k];       // log sigma, the entry behind the k coefficients of the rows
    d64::stage_beta(bet, coef, k);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        d4_t acc[G::MAXT];
#pragma unroll
        for (int s = 0; s < G::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        double sums[NW_SUMS] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + r;
            const bool ok = i < r1;
            d2_t v[2 * NT];
            const double dot = d64::row_dot<NT, VEC>(X + (ok ? i : r0) * (int64_t)k, ok, k, sub, bet, v);
            double* __restrict__ slot = rows + r * S;
#pragma unroll
            for (int j = 0; j < 2 * NT; ++j) *reinterpret_cast<d2_t*>(slot + 8 * j + 2 * sub) = v[j];
            if (sub == 0) {
                RowTerms t = {0.0, 0.0, {0.0, 0.0, 0.0, 0.0}};
                if (ok) t = row_terms(code, param, dot, y[i], w[i]);
                wws[r] = t.hc;
                wws[64 + r] = t.gc;
#pragma unroll
                for (int q = 0; q < NW_SUMS; ++q) terms[q][r] = t.s[q];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int q = 0; q < NW_SUMS; ++q) sums[q] += osum::wave_sum_desc(terms[q][lane]);
            }
            G::batch(acc, rows, wws, wave, g, m);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < NW_SUMS; ++q) pc[q] = sums[q];
        }
        G::template finish<NewtonStore<NT>>(acc, red, wave, lane, pc, k, g, m);
    }
}

// ---- the softmax pass ----
//
// alink_newton_softmax_f64: X [n, m] (1 <= m <= 128), coefficients W [k1, m] as the tile-outermost image of
// softmax_fused.hip (pivot class k1 with logit 0, 1 <= k1 <= 64, k1 m <= 1024), class indices y, weights w.  With
// D = k1 m it gives [ sum w | sum l | G (k1 x m) | H (D x D) ] in the [k][featDim] layout of SoftmaxObjFunc,
//     H[(s,.),(t,.)] = sum_i w_i (delta_st phi_is - phi_is phi_it) x_i x_i^T,
//     G[s] = sum_i w_i (phi_is - [y_i = s]) x_i,
// the loss sum unweighted.  Every block (s, t) is a weighted Gram of the same rows, so only the class pairs s <= t and
// in each only the upper tile triangle are computed.  A unit of work is (row chunk, group of PG class pairs in the
// order s ascending, then t); PG follows from NT alone (pair_group: at most 12 accumulator tiles per wave and 44 per
// unit).  A unit walks its chunk 64 rows at a time:
//   logits  as softmax_fused.hip: lane (mm, g) of a wave holds its row's dims in registers, the image is read through
//           the caches, the logits of all classes on the matrix cores; the row goes to LDS at the stride of GramTiles.
//   softmax the pivot softmax in registers (row_lse of dense64_mfma.h); phi [64, 16 T], w, y and the loss to LDS.
//   pairs   one wave per pair of the group writes ww = w (delta phi_s - phi_s phi_t) and, for a diagonal pair (s, s),
//           the scalar sc = w (phi_s - [y = s]) (0 otherwise) beside the rows; then each pair runs the tile deal of
//           gram64_mfma.h into accumulators of its own.  The scalar-operand tiles of a diagonal pair give G[s]; the
//           unit that holds pair (0, 0) adds the two sums.  Every element comes from exactly one unit.
//   merge   the chunk partials are merged in chunk order (ordered_sum.h) with the map SoftmaxMirror: an element of
//           the output reads block (min(s, t), max(s, t)) at (min(a, b), max(a, b)): the transposed blocks and the
//           mirror inside a block in one rule, so H is exactly symmetric.  No [n, k1] block is written to memory.
// The logits of a unit's batch are recomputed by every pair group: T MT of the unit's T MT + PG (TU + NT) matrix
// instructions per 16 rows and wave (profiles/newton.txt has the share at the measured shapes).

constexpr int SM_KMAX = 64, SM_DMAX = 1024;

// class pairs per unit for NT dim tiles
constexpr int pair_group(int nt) {
    const int tiles = nt * (nt + 1) / 2 + nt, maxt = nt <= 2 ? tiles : (tiles + 3) / 4;
    const int by_wave = 12 / maxt, by_unit = 44 / tiles;
    const int pg = by_wave < by_unit ? by_wave : by_unit;
    return pg < 1 ? 1 : pg;
}

// block (s, t) of the chunk's [sums (2) | G | H]: the upper tiles into H, row 0 of the scalar tiles of a diagonal
// pair into G[s]
template <int NT>
struct SoftmaxStore {
    using G = d64::GramTiles<NT, true, d64::SCALAR>;
    template <int WAVE, int i = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[G::MAXT], double* __restrict__ pc, int m, int64_t D,
                                                 int s, int t, int g, int mm) {
        if constexpr (i < G::MAXT) {
            constexpr int tl = G::tile(WAVE, i);
            if constexpr (tl < G::TU) {
                constexpr int ta = d64::tile_a(NT, tl), tb = d64::tile_b(NT, tl);
                const int cb = 16 * tb + mm;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ra = 16 * ta + g + 4 * q;
                    if (ra < m && cb < m) pc[2 + D + ((int64_t)s * m + ra) * D + (int64_t)t * m + cb] = acc[i][q];
                }
            } else if constexpr (tl < G::T) {
                const int cb = 16 * (tl - G::TU) + mm;
                if (s == t && g == 0 && cb < m) pc[2 + (int64_t)s * m + cb] = acc[i][0];
            }
            store<WAVE, i + 1>(acc, pc, m, D, s, t, g, mm);
        }
    }
};

template <int T, int NT, bool VEC>
__global__ __launch_bounds__(256) void newton_softmax_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w, int64_t n, int m,
        int k1, const double* __restrict__ img, int64_t chunk_rows, int64_t nchunk, int ngroup,
        double* __restrict__ part) {
    using G = d64::GramTiles<NT, true, d64::SCALAR>;
    constexpr int PG = pair_group(NT), NDCH = (NT + 1) / 2, S = G::S, SP = 16 * T;
    __shared__ __attribute__((aligned(32))) double rows[64 * S];
    __shared__ double phi[64 * SP];
    __shared__ double wws[PG][128];         // per pair: the rows' ww, then their sc
    __shared__ double wl[64], ll[64];
    __shared__ int yl[64];
    __shared__ __attribute__((aligned(32))) double red[G::RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mm = lane & 15, g = lane >> 4;
    const int lr = wave * 16 + mm;          // the lane's row of a batch
    const int64_t D = (int64_t)k1 * m, P = 2 + D + D * D;
    const int npair = k1 * (k1 + 1) / 2;
    for (int64_t unit = blockIdx.x; unit < nchunk * ngroup; unit += gridDim.x) {
        const int64_t c = unit / ngroup;
        const int grp = (int)(unit - c * ngroup);
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        int ps[PG], pt[PG];                 // the classes of the unit's pairs; ps = -1 behind the last pair
#pragma unroll
        for (int j = 0; j < PG; ++j) {
            int p = grp * PG + j, s = 0;
            if (p < npair) {
                while (p >= k1 - s) {
                    p -= k1 - s;
                    ++s;
                }
                ps[j] = s;
                pt[j] = s + p;
            } else {
                ps[j] = -1;
                pt[j] = -1;
            }
        }
        d4_t acc[PG][G::MAXT];
#pragma unroll
        for (int j = 0; j < PG; ++j) {
#pragma unroll
            for (int i = 0; i < G::MAXT; ++i) acc[j][i] = d4_t{0.0, 0.0, 0.0, 0.0};
        }
        double sums[2] = {0.0, 0.0};
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + lr;
            const bool ok = i < r1;
            const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)m;
            double xb[NDCH][2][4];
#pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) d64::load_chunk<VEC>(xb[dc], xr, ok, dc, g, m);
            const double wi = ok ? w[i] : 0.0;
            const int yi = ok ? (int)y[i] : k1;
            d4_t e[T];
#pragma unroll
            for (int t = 0; t < T; ++t) e[t] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (2 * dc + u >= NT) continue;         // no dim tile there
                    d4_t a[T];
#pragma unroll
                    for (int t = 0; t < T; ++t)
                        a[t] = *reinterpret_cast<const d4_t*>(
                            img + ((((t * NDCH + dc) * 2 + u) * 4 + g) * 16 + mm) * 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma unroll
                        for (int t = 0; t < T; ++t) e[t] = d64::mf64(a[t][q], xb[dc][u][q], e[t]);
                    }
                    *reinterpret_cast<d4_t*>(rows + lr * S + 16 * (2 * dc + u) + 4 * g) =
                        d4_t{xb[dc][u][0], xb[dc][u][1], xb[dc][u][2], xb[dc][u][3]};
                }
            }
            const double lse = d64::row_lse<T>(e, k1, g);
            double ey = 0.0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cls = 16 * t + g + 4 * q;
                    phi[lr * SP + cls] = cls < k1 ? exp(e[t][q] - lse) : 0.0;
                    if (cls < k1 && cls == yi) ey = e[t][q];
                }
            }
            ey = d64::group_sum(ey);
            if (g == 0) {
                wl[lr] = wi;
                ll[lr] = ok ? lse - ey : 0.0;
                yl[lr] = yi;
            }
            __syncthreads();
            for (int j = wave; j < PG; j += 4) {            // one wave per pair, one lane per row
                const int s = ps[j], t = pt[j];
                double ww = 0.0, sc = 0.0;
                if (s >= 0) {
                    const double a = phi[lane * SP + s], b = phi[lane * SP + t], wr = wl[lane];
                    if (s == t) {
                        ww = (a - a * a) * wr;
                        sc = (yl[lane] == s ? a - 1.0 : a) * wr;
                    } else {
                        ww = (-(a * b)) * wr;
                    }
                }
                wws[j][lane] = ww;
                wws[j][64 + lane] = sc;
            }
            if (wave == 0 && grp == 0) {
                sums[0] += osum::wave_sum_desc(wl[lane]);
                sums[1] += osum::wave_sum_desc(ll[lane]);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PG; ++j)
                if (ps[j] >= 0) G::batch(acc[j], rows, wws[j], wave, g, mm);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        if (grp == 0 && tid == 0) {
            pc[0] = sums[0];
            pc[1] = sums[1];
        }
#pragma unroll
        for (int j = 0; j < PG; ++j)
            if (ps[j] >= 0)
                G::template finish<SoftmaxStore<NT>>(acc[j], red, wave, lane, pc, m, D, ps[j], pt[j], g, mm);
    }
}

// the merge's map for [sums (2) | G [D] | H [D, D]]: element [(s, a), (t, b)] of H reads block (min(s, t), max(s, t))
// at (min(a, b), max(a, b))
struct SoftmaxMirror {
    int m;
    int64_t D;
    __device__ int64_t operator()(int64_t e) const {
        if (e < 2 + D) return e;
        const int64_t A = (e - 2 - D) / D, B = (e - 2 - D) - A * D;
        const int s = (int)(A / m), a = (int)(A - (int64_t)s * m), t = (int)(B / m), b = (int)(B - (int64_t)t * m);
        const int s0 = s < t ? s : t, t0 = s < t ? t : s, a0 = a < b ? a : b, b0 = a < b ? b : a;
        return 2 + D + ((int64_t)s0 * m + a0) * D + (int64_t)t0 * m + b0;
    }
};

template <int T, bool VEC, class... Args>
void launch_softmax(int nt, unsigned blocks, hipStream_t st, Args... a) {
#define ALINK_NW_SM(NT) hipLaunchKernelGGL((newton_softmax_kernel<T, NT, VEC>), dim3(blocks), dim3(256), 0, st, a...)
    if constexpr (T == 1) {
        switch (nt) {
            case 1: ALINK_NW_SM(1); break;
            case 2: ALINK_NW_SM(2); break;
            case 3: ALINK_NW_SM(3); break;
            case 4: ALINK_NW_SM(4); break;
            case 5: ALINK_NW_SM(5); break;
            case 6: ALINK_NW_SM(6); break;
            case 7: ALINK_NW_SM(7); break;
            default: ALINK_NW_SM(8); break;
        }
    } else if constexpr (T == 2) {          // k1 >= 17: m <= 60
        switch (nt) {
            case 1: ALINK_NW_SM(1); break;
            case 2: ALINK_NW_SM(2); break;
            case 3: ALINK_NW_SM(3); break;
            default: ALINK_NW_SM(4); break;
        }
    } else {                                // k1 >= 33: m <= 31
        if (nt == 1) ALINK_NW_SM(1);
        else ALINK_NW_SM(2);
    }
#undef ALINK_NW_SM
}

template <bool VEC, class... Args>
void launch_softmax_t(int t, int nt, unsigned blocks, hipStream_t st, Args... a) {
    switch (t) {
        case 1: launch_softmax<1, VEC>(nt, blocks, st, a...); break;
        case 2: launch_softmax<2, VEC>(nt, blocks, st, a...); break;
        case 3: launch_softmax<3, VEC>(nt, blocks, st, a...); break;
        default: launch_softmax<4, VEC>(nt, blocks, st, a...); break;
    }
}

}  // namespace

extern "C" {

// One Newton statistics pass over X [n, k] (1 <= k <= 128), y, w [n] at coef [k] (code 9, AFT: coef [k + 1], the last
// entry log sigma): out [4 + k + k k] = [sum w | sum l | s2 | s3 | g | H] through nchunk = ceil(n / chunk_rows) row
// chunks (chunk_rows a multiple of 64) whose partials part [nchunk, 4 + k + k k] are merged in chunk order.  code: the
// loss codes 0..8 of ops/linear.loss_code with their parameter param, or 9.
int alink_newton_unary_f64(const double* X, const double* y, const double* w, const double* coef, int64_t n, int k,
                           int code, double param, int64_t chunk_rows, int64_t nchunk, double* part, double* out,
                           int grid, void* stream) {
    if (n <= 0) return 0;
    if (k < 1 || k > NW_KMAX || n >= (1ll << 31) || code < LOG || code > AFT) return 1;
    if (chunk_rows < 64 || chunk_rows % 64 != 0 || nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || coef == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nt = (k + 15) / 16;
    const unsigned blocks = (unsigned)(grid > 0 && grid < nchunk ? grid : nchunk);
    ALINK_D64_LAUNCH_NT8(newton_unary_kernel, nt, d64::vec_ok(k, X), blocks, st, X, y, w, coef, n, k, code, param,
                         chunk_rows, nchunk, part);
    osum::chunk_merge(osum::GramMirror{NW_SUMS + k, k}, NW_SUMS + k + (int64_t)k * k, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// One softmax Newton pass over X [n, m] (1 <= m <= 128), y, w [n] at the coefficients whose tile-outermost image is
// img [ceil(k1 / 16), ceil(m / 32), 2, 4, 16, 4] (1 <= k1 <= 64, D = k1 m <= 1024): out [2 + D + D D] =
// [sum w | sum l | G [k1, m] | H [D, D]] through nchunk = ceil(n / chunk_rows) row chunks (chunk_rows a multiple of
// 64) whose partials part [nchunk, 2 + D + D D] are merged in chunk order.
int alink_newton_softmax_f64(const double* X, const double* y, const double* w, int64_t n, int m, int k1,
                             const double* img, int64_t chunk_rows, int64_t nchunk, double* part, double* out,
                             int grid, void* stream) {
    if (n <= 0) return 0;
    if (m < 1 || m > NW_KMAX || k1 < 1 || k1 > SM_KMAX || k1 * m > SM_DMAX || n >= (1ll << 31)) return 1;
    if (chunk_rows < 64 || chunk_rows % 64 != 0 || nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || img == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int t = (k1 + 15) / 16, nt = (m + 15) / 16, pg = pair_group(nt);
    const int ngroup = (k1 * (k1 + 1) / 2 + pg - 1) / pg;
    const int64_t units = nchunk * ngroup, D = (int64_t)k1 * m, P = 2 + D + D * D;
    const unsigned blocks = (unsigned)(grid > 0 && grid < units ? grid : units);
    if (d64::vec_ok(m, X))
        launch_softmax_t<true>(t, nt, blocks, st, X, y, w, n, m, k1, img, chunk_rows, nchunk, ngroup, part);
    else
        launch_softmax_t<false>(t, nt, blocks, st, X, y, w, n, m, k1, img, chunk_rows, nchunk, ngroup, part);
    osum::chunk_merge(SoftmaxMirror{m, D}, P, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
