// Multinomial (softmax) regression on gfx950 / MI355X: the fused gradient pass and the row pass of
// models/linear/objfunc.py SoftmaxObjFunc, for contiguous fp64 rows X [n, m], coefficients W [k1, m] (pivot class k1
// with logit 0, 1 <= k1 <= 64), fp64 class indices y in [0, k1] and weights w (ops/softmax_fused.py).  All arithmetic
// is fp64; no [n, k1] block of logits is ever written.
//
// alink_softmax_fused_grad_f64 (1 <= m <= 128): one read of X gives [sum w loss | G [k1, m]], G = sum_i r_i x_i^T.
// A workgroup of 4 waves owns one row chunk and walks it 64 rows at a time (T = ceil(k1 / 16) class tiles,
// MT = ceil(m / 16) dim tiles, NDCH = ceil(MT / 2) dim chunks of 32):
//   logits  the operand maps, load_chunk and mf64 of dense64_mfma.h: a wave owns 16 rows, lane (mm, g) its row mm's
//           dims 32 dc + 16 u + 4 g + s, which stay in registers.  The table is W as a tile-outermost image
//           [t][dc][u][g][mm][s] (the layout gmm_em.hip keeps), staged once per workgroup; the one shape whose image
//           (64 KiB) does not fit beside the batch, T = 4 with NDCH = 4, reads it through the caches.
//   softmax a lane holds the classes 16 t + g + 4 q of its own row: the maximum (pivot 0 included) over its own
//           accumulators first, across the four lane groups last; the exp terms in ascending class order per lane,
//           then group_sum, then the pivot's term; lse = max + log(sum), loss = lse - eta[y] (0 for the pivot),
//           r_c = w (exp(eta_c - lse) - [c == y]).  A padded class slot gives exactly 0 and never enters the maximum.
//   stage   the batch's r [64, 16 T] and x [64, 16 MT] go to LDS from the registers that hold them.  Rows are 16 T
//           and 16 MT doubles apart; where that count of tiles is even, a row's columns are xor-ed with 16 on odd
//           rows, so that rows of either parity start 32 banks apart in every case.
//   Gram    after one barrier G += r^T x on v_mfma_f64_16x16x4_f64, four rows per instruction: A[mm][g] =
//           r[i0 + g][16 tc + mm], B[g][mm] = x[i0 + g][16 td + mm], result slot q = G[16 tc + g + 4 q][16 td + mm].
//           The tiles t = tc MT + td are dealt to the waves by WaveDeal of gram64_mfma.h (at most 8 accumulator
//           tiles per wave), the split rule for fewer than 4 tiles: a rule of (k1, m) alone.
//   merge   part [nchunk, 1 + k1 m] holds each chunk's loss sum and G, merged in chunk order (ordered_sum.h): the
//           same bits for every grid and run.
//
// alink_softmax_fused_rows_f64 (1 <= m <= 1024): the chunk-walking tile loop of dense64_mfma.h (load_chunk, stage,
// mfma_group, the lane-ordered image of one block of NT tiles).  Plain: the table is W (TW = 1, 2 or 4 class tiles);
// by mask R [n, k1] is written and sum w loss returned.  Search: the table is [W ; D], both padded to TW tiles, so
// class tile t of W and of D land in the same lane slots (accumulators t and TW + t); a row evaluates
// w (lse(e_s) - e_s[y]) for e_s = ec - s (beta ed), s < nsteps <= 64, in registers.  An image of at most 48 KiB is
// staged whole, once per workgroup; a larger one chunk by chunk.  Sums: one partial per 64-row batch and step (the
// wave's rows by xor steps, the waves in wave order), part [nsteps, nb], added per step by the batch sums of
// ordered_sum.h: independent of the grid.
//
// The formulas follow ops/softmax.softmax_grad_torch / softmax_search_torch operation for operation (no contraction:
// the only fused operation is the matrix instruction).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gram64_mfma.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using namespace d64;

constexpr int SM_KMAX = 64, SM_GRAD_MAX_M = 128, SM_MAX_M = 1024, SM_MAX_STEPS = 64;
constexpr int SM_WHOLE = 12;        // (tile, chunk) units of 4 KiB of an image that the row pass stages whole
enum { M_R = 1, M_LOSS = 2 };

// The layout and the tile deal of the gradient pass for T class tiles and MT dim tiles.
template <int T, int MT>
struct GradTiles : WaveDeal<T * MT, (T * MT < 4)> {
    using Deal = WaveDeal<T * MT, (T * MT < 4)>;
    using Deal::MAXT;
    using Deal::SPLIT;
    using Deal::tile;
    static constexpr int NDCH = (MT + 1) / 2;
    static constexpr int SX = 16 * MT, SR = 16 * T;             // LDS row strides in doubles
    static constexpr bool XSW = MT % 2 == 0, RSW = T % 2 == 0;  // xor 16 into the columns of odd rows
    static constexpr int NTILES = T * MT;
    static constexpr bool W_LDS = T * NDCH < 16;

    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void step(d4_t (&acc)[MAXT], const double (&a)[T], const double (&b)[MT]) {
        if constexpr (s < MAXT) {
            constexpr int t = tile(WAVE, s);
            if constexpr (t < NTILES) acc[s] = mf64(a[t / MT], b[t % MT], acc[s]);
            step<WAVE, s + 1>(acc, a, b);
        }
    }

    template <int WAVE>
    static __device__ __forceinline__ void batch_of(d4_t (&acc)[MAXT], const double* __restrict__ xs,
                                                    const double* __restrict__ rs, int wave, int g, int mm) {
        const int base = SPLIT ? 16 * wave : 0;
        const int sw = (g & 1) << 4;        // the row's parity is g's
#pragma unroll 2
        for (int r4 = 0; r4 < (SPLIT ? 4 : 16); ++r4) {
            const int row = base + 4 * r4 + g;
            double a[T], b[MT];
#pragma unroll
            for (int t = 0; t < T; ++t) a[t] = rs[row * SR + ((16 * t + mm) ^ (RSW ? sw : 0))];
#pragma unroll
            for (int t = 0; t < MT; ++t) b[t] = xs[row * SX + ((16 * t + mm) ^ (XSW ? sw : 0))];
            step<WAVE>(acc, a, b);
        }
    }

    static __device__ __forceinline__ void batch(d4_t (&acc)[MAXT], const double* __restrict__ xs,
                                                 const double* __restrict__ rs, int wave, int g, int mm) {
        switch (wave) {
            case 0: batch_of<0>(acc, xs, rs, wave, g, mm); break;
            case 1: batch_of<1>(acc, xs, rs, wave, g, mm); break;
            case 2: batch_of<2>(acc, xs, rs, wave, g, mm); break;
            default: batch_of<3>(acc, xs, rs, wave, g, mm); break;
        }
    }

    // pc = the chunk's [loss | G [k1, m]]: slot s, q of a lane is G[16 tc + g + 4 q][16 td + mm]; the Store of finish
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[MAXT], double* __restrict__ pc, int k1, int m,
                                                 int g, int mm) {
        if constexpr (s < MAXT) {
            constexpr int t = tile(WAVE, s);
            if constexpr (t < NTILES) {
                const int col = 16 * (t % MT) + mm;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cls = 16 * (t / MT) + g + 4 * q;
                    if (cls < k1 && col < m) pc[1 + (int64_t)cls * m + col] = acc[s][q];
                }
            }
            store<WAVE, s + 1>(acc, pc, k1, m, g, mm);
        }
    }
};

template <int T, int MT, bool VEC>
__global__ __launch_bounds__(256) void softmax_grad_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w, int64_t n, int m,
        int k1, const double* __restrict__ img, int64_t chunk_rows, int64_t nchunk, double* __restrict__ part) {
    using L = GradTiles<T, MT>;
    constexpr int NDCH = L::NDCH;
    __shared__ __attribute__((aligned(32))) double xs[64 * L::SX];
    __shared__ __attribute__((aligned(32))) double rs[64 * L::SR];
    __shared__ __attribute__((aligned(32))) double wimg[L::W_LDS ? T * NDCH * 512 : 4];
    __shared__ __attribute__((aligned(32))) double red[L::RED];
    __shared__ double wl[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mm = lane & 15, g = lane >> 4;
    const int lr = wave * 16 + mm;          // the lane's row of a batch
    const int64_t P = 1 + (int64_t)k1 * m;
    if constexpr (L::W_LDS) {
#pragma unroll
        for (int i = 0; i < T * NDCH; ++i)
            reinterpret_cast<d2_t*>(wimg)[i * 256 + tid] = reinterpret_cast<const d2_t*>(img)[i * 256 + tid];
        __syncthreads();
    }
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        d4_t acc[L::MAXT];
#pragma unroll
        for (int s = 0; s < L::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        double lsum = 0.0;
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + lr;
            const bool ok = i < r1;
            const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)m;
            double xb[NDCH][2][4];
#pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) load_chunk<VEC>(xb[dc], xr, ok, dc, g, m);
            const double wi = ok ? w[i] : 0.0;
            const int yi = ok ? (int)y[i] : k1;
            d4_t e[T];
#pragma unroll
            for (int t = 0; t < T; ++t) e[t] = d4_t{0.0, 0.0, 0.0, 0.0};
            // The image does not change from batch to batch, and a small one may stay in registers for the whole
            // chunk; one of more than 8 (tile, group) units would be hoisted there too and spill, so its reads are
            // tied to a zero the compiler cannot see through.
            int pin = 0;
            if constexpr (T * MT > 8) asm volatile("" : "+v"(pin));
#pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (2 * dc + u >= MT) continue;         // no dim tile there
                    d4_t a[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int at = ((((t * NDCH + dc) * 2 + u) * 4 + g) * 16 + mm) * 4 + pin;
                        if constexpr (L::W_LDS) a[t] = *reinterpret_cast<const d4_t*>(wimg + at);
                        else a[t] = *reinterpret_cast<const d4_t*>(img + at);
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
#pragma unroll
                        for (int t = 0; t < T; ++t) e[t] = mf64(a[t][s], xb[dc][u][s], e[t]);
                    }
                    const int col = (16 * (2 * dc + u) + 4 * g) ^ (L::XSW ? (lr & 1) << 4 : 0);
                    *reinterpret_cast<d4_t*>(xs + lr * L::SX + col) =
                        d4_t{xb[dc][u][0], xb[dc][u][1], xb[dc][u][2], xb[dc][u][3]};
                }
            }
            const double lse = row_lse<T>(e, k1, g);
            double ey = 0.0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cls = 16 * t + g + 4 * q;
                    double r = 0.0;
                    if (cls < k1) {
                        r = exp(e[t][q] - lse);
                        if (cls == yi) {
                            r -= 1.0;
                            ey = e[t][q];
                        }
                        r *= wi;
                    }
                    rs[lr * L::SR + (cls ^ (L::RSW ? (lr & 1) << 4 : 0))] = r;
                }
            }
            ey = group_sum(ey);
            if (g == 0) lsum += (lse - ey) * wi;
            __syncthreads();
            L::batch(acc, xs, rs, wave, g, mm);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        lsum = osum::wave_sum_asc(lsum);    // the lanes with g > 0 add zeros
        if (lane == 0) wl[wave] = lsum;
        __syncthreads();
        if (tid == 0) pc[0] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
        L::template finish<L>(acc, red, wave, lane, pc, k1, m, g, mm);
        __syncthreads();            // wl and red may be written again
    }
}

// img: one block of NT tiles in the image order of dense64_mfma.h, [ndch][u][NT][g][mm][s]
template <int TW, bool SEARCH, bool WHOLE, bool VEC>
__global__ __launch_bounds__(256) void softmax_rows_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w, int64_t n, int d,
        int k1, const double* __restrict__ img, int ndch, double beta, int nsteps, int mask, double* __restrict__ R,
        double* __restrict__ part, int64_t nb) {
    constexpr int NT = SEARCH ? 2 * TW : TW;
    extern __shared__ __attribute__((aligned(16))) double cent[];       // WHOLE: ndch chunks, else one
    __shared__ double ws[SEARCH ? SM_MAX_STEPS : 1][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mm = lane & 15, g = lane >> 4;
    if constexpr (WHOLE) {
        for (int i = 0; i < ndch * NT; ++i)
            reinterpret_cast<d2_t*>(cent)[i * 256 + tid] = reinterpret_cast<const d2_t*>(img)[i * 256 + tid];
        __syncthreads();
    }
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + mm;
        const bool ok = row < n;
        const double* __restrict__ xr = X + (ok ? row : 0) * (int64_t)d;
        d4_t acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int dc = 0; dc < ndch; ++dc) {
            double xb[2][4];
            load_chunk<VEC>(xb, xr, ok, dc, g, d);
            if constexpr (!WHOLE) stage<NT>(cent, img, 0, ndch, dc);
            const double* __restrict__ cc = WHOLE ? cent + dc * (NT * 512) : cent;
            mfma_group<NT>(acc, cc, xb[0], 0, g, mm);
            if (dc * DCH + 16 < d) mfma_group<NT>(acc, cc, xb[1], 1, g, mm);
        }
        const double wi = ok ? w[row] : 0.0;
        const int yi = ok ? (int)y[row] : k1;
        if constexpr (SEARCH) {
            double ecy = 0.0, edy = 0.0;
            d4_t dd[TW];
#pragma unroll
            for (int t = 0; t < TW; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (16 * t + g + 4 * q == yi && yi < k1) {
                        ecy = acc[t][q];
                        edy = acc[TW + t][q];
                    }
                    dd[t][q] = acc[TW + t][q] * beta;
                }
            }
            ecy = group_sum(ecy);
            const double dy = group_sum(edy) * beta;
            for (int s = 0; s < nsteps; ++s) {
                const double sd = (double)s;
                d4_t e[TW];
#pragma unroll
                for (int t = 0; t < TW; ++t) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) e[t][q] = acc[t][q] - sd * dd[t][q];
                }
                const double lse = row_lse<TW>(e, k1, g);
                const double v = osum::wave_sum_asc(g == 0 ? (lse - (ecy - sd * dy)) * wi : 0.0);
                if (lane == 0) ws[s][wave] = v;
            }
        } else {
            const double lse = row_lse<TW>(acc, k1, g);
            double ey = 0.0;
            double* __restrict__ rr = R + (ok ? row : 0) * (int64_t)k1;
#pragma unroll
            for (int t = 0; t < TW; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cls = 16 * t + g + 4 * q;
                    if (cls < k1) {
                        if (cls == yi) ey = acc[t][q];
                        if ((mask & M_R) && ok) {
                            double r = exp(acc[t][q] - lse);
                            if (cls == yi) r -= 1.0;
                            rr[cls] = r * wi;
                        }
                    }
                }
            }
            ey = group_sum(ey);
            const double v = osum::wave_sum_asc(g == 0 ? (lse - ey) * wi : 0.0);
            if (lane == 0) ws[0][wave] = v;
        }
        if (SEARCH || (mask & M_LOSS)) {
            __syncthreads();
            if (tid < nsteps) part[(int64_t)tid * nb + b] = ((ws[tid][0] + ws[tid][1]) + ws[tid][2]) + ws[tid][3];
            __syncthreads();        // ws may be written again
        }
    }
}

template <int T, bool VEC, class... Args>
void launch_grad(int mt, unsigned blocks, hipStream_t st, Args... a) {
    switch (mt) {
        case 1: hipLaunchKernelGGL((softmax_grad_kernel<T, 1, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 2: hipLaunchKernelGGL((softmax_grad_kernel<T, 2, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 3: hipLaunchKernelGGL((softmax_grad_kernel<T, 3, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 4: hipLaunchKernelGGL((softmax_grad_kernel<T, 4, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 5: hipLaunchKernelGGL((softmax_grad_kernel<T, 5, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 6: hipLaunchKernelGGL((softmax_grad_kernel<T, 6, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        case 7: hipLaunchKernelGGL((softmax_grad_kernel<T, 7, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
        default: hipLaunchKernelGGL((softmax_grad_kernel<T, 8, VEC>), dim3(blocks), dim3(256), 0, st, a...); break;
    }
}

template <bool VEC, class... Args>
void launch_grad_t(int t, int mt, unsigned blocks, hipStream_t st, Args... a) {
    switch (t) {
        case 1: launch_grad<1, VEC>(mt, blocks, st, a...); break;
        case 2: launch_grad<2, VEC>(mt, blocks, st, a...); break;
        case 3: launch_grad<3, VEC>(mt, blocks, st, a...); break;
        default: launch_grad<4, VEC>(mt, blocks, st, a...); break;
    }
}

template <int TW, bool SEARCH, class... Args>
void launch_rows(bool whole, bool vec, unsigned blocks, size_t lds, hipStream_t st, Args... a) {
    if (whole && vec)
        hipLaunchKernelGGL((softmax_rows_kernel<TW, SEARCH, true, true>), dim3(blocks), dim3(256), lds, st, a...);
    else if (whole)
        hipLaunchKernelGGL((softmax_rows_kernel<TW, SEARCH, true, false>), dim3(blocks), dim3(256), lds, st, a...);
    else if (vec)
        hipLaunchKernelGGL((softmax_rows_kernel<TW, SEARCH, false, true>), dim3(blocks), dim3(256), lds, st, a...);
    else
        hipLaunchKernelGGL((softmax_rows_kernel<TW, SEARCH, false, false>), dim3(blocks), dim3(256), lds, st, a...);
}

}  // namespace

extern "C" {

// One gradient pass over X [n, m] (1 <= m <= 128), y, w [n] at the coefficients whose tile-outermost image is img
// [ceil(k1 / 16), ceil(m / 32), 2, 4, 16, 4]: out [1 + k1 m] = [sum w loss | G [k1, m]] through nchunk =
// ceil(n / chunk_rows) row chunks (chunk_rows a multiple of 64) whose partials part [nchunk, 1 + k1 m] are merged in
// chunk order.
int alink_softmax_fused_grad_f64(const double* X, const double* y, const double* w, int64_t n, int m, int k1,
                                 const double* img, int64_t chunk_rows, int64_t nchunk, double* part, double* out,
                                 int grid, void* stream) {
    if (n <= 0) return 0;
    if (m < 1 || m > SM_GRAD_MAX_M || k1 < 1 || k1 > SM_KMAX || n >= (1ll << 31)) return 1;
    if (chunk_rows < 64 || chunk_rows % 64 != 0 || nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || img == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int t = (k1 + 15) / 16, mt = (m + 15) / 16;
    const unsigned blocks = (unsigned)(grid > 0 && grid < nchunk ? grid : nchunk);
    if (vec_ok(m, X)) launch_grad_t<true>(t, mt, blocks, st, X, y, w, n, m, k1, img, chunk_rows, nchunk, part);
    else launch_grad_t<false>(t, mt, blocks, st, X, y, w, n, m, k1, img, chunk_rows, nchunk, part);
    osum::chunk_merge(osum::Identity{}, 1 + (int64_t)k1 * m, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The row pass over X [n, m] (1 <= m <= 1024) with the lane-ordered image img [ceil(m / 32), 2, NT, 4, 16, 4] of the
// table: W padded to tw = 1, 2 or 4 tiles of 16 classes (NT = tw), or with search != 0 [W ; D], each padded to tw
// tiles (NT = 2 tw).  Plain: mask 1 writes R [n, k1], mask 2 gives out [1] = sum w loss.  Search: out [nsteps] = the
// weighted losses at W - s beta D, s < nsteps <= 64.  part [nsteps, ceil(n / 64)] (nsteps = 1 for the plain pass).
int alink_softmax_fused_rows_f64(const double* X, const double* y, const double* w, int64_t n, int m, int k1,
                                 const double* img, int tw, int search, double beta, int nsteps, int mask, double* R,
                                 double* part, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (m < 1 || m > SM_MAX_M || k1 < 1 || k1 > SM_KMAX || n >= (1ll << 31)) return 1;
    if ((tw != 1 && tw != 2 && tw != 4) || 16 * tw < k1) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || img == nullptr) return 1;
    if (search) {
        if (nsteps < 1 || nsteps > SM_MAX_STEPS || part == nullptr || out == nullptr) return 1;
        mask = 0;
    } else {
        if (mask <= 0 || mask > (M_R | M_LOSS)) return 1;
        if ((mask & M_R) && R == nullptr) return 1;
        if ((mask & M_LOSS) && (part == nullptr || out == nullptr)) return 1;
        nsteps = 1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (m + DCH - 1) / DCH, nt = search ? 2 * tw : tw;
    const bool whole = ndch * nt <= SM_WHOLE, vec = vec_ok(m, X);
    const size_t lds = (size_t)(whole ? ndch : 1) * nt * 512 * sizeof(double);
    const int64_t nb = (n + ROWS - 1) / ROWS;
    const unsigned blocks = row_blocks(n, grid, 4096);
#define ALINK_SM_ROWS(TW, SEARCH) \
    launch_rows<TW, SEARCH>(whole, vec, blocks, lds, st, X, y, w, n, m, k1, img, ndch, beta, nsteps, mask, R, part, nb)
    if (search) {
        if (tw == 1) ALINK_SM_ROWS(1, true);
        else if (tw == 2) ALINK_SM_ROWS(2, true);
        else ALINK_SM_ROWS(4, true);
    } else {
        if (tw == 1) ALINK_SM_ROWS(1, false);
        else if (tw == 2) ALINK_SM_ROWS(2, false);
        else ALINK_SM_ROWS(4, false);
    }
#undef ALINK_SM_ROWS
    if (search || (mask & M_LOSS)) osum::batch_sums(part, nb, nsteps, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
