// The upper-triangle Gram tile deal shared by the fp64 Gram passes — glm.hip (the weighted Gram of the IRLS pass),
// moments.hip (the diagonal units of the moment pass) and newton.hip (the Hessian and gradient of the Newton pass) —
// gfx950 / MI355X.
//
// The problem they share: a workgroup of 4 waves has staged a batch of 64 rows a_i of NT tiles of 16 columns in LDS
// (row stride S = 16 NT + 16 doubles, so the four lane groups of a read start 32 banks apart; the columns behind the
// row's width are zero) and adds sum_i w_i a_i a_i^T to accumulators that stay in registers for a whole row chunk.
//
// Operand and result maps (one v_mfma_f64_16x16x4_f64 = four consecutive rows i0 .. i0 + 3, m = lane & 15,
// g = lane >> 4):
//   A[m][g] = a_{i0+g}[16 ta + m]   (WEIGHTED: times the row weight ww_{i0+g}, read from wws);
//   B[g][m] = a_{i0+g}[16 tb + m];
//   D  slot q = 0..3 of a lane is element [16 ta + g + 4 q][16 tb + m] of the sum.
//   A lane reads its row's NT column values from LDS once per step and uses them for every tile it owns.
// Tiles: the TU = NT (NT + 1) / 2 upper tiles in the order ta ascending, then tb (tile_a / tile_b); ONES: behind them
// NT "ones" tiles, A = 1.0 on every lane, whose every result row is the column sum of tile tb (result row 0 is kept).
// ONES = SCALAR (newton.hip): the same NT tiles with A = the row's scalar sc_{i0+g}, read from wws[64 + row] behind the
// 64 weights, where the ones tiles have 1.0: every result row is sum_i sc_i a_i[16 tb + m] (result row 0 is kept).
//
// Ownership, two rules:
//   NT >= 3  tile t belongs to wave t mod 4, which runs all 64 rows of the batch for it;
//   NT <= 2  (SPLIT) every wave holds all T tiles and runs its own 16 rows of the batch; at the chunk's end the four
//            waves' partials are added through LDS (`red`) in wave order by wave 0, which stores them.
// Both rules depend on the width (NT) alone: never on the grid, the chunk length or the row count, so a chunk's
// partial has the same bits in every launch.  The two rules themselves, for any list of T tiles, are WaveDeal, which
// the gradient pass of softmax_fused.hip deals its own tile list by (mlp_fused.hip keeps the rules written out:
// profiles/ordered_sum.txt).  The chunks' partials are then merged in chunk order (ordered_sum.h, with the map that
// mirrors the lower triangle from the upper).
//
// The store of a wave's tiles at the chunk's end is the caller's: `finish` takes a type Store with
//   template <int WAVE> static void store(const d4_t (&acc)[MAXT], Args... args)
// and passes its trailing arguments on by value.  Store walks the wave's slots with tile() and writes slot q of a
// tile by the result map above.  (An element hook `put(ra, cb, v)` under a shared store was tried first: it compiled
// the guards of moments.hip to other code and the moment pass measured 0.2 % to 1 % slower at 96 and 128 columns,
// profiles/gram_shared_triangle.txt.)
//
// No contraction: the pragma below covers this header's own code (the weight's multiply, the fold's additions) whatever
// the including file says later; it stands here, before the first function, because a file-scope pragma holds from
// where it is written and the including files set theirs only after their includes.
#pragma once
#include "dense64_mfma.h"

#pragma clang fp contract(off)

namespace d64 {

// upper tile t of an NT x NT tile matrix, tile rows ascending, then tile columns
constexpr int tile_a(int nt, int t) {
    int ta = 0;
    while (t >= nt - ta) {
        t -= nt - ta;
        ++ta;
    }
    return ta;
}
constexpr int tile_b(int nt, int t) {
    int ta = 0;
    while (t >= nt - ta) {
        t -= nt - ta;
        ++ta;
    }
    return ta + t;
}

// the values of ONES: false (0) no such tiles, true (1) the ones tiles, SCALAR the scalar-operand tiles
constexpr int SCALAR = 2;

// The deal of a list of T accumulator tiles to the four waves of a workgroup, and the fold at a chunk's end.
// SPLIT false: tile t belongs to wave t mod 4 (slot t / 4), which runs all 64 rows of a batch for it.  SPLIT true
// (a short list; the threshold is the caller's): every wave holds all T tiles and runs its own 16 rows.
template <int T, bool SPLIT_>
struct WaveDeal {
    static constexpr bool SPLIT = SPLIT_;               // the waves split the rows, not the tiles
    static constexpr int MAXT = SPLIT ? T : (T + 3) / 4;    // accumulator tiles per wave
    static constexpr int RED = SPLIT ? 4 * T * 256 : 1;     // doubles of the LDS array `red` (32-byte aligned)

    // the tile in slot s of wave `wave`
    static constexpr int tile(int wave, int s) { return SPLIT ? s : wave + 4 * s; }

    // the end of a chunk: every thread of the workgroup calls it.  SPLIT: the four waves' partials through red
    // [RED] in wave order, stored by wave 0 (two barriers, the second so that red may be written again); else every
    // wave stores its own tiles, Store::store<WAVE>(acc, args...).
    template <class Store, class... Args>
    static __device__ __forceinline__ void finish(d4_t (&acc)[MAXT], double* __restrict__ red, int wave, int lane,
                                                  Args... args) {
        if constexpr (SPLIT) {
#pragma unroll
            for (int s = 0; s < MAXT; ++s) *reinterpret_cast<d4_t*>(red + ((wave * T + s) * 64 + lane) * 4) = acc[s];
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int s = 0; s < MAXT; ++s) {
                    d4_t a = *reinterpret_cast<const d4_t*>(red + (s * 64 + lane) * 4);
                    for (int ws = 1; ws < 4; ++ws)
                        a += *reinterpret_cast<const d4_t*>(red + ((ws * T + s) * 64 + lane) * 4);
                    acc[s] = a;
                }
                Store::template store<0>(acc, args...);
            }
            __syncthreads();
        } else {
            switch (wave) {
                case 0: Store::template store<0>(acc, args...); break;
                case 1: Store::template store<1>(acc, args...); break;
                case 2: Store::template store<2>(acc, args...); break;
                default: Store::template store<3>(acc, args...); break;
            }
        }
    }
};

template <int NT, bool WEIGHTED, int ONES>
struct GramTiles : WaveDeal<NT * (NT + 1) / 2 + (ONES ? NT : 0), (NT <= 2)> {
    using Deal = WaveDeal<NT * (NT + 1) / 2 + (ONES ? NT : 0), (NT <= 2)>;
    using Deal::MAXT;
    using Deal::SPLIT;
    using Deal::tile;
    static constexpr int S = 16 * NT + 16;              // LDS row stride in doubles
    static constexpr int TU = NT * (NT + 1) / 2;        // upper tiles
    static constexpr int T = TU + (ONES ? NT : 0);      // and the ones tiles behind them

    // one step of four rows for the wave's slots s, the tile indices compile-time
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void step(d4_t (&acc)[MAXT], double ww, double sc, const double (&v)[NT]) {
        if constexpr (s < MAXT) {
            constexpr int t = tile(WAVE, s);
            // the tile's indices as constants of their own: left inside the call, their loops run on the device
            constexpr int ta = t < TU ? tile_a(NT, t) : 0, tb = t < TU ? tile_b(NT, t) : t - TU;
            if constexpr (t < TU && WEIGHTED) acc[s] = mf64(ww * v[ta], v[tb], acc[s]);
            else if constexpr (t < TU) acc[s] = mf64(v[ta], v[tb], acc[s]);
            else if constexpr (t < T) acc[s] = mf64(ONES == SCALAR ? sc : 1.0, v[tb], acc[s]);
            step<WAVE, s + 1>(acc, ww, sc, v);
        }
    }

    // the products of the staged batch: all 64 rows for the wave's tiles, or the wave's 16 rows for every tile
    template <int WAVE>
    static __device__ __forceinline__ void batch_of(d4_t (&acc)[MAXT], const double* __restrict__ rows,
                                                    const double* __restrict__ wws, int wave, int g, int m) {
        const int base = SPLIT ? 16 * wave : 0;
#pragma unroll 2
        for (int r4 = 0; r4 < (SPLIT ? 4 : 16); ++r4) {
            const int row = base + 4 * r4 + g;
            double ww = 0.0, sc = 0.0;
            if constexpr (WEIGHTED) ww = wws[row];
            if constexpr (ONES == SCALAR) sc = wws[64 + row];
            double v[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) v[t] = rows[row * S + 16 * t + m];
            step<WAVE>(acc, ww, sc, v);
        }
    }

    // the batch staged in rows [64 * S] (and wws [64], read when WEIGHTED only; SCALAR: wws [128]) into the wave's
    // accumulators; the
    // caller's barriers stand before it (the batch is staged) and after it (its reads are done)
    static __device__ __forceinline__ void batch(d4_t (&acc)[MAXT], const double* __restrict__ rows,
                                                 const double* __restrict__ wws, int wave, int g, int m) {
        switch (wave) {
            case 0: batch_of<0>(acc, rows, wws, wave, g, m); break;
            case 1: batch_of<1>(acc, rows, wws, wave, g, m); break;
            case 2: batch_of<2>(acc, rows, wws, wave, g, m); break;
            default: batch_of<3>(acc, rows, wws, wave, g, m); break;
        }
    }
};

// The row load of the passes that stage whole rows (glm.hip, newton.hip).
// The row xr [k] as seen by lane sub of its four lanes: v[j] = the columns 8 j + 2 sub and + 1 (zero behind k or
// when the row is not `ok`; no address is loaded that lies outside the row), and the row's dot with bet (LDS, zero
// behind k): every lane adds its pairs by fma in ascending j, then the four lanes are added by two xor steps, so
// all four return the same bits, which depend on the row and k alone.
template <int NT, bool VEC>
__device__ __forceinline__ double row_dot(const double* __restrict__ xr, bool ok, int k, int sub,
                                          const double* __restrict__ bet, d2_t (&v)[2 * NT]) {
#pragma unroll
    for (int j = 0; j < 2 * NT; ++j) {
        const int c = 8 * j + 2 * sub;
        d2_t t = {0.0, 0.0};
        if (VEC) {
            if (ok && c < k) t = *reinterpret_cast<const d2_t*>(xr + c);
        } else {
            if (ok && c < k) t[0] = xr[c];
            if (ok && c + 1 < k) t[1] = xr[c + 1];
        }
        v[j] = t;
    }
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * NT; ++j) {
        const d2_t b = *reinterpret_cast<const d2_t*>(bet + 8 * j + 2 * sub);
        dot = fma(v[j][0], b[0], dot);
        dot = fma(v[j][1], b[1], dot);
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    return dot;
}

// beta [k] into bet [128], zero behind k (or everywhere without a beta); every thread of the workgroup calls it
__device__ __forceinline__ void stage_beta(double* __restrict__ bet, const double* __restrict__ beta, int k) {
    const int tid = threadIdx.x;
    if (tid < 128) bet[tid] = (beta != nullptr && tid < k) ? beta[tid] : 0.0;
    __syncthreads();
}

}  // namespace d64
