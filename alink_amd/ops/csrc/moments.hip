// Second-moment statistics and the PCA projection on gfx950 / MI355X (ops/moments.py), for contiguous fp64 rows
// X [n, d] with 1 <= d <= 1024.
//
// alink_moments_f64: one pass that gives out = [t | C], t = sum_i y_i, C = sum_i y_i y_i^T over the shifted rows
// y_i = x_i - shift (shift [d] or null: zero).  The columns are cut into blocks of MB = 128 (8 MFMA tiles of 16); a
// unit of work is (row chunk, block pair A <= B).  A workgroup of 4 waves walks its chunk 64 rows at a time:
//   load    four lanes per row (tid >> 2 the row, tid & 3 = sub) read the row's slice of block A (and of block B in
//           an off-diagonal unit), lane sub the 4-column groups 4 j + sub (d64::load_group: two 16-byte loads where d
//           is even and X 16-byte aligned, four 8-byte loads otherwise; no address outside the row is loaded),
//           subtract the shift (staged once per unit in LDS) and store the shifted slice to the row's LDS slot; the
//           columns behind d and the rows behind the chunk are zero.
//   tiles   after one barrier, v_mfma_f64_16x16x4_f64 over four consecutive rows per instruction, with the operand
//           and result maps of gram64_mfma.h.  Accumulators stay in registers for the whole chunk.
//           diagonal unit (block of NT tiles): the upper tile triangle of gram64_mfma.h with its NT "ones" tiles,
//             whose result is the column sum t: at most 36 + 8 tiles (which wave owns which is described there).
//           off-diagonal unit (A < B, so A has 8 tiles, B has nb <= 8): wave w owns the tile rows 2 w and 2 w + 1
//             and all nb tile columns, 16 tiles at most.
//           Both rules depend on (d, A, B) alone, and t comes out of the matrix instruction: nothing depends on
//           the grid.
//   merge   part [nchunk, d + d d] holds each chunk's t and the entries of its upper tiles, merged in chunk order
//           with the mirror map of ordered_sum.h, so C is exactly symmetric: the same bits for every grid and run.
// The diagonal units of the full blocks, the diagonal unit of a last block of fewer tiles and the off-diagonal units
// are three launches (each kernel has its own tile count at compile time); they write disjoint parts of `part`.
//
// alink_pca_project_f64: P[i, j] = sum_c z_ic T[j, c] / sstd[j], z_ic = (x_ic - mean[c]) / scale[c] (a true fp64
// division; scale[c] = 0 gives exactly 0 whatever the cell holds), on the shared tile loop of dense64_mfma.h: 64
// rows per workgroup, the table T as the lane-ordered image staged in LDS per (block, dim chunk), the row chunk
// transformed in registers right after the guarded load (load_shifted = load_group + shift_group, as the moment pass).  The epilogue
// divides by sstd[j] and writes P [n, k] only.
//
// alink_pairwise_moments_f64: the pairwise-complete statistics of rows whose NaN cells are missing, out [4, d, d] =
// [N | S | Q | P] with y_ia = x_ia - shift_a on present cells and m_ia the presence flag:
//   N[a,b] = sum_i m_ia m_ib,  S[a,b] = sum_i y_ia m_ib,  Q[a,b] = sum_i y_ia^2 m_ib,  P[a,b] = sum_i y_ia y_ib m_ia m_ib
// (S and Q are not symmetric).  The scheme of the moment pass with a tile plan of its own: blocks of PB = 64 columns
// (4 tiles; a tile pair needs about six accumulator tiles here, not one), a unit is (row chunk, block pair A <= B).
//   load    as above, but only y goes to LDS, one slice per block (41 KB, 82 KB in an off-diagonal unit), and NaN is
//           kept as the missing marker: the columns behind d and the rows behind the chunk are staged as NaN.
//   tiles   a lane reads its row's y of a tile once per four-row step and forms v = isnan(y) ? 0 : y, z = v v and
//           k = isnan(y) ? 0 : 1 in registers; one matrix instruction per tile pair gives k^T k (N), v^T v (P),
//           v^T k (S) and z^T k (Q).
//           diagonal unit of NT tiles: the upper triangle for N and P, all NT^2 pairs for S and Q, 2 NT (NT + 1) / 2 +
//             2 NT^2 tiles (52 at NT = 4, 4 at NT = 1);
//           off-diagonal unit (A of 4 tiles, B of nb <= 4): N_AB, P_AB, S_AB = v_A^T k_B, S_BA = v_B^T k_A, Q_AB,
//             Q_BA, 24 nb tiles (96 at nb = 4: 192 accumulator registers of a wave).
//           One rule for every width: tile t of the unit's list belongs to wave t mod 4, which runs all 64 rows of a
//           batch for it (at NT = 1 the four waves hold N, P, S and Q).  It depends on (d, A, B) alone.  No
//           instantiation spills, so no deal was narrowed.
//   merge   part [nchunk, 4 d d], merged in chunk order with the map PairwiseMirror, which mirrors the lower triangles
//           of N and P only: they are exactly symmetric, S and Q stay as computed; no float atomics, the same bits
//           for every grid, run and alignment.
// The diagonal units of the full blocks, of a ragged last block, the off-diagonal units between full blocks and those
// against the last block are four launches; they write disjoint parts of `part`.
//
// All arithmetic is fp64, no contraction: the only fused operation is the matrix instruction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram64_mfma.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using namespace d64;

constexpr int MB = 128;             // columns per block: 8 tiles, the widest triangle one workgroup holds
constexpr int MOMENTS_DMAX = 1024;

// The shift of one loaded group: v[s] - sh[so + s] for the four dims j0 .. j0 + 3 of a row (v by load_group);
// SCALED: then divided by sc[so + s], a zero scale giving exactly 0 (also for a non-finite cell).  Zero outside
// [0, d) or when the row is not `ok`.  SCALED reads sh / sc for dims inside the row only (global tables of d
// entries); otherwise sh[so .. so + 3] is read whole (an LDS slice, zero behind d), which keeps the guards flat
// selects and lets a caller keep many loads in flight.
template <bool SCALED>
__device__ __forceinline__ d4_t shift_group(d4_t v, bool ok, int j0, int d, const double* __restrict__ sh,
                                            const double* __restrict__ sc, int so) {
    d4_t r;
    if (SCALED) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            double y = 0.0;
            if (ok && j0 + s < d) {
                const double c = sc[so + s];
                y = c == 0.0 ? 0.0 : (v[s] - sh[so + s]) / c;
            }
            r[s] = y;
        }
    } else {
        const d4_t h = *reinterpret_cast<const d4_t*>(sh + so);
#pragma unroll
        for (int s = 0; s < 4; ++s) r[s] = (ok && j0 + s < d) ? v[s] - h[s] : 0.0;
    }
    return r;
}

// the guarded load and its shift in one: the shifted load of the moment pass and of the projection
template <bool VEC, bool SCALED>
__device__ __forceinline__ d4_t load_shifted(const double* __restrict__ xr, bool ok, int j0, int d,
                                             const double* __restrict__ sh, const double* __restrict__ sc, int so) {
    return shift_group<SCALED>(load_group<VEC>(xr, ok, j0, d), ok, j0, d, sh, sc, so);
}

// One row's slice of NT tiles starting at column c0 into its LDS slot: lane sub of the row's four lanes the
// 4-column groups 4 j + sub.  All NT loads are issued before the first is used (load_slice), then shifted and
// stored (store_slice = the rest of load_shifted).
template <int NT, bool VEC>
__device__ __forceinline__ void load_slice(d4_t (&v)[NT], const double* __restrict__ xr, bool ok, int c0, int d,
                                           int sub) {
#pragma unroll
    for (int j = 0; j < NT; ++j) v[j] = load_group<VEC>(xr, ok, c0 + 4 * (4 * j + sub), d);
}

template <int NT>
__device__ __forceinline__ void store_slice(double* __restrict__ slot, const d4_t (&v)[NT], bool ok, int c0, int d,
                                            const double* __restrict__ sh, int sub) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int q = 4 * (4 * j + sub);
        *reinterpret_cast<d4_t*>(slot + q) = shift_group<false>(v[j], ok, c0 + q, d, sh, nullptr, q);
    }
}

// the shift of the NT tiles from column c0 on into sh (zero behind d or without a shift); threads t0 .. t0 + 16 NT
__device__ __forceinline__ void stage_shift(double* __restrict__ sh, const double* __restrict__ shift, int c0, int d,
                                            int nt, int t) {
    if (t >= 0 && t < 16 * nt) sh[t] = (shift != nullptr && c0 + t < d) ? shift[c0 + t] : 0.0;
}

// pc = the chunk's [t | C], the block starts at column c0: the upper tiles' entries and, from result row 0 of a ones
// tile, t
template <int NT>
struct DiagStore {
    using D = GramTiles<NT, false, true>;
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[D::MAXT], double* __restrict__ pc, int d, int c0,
                                                 int g, int m) {
        if constexpr (s < D::MAXT) {
            constexpr int t = D::tile(WAVE, s);
            if constexpr (t < D::TU) {
                constexpr int ta = tile_a(NT, t), tb = tile_b(NT, t);
                const int cb = c0 + 16 * tb + m;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ra = c0 + 16 * ta + g + 4 * q;
                    if (ra < d && cb < d) pc[d + (int64_t)ra * d + cb] = acc[s][q];
                }
            } else if constexpr (t < D::T) {
                const int cb = c0 + 16 * (t - D::TU) + m;
                if (g == 0 && cb < d) pc[cb] = acc[s][0];
            }
            store<WAVE, s + 1>(acc, pc, d, c0, g, m);
        }
    }
};

// the diagonal units (chunk, block blk0 + b), b < nblk, every block of NT tiles
template <int NT, bool VEC>
__global__ __launch_bounds__(256) void moments_diag_kernel(const double* __restrict__ X, int64_t n, int d,
                                                           const double* __restrict__ shift, int blk0, int nblk,
                                                           int64_t chunk_rows, int64_t nchunk,
                                                           double* __restrict__ part) {
    using D = GramTiles<NT, false, true>;
    constexpr int S = D::S;
    __shared__ __attribute__((aligned(32))) double rows[64 * S];
    __shared__ __attribute__((aligned(32))) double sh[16 * NT];
    __shared__ __attribute__((aligned(32))) double red[D::RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid >> 2, sub = tid & 3;
    const int m = lane & 15, g = lane >> 4;
    const int64_t P = d + (int64_t)d * d;
    for (int64_t u = blockIdx.x; u < nchunk * nblk; u += gridDim.x) {
        const int64_t c = u / nblk;
        const int c0 = (blk0 + (int)(u - c * nblk)) * MB;
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        stage_shift(sh, shift, c0, d, NT, tid);     // the previous unit's reads ended at its last barrier
        __syncthreads();
        d4_t acc[D::MAXT];
#pragma unroll
        for (int s = 0; s < D::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + r;
            const bool ok = i < r1;
            d4_t v[NT];
            load_slice<NT, VEC>(v, X + (ok ? i : r0) * (int64_t)d, ok, c0, d, sub);
            store_slice<NT>(rows + r * S, v, ok, c0, d, sh, sub);
            __syncthreads();
            D::batch(acc, rows, nullptr, wave, g, m);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        D::template finish<DiagStore<NT>>(acc, red, wave, lane, pc, d, c0, g, m);
    }
}

constexpr int OS = MB + 16;         // LDS row stride of the off-diagonal slices

// The products of the staged batch of an off-diagonal unit: wave WAVE's tile rows 2 WAVE and 2 WAVE + 1 against the
// nb tile columns of B (FULL: nb = 8, no test), acc[8 i + j] the tile (2 WAVE + i, j).
template <int WAVE, bool FULL>
__device__ __forceinline__ void off_batch(d4_t (&acc)[16], const double* __restrict__ ra, const double* __restrict__ rb,
                                          int nb, int g, int m) {
#pragma unroll 2
    for (int r4 = 0; r4 < 16; ++r4) {
        const int row = 4 * r4 + g;
        const double a0 = ra[row * OS + 32 * WAVE + m], a1 = ra[row * OS + 32 * WAVE + 16 + m];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (FULL || j < nb) {
                const double b = rb[row * OS + 16 * j + m];
                acc[j] = mf64(a0, b, acc[j]);
                acc[8 + j] = mf64(a1, b, acc[8 + j]);
            }
        }
    }
}

template <int WAVE>
__device__ __forceinline__ void off_store(const d4_t (&acc)[16], double* __restrict__ pc, int d, int ca, int cb0,
                                          int g, int m) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int cb = cb0 + 16 * j + m;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra = ca + 16 * (2 * WAVE + i) + g + 4 * q;
                if (ra < d && cb < d) pc[d + (int64_t)ra * d + cb] = acc[8 * i + j][q];
            }
        }
    }
}

// the off-diagonal units (chunk, A < B) of nblk >= 2 blocks, the pairs in the order A ascending, then B
template <bool VEC>
__global__ __launch_bounds__(256) void moments_off_kernel(const double* __restrict__ X, int64_t n, int d,
                                                          const double* __restrict__ shift, int nblk,
                                                          int64_t chunk_rows, int64_t nchunk,
                                                          double* __restrict__ part) {
    __shared__ __attribute__((aligned(32))) double ra[64 * OS];
    __shared__ __attribute__((aligned(32))) double rb[64 * OS];
    __shared__ __attribute__((aligned(32))) double sh[2 * MB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid >> 2, sub = tid & 3;
    const int m = lane & 15, g = lane >> 4;
    const int64_t P = d + (int64_t)d * d;
    const int npair = nblk * (nblk - 1) / 2;
    for (int64_t u = blockIdx.x; u < nchunk * npair; u += gridDim.x) {
        const int64_t c = u / npair;
        int p = (int)(u - c * npair), A = 0;
        while (p >= nblk - 1 - A) {
            p -= nblk - 1 - A;
            ++A;
        }
        const int ca = A * MB, cb0 = (A + 1 + p) * MB;
        const int nb = d - cb0 >= MB ? 8 : (d - cb0 + 15) / 16;
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        stage_shift(sh, shift, ca, d, 8, tid);
        stage_shift(sh + MB, shift, cb0, d, 8, tid - MB);
        __syncthreads();
        d4_t acc[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + r;
            const bool ok = i < r1;
            const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)d;
            d4_t va[8], vb[8];
            load_slice<8, VEC>(va, xr, ok, ca, d, sub);
            load_slice<8, VEC>(vb, xr, ok, cb0, d, sub);
            store_slice<8>(ra + r * OS, va, ok, ca, d, sh, sub);
            store_slice<8>(rb + r * OS, vb, ok, cb0, d, sh + MB, sub);
            __syncthreads();
            if (nb == 8) {
                switch (wave) {
                    case 0: off_batch<0, true>(acc, ra, rb, nb, g, m); break;
                    case 1: off_batch<1, true>(acc, ra, rb, nb, g, m); break;
                    case 2: off_batch<2, true>(acc, ra, rb, nb, g, m); break;
                    default: off_batch<3, true>(acc, ra, rb, nb, g, m); break;
                }
            } else {
                switch (wave) {
                    case 0: off_batch<0, false>(acc, ra, rb, nb, g, m); break;
                    case 1: off_batch<1, false>(acc, ra, rb, nb, g, m); break;
                    case 2: off_batch<2, false>(acc, ra, rb, nb, g, m); break;
                    default: off_batch<3, false>(acc, ra, rb, nb, g, m); break;
                }
            }
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        switch (wave) {
            case 0: off_store<0>(acc, pc, d, ca, cb0, g, m); break;
            case 1: off_store<1>(acc, pc, d, ca, cb0, g, m); break;
            case 2: off_store<2>(acc, pc, d, ca, cb0, g, m); break;
            default: off_store<3>(acc, pc, d, ca, cb0, g, m); break;
        }
    }
}

// img: the image of T [k, nx] (dense64_mfma.h), nblk blocks of 16 NT table rows, ndch = ceil(nx / 32) dim chunks
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void pca_project_kernel(
        const double* __restrict__ X, int64_t n, int nx, const double* __restrict__ mean,
        const double* __restrict__ scale, const double* __restrict__ img, int k, int nblk, int ndch,
        const double* __restrict__ sstd, double* __restrict__ P) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + m;
        const bool row_ok = row < n;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)nx;
        for (int cb = 0; cb < nblk; ++cb) {
            d4_t acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
            for (int dc = 0; dc < ndch; ++dc) {
                // this lane's dims of the row, standardised (zero outside the row), then the table block of the chunk
                double xb[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j0 = dc * DCH + 16 * u + 4 * g;
                    const d4_t v = load_shifted<VEC, true>(xr, row_ok, j0, nx, mean, scale, j0);
#pragma unroll
                    for (int s = 0; s < 4; ++s) xb[u][s] = v[s];
                }
                stage<NT>(cent, img, cb, ndch, dc);
#pragma unroll
                for (int u = 0; u < 2; ++u) mfma_group<NT>(acc, cent, xb[u], u, g, m);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = (cb * NT + t) * 16 + g + 4 * q;
                    if (row_ok && j < k) P[row * (int64_t)k + j] = acc[t][q] / sstd[j];
                }
            }
        }
    }
}

// ---- the pairwise-complete moment pass ----

constexpr int PB = 64;              // columns per block of the pairwise pass: 4 tiles (six accumulator families)

// One accumulator tile: plane `fam` of out (0 N, 1 S, 2 Q, 3 P); the A operand is kind ka (0 k, 1 v, 2 z) of tile ta
// of side sa (0 block A, 1 block B) and gives the result's rows, the B operand (kb, sb, tb) its columns.
struct PwTile {
    int fam, ka, sa, ta, kb, sb, tb;
};

// The tiles of a unit and their deal: tile t belongs to wave t mod 4, which runs all 64 rows of a batch for it.
// Diagonal unit (OFF false, NB = NA): N's upper tiles, P's upper tiles, S's NA^2, Q's NA^2.  Off-diagonal unit
// (NA = 4): the families N_AB, P_AB, S_AB, S_BA, Q_AB, Q_BA of 4 NB tiles each, tile rows of A ascending, then B's.
template <int NA, int NB, bool OFF>
struct PairTiles {
    static constexpr int SA = 16 * NA + 16, SB = 16 * NB + 16;     // LDS row strides (the rule of gram64_mfma.h)
    static constexpr int TU = NA * (NA + 1) / 2;
    static constexpr int T = OFF ? 6 * NA * NB : 2 * TU + 2 * NA * NA;
    static constexpr int MAXT = (T + 3) / 4;

    static constexpr PwTile get(int t) {
        if (OFF) {
            const int f = t / (NA * NB), ta = t % (NA * NB) / NB, tb = t % NB;
            switch (f) {
                case 0: return {0, 0, 0, ta, 0, 1, tb};
                case 1: return {3, 1, 0, ta, 1, 1, tb};
                case 2: return {1, 1, 0, ta, 0, 1, tb};
                case 3: return {1, 1, 1, tb, 0, 0, ta};
                case 4: return {2, 2, 0, ta, 0, 1, tb};
                default: return {2, 2, 1, tb, 0, 0, ta};
            }
        }
        if (t < TU) return {0, 0, 0, tile_a(NA, t), 0, 0, tile_b(NA, t)};
        t -= TU;
        if (t < TU) return {3, 1, 0, tile_a(NA, t), 1, 0, tile_b(NA, t)};
        t -= TU;
        if (t < NA * NA) return {1, 1, 0, t / NA, 0, 0, t % NA};
        t -= NA * NA;
        return {2, 2, 0, t / NA, 0, 0, t % NA};
    }

    // one step of four rows for the wave's slots; o[side][kind][tile] are the lane's operands of the step
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void step(d4_t (&acc)[MAXT], const double (&o)[2][3][4]) {
        if constexpr (s < MAXT) {
            if constexpr (WAVE + 4 * s < T) {
                constexpr PwTile p = get(WAVE + 4 * s);
                acc[s] = mf64(o[p.sa][p.ka][p.ta], o[p.sb][p.kb][p.tb], acc[s]);
            }
            step<WAVE, s + 1>(acc, o);
        }
    }

    // v, z and k of one side's NTS tiles from the staged y (NaN: missing); what the wave's tiles do not use is dropped
    template <int NTS>
    static __device__ __forceinline__ void operands(double (&o)[3][4], const double* __restrict__ yr, int m) {
#pragma unroll
        for (int t = 0; t < NTS; ++t) {
            const double y = yr[16 * t + m];
            const bool miss = y != y;
            const double v = miss ? 0.0 : y;
            o[0][t] = miss ? 0.0 : 1.0;
            o[1][t] = v;
            o[2][t] = v * v;
        }
    }

    // the products of the staged batch for wave WAVE
    template <int WAVE>
    static __device__ __forceinline__ void batch_of(d4_t (&acc)[MAXT], const double* __restrict__ ra,
                                                    const double* __restrict__ rb, int g, int m) {
        for (int r4 = 0; r4 < 16; ++r4) {
            const int row = 4 * r4 + g;
            double o[2][3][4];
            operands<NA>(o[0], ra + row * SA, m);
            if constexpr (OFF) operands<NB>(o[1], rb + row * SB, m);
            step<WAVE>(acc, o);
        }
    }

    // the wave's tiles into the chunk's partial pc [4, d, d]; ca / cb the first columns of the two blocks
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[MAXT], double* __restrict__ pc, int d, int ca,
                                                 int cb, int g, int m) {
        if constexpr (s < MAXT) {
            if constexpr (WAVE + 4 * s < T) {
                constexpr PwTile p = get(WAVE + 4 * s);
                const int col = (p.sb ? cb : ca) + 16 * p.tb + m;
                double* __restrict__ pf = pc + (int64_t)p.fam * d * d;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = (p.sa ? cb : ca) + 16 * p.ta + g + 4 * q;
                    if (row < d && col < d) pf[(int64_t)row * d + col] = acc[s][q];
                }
            }
            store<WAVE, s + 1>(acc, pc, d, ca, cb, g, m);
        }
    }
};

// store_slice with the missing marker: NaN where the row is not `ok` or the column is behind d; a NaN cell stays NaN
// through the shift
template <int NT>
__device__ __forceinline__ void store_slice_nan(double* __restrict__ slot, const d4_t (&v)[NT], bool ok, int c0, int d,
                                                const double* __restrict__ sh, int sub) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int q = 4 * (4 * j + sub);
        d4_t y = shift_group<false>(v[j], ok, c0 + q, d, sh, nullptr, q);
#pragma unroll
        for (int s = 0; s < 4; ++s) y[s] = (ok && c0 + q + s < d) ? y[s] : __builtin_nan("");
        *reinterpret_cast<d4_t*>(slot + q) = y;
    }
}

// The units (chunk, pair) of one launch.  Diagonal (OFF false): pair = block blk0 + p, p < npair, of NA tiles.
// Off-diagonal: A < B with A of 4 tiles and B of NB; last < 0: the pairs of the blocks 0 .. blk0 - 1 in the order A
// ascending, then B (npair = blk0 (blk0 - 1) / 2); else B = last and A = p < npair.
template <int NA, int NB, bool OFF, bool VEC>
__device__ __forceinline__ void pairwise_units(const double* __restrict__ X, int64_t n, int d,
                                               const double* __restrict__ shift, int blk0, int npair, int last,
                                               int64_t chunk_rows, int64_t nchunk, double* __restrict__ part) {
    using D = PairTiles<NA, NB, OFF>;
    __shared__ __attribute__((aligned(32))) double ra[64 * D::SA];
    __shared__ __attribute__((aligned(32))) double rb[OFF ? 64 * D::SB : 4];
    __shared__ __attribute__((aligned(32))) double sh[2 * PB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid >> 2, sub = tid & 3;
    const int m = lane & 15, g = lane >> 4;
    const int64_t P = 4 * (int64_t)d * d;
    for (int64_t u = blockIdx.x; u < nchunk * npair; u += gridDim.x) {
        const int64_t c = u / npair;
        int p = (int)(u - c * npair), A = 0, B;
        if (!OFF) {
            A = B = blk0 + p;
        } else if (last >= 0) {
            A = p;
            B = last;
        } else {
            while (p >= blk0 - 1 - A) {
                p -= blk0 - 1 - A;
                ++A;
            }
            B = A + 1 + p;
        }
        const int ca = A * PB, cb = B * PB;
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        stage_shift(sh, shift, ca, d, NA, tid);         // the previous unit's reads ended at its last barrier
        if (OFF) stage_shift(sh + PB, shift, cb, d, NB, tid - PB);
        __syncthreads();
        d4_t acc[D::MAXT];
#pragma unroll
        for (int s = 0; s < D::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + r;
            const bool ok = i < r1;
            const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)d;
            d4_t va[NA], vb[OFF ? NB : 1];
            load_slice<NA, VEC>(va, xr, ok, ca, d, sub);
            if constexpr (OFF) load_slice<NB, VEC>(vb, xr, ok, cb, d, sub);
            store_slice_nan<NA>(ra + r * D::SA, va, ok, ca, d, sh, sub);
            if constexpr (OFF) store_slice_nan<NB>(rb + r * D::SB, vb, ok, cb, d, sh + PB, sub);
            __syncthreads();
            switch (wave) {
                case 0: D::template batch_of<0>(acc, ra, rb, g, m); break;
                case 1: D::template batch_of<1>(acc, ra, rb, g, m); break;
                case 2: D::template batch_of<2>(acc, ra, rb, g, m); break;
                default: D::template batch_of<3>(acc, ra, rb, g, m); break;
            }
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        switch (wave) {
            case 0: D::template store<0>(acc, pc, d, ca, cb, g, m); break;
            case 1: D::template store<1>(acc, pc, d, ca, cb, g, m); break;
            case 2: D::template store<2>(acc, pc, d, ca, cb, g, m); break;
            default: D::template store<3>(acc, pc, d, ca, cb, g, m); break;
        }
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void pairwise_diag_kernel(const double* __restrict__ X, int64_t n, int d,
                                                            const double* __restrict__ shift, int blk0, int npair,
                                                            int last, int64_t chunk_rows, int64_t nchunk,
                                                            double* __restrict__ part) {
    pairwise_units<NT, NT, false, VEC>(X, n, d, shift, blk0, npair, last, chunk_rows, nchunk, part);
}

template <int NB, bool VEC>
__global__ __launch_bounds__(256) void pairwise_off_kernel(const double* __restrict__ X, int64_t n, int d,
                                                           const double* __restrict__ shift, int blk0, int npair,
                                                           int last, int64_t chunk_rows, int64_t nchunk,
                                                           double* __restrict__ part) {
    pairwise_units<4, NB, true, VEC>(X, n, d, shift, blk0, npair, last, chunk_rows, nchunk, part);
}

// the merge's map for [4, d, d]: the lower triangles of N (plane 0) and P (plane 3) are read from the upper, S and Q
// are left as computed
struct PairwiseMirror {
    int d;
    __device__ int64_t operator()(int64_t e) const {
        const int64_t dd = (int64_t)d * d;
        const int f = (int)(e / dd);
        const int a = (int)((e - f * dd) / d), b = (int)((e - f * dd) - (int64_t)a * d);
        return ((f == 0 || f == 3) && a > b) ? f * dd + (int64_t)b * d + a : e;
    }
};

}  // namespace

extern "C" {

// One moment pass over X [n, d] (1 <= d <= 1024), shift [d] or null: out [d + d d] = [t | C] through
// nchunk = ceil(n / crows) row chunks (crows a multiple of 64) whose partials part [nchunk, d + d d] are merged in
// chunk order.  grid > 0 caps the workgroups of every launch; it changes no bit of the result.
int alink_moments_f64(const double* X, int64_t n, int d, const double* shift, int64_t crows, int64_t nchunk,
                      double* part, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > MOMENTS_DMAX || n >= (1ll << 31)) return 1;
    if (crows < 64 || crows % 64 != 0 || nchunk != (n + crows - 1) / crows) return 1;
    if (X == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = vec_ok(d, X);
    const int nfull = d / MB, ntl = (d % MB + 15) / 16, nblk = nfull + (ntl > 0);
    auto blocks = [&](int64_t units) { return (unsigned)(grid > 0 && grid < units ? grid : units); };
    if (nfull > 0)
        ALINK_D64_LAUNCH_VEC(moments_diag_kernel, 8, vec, blocks(nchunk * nfull), st, X, n, d, shift, 0, nfull, crows,
                             nchunk, part);
    if (ntl > 0)
        ALINK_D64_LAUNCH_NT8(moments_diag_kernel, ntl, vec, blocks(nchunk), st, X, n, d, shift, nfull, 1, crows, nchunk,
                             part);
    if (nblk > 1) {
        const unsigned ob = blocks(nchunk * (nblk * (nblk - 1) / 2));
        if (vec)
            hipLaunchKernelGGL(moments_off_kernel<true>, dim3(ob), dim3(256), 0, st, X, n, d, shift, nblk, crows,
                               nchunk, part);
        else
            hipLaunchKernelGGL(moments_off_kernel<false>, dim3(ob), dim3(256), 0, st, X, n, d, shift, nblk, crows,
                               nchunk, part);
    }
    osum::chunk_merge(osum::GramMirror{d, d}, d + (int64_t)d * d, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// One pairwise-complete moment pass over X [n, d] (1 <= d <= 1024; a NaN cell is missing), shift [d] or null:
// out [4, d, d] = [N | S | Q | P] through nchunk = ceil(n / crows) row chunks (crows a multiple of 64) whose partials
// part [nchunk, 4 d d] are merged in chunk order.  grid > 0 caps the workgroups of every launch; it changes no bit.
int alink_pairwise_moments_f64(const double* X, int64_t n, int d, const double* shift, int64_t crows, int64_t nchunk,
                               double* part, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > MOMENTS_DMAX || n >= (1ll << 31)) return 1;
    if (crows < 64 || crows % 64 != 0 || nchunk != (n + crows - 1) / crows) return 1;
    if (X == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = vec_ok(d, X);
    const int nfull = d / PB, ntl = (d % PB + 15) / 16;
    auto blocks = [&](int64_t units) { return (unsigned)(grid > 0 && grid < units ? grid : units); };
    if (nfull > 0)
        ALINK_D64_LAUNCH_VEC(pairwise_diag_kernel, 4, vec, blocks(nchunk * nfull), st, X, n, d, shift, 0, nfull, -1,
                             crows, nchunk, part);
    if (ntl > 0)
        ALINK_D64_LAUNCH(pairwise_diag_kernel, ntl, 1, 2, 3, 4, vec, blocks(nchunk), st, X, n, d, shift, nfull, 1, -1,
                         crows, nchunk, part);
    if (nfull > 1) {
        const int npair = nfull * (nfull - 1) / 2;
        ALINK_D64_LAUNCH_VEC(pairwise_off_kernel, 4, vec, blocks(nchunk * npair), st, X, n, d, shift, nfull, npair, -1,
                             crows, nchunk, part);
    }
    if (nfull > 0 && ntl > 0)
        ALINK_D64_LAUNCH(pairwise_off_kernel, ntl, 1, 2, 3, 4, vec, blocks(nchunk * nfull), st, X, n, d, shift, nfull,
                         nfull, nfull, crows, nchunk, part);
    osum::chunk_merge(PairwiseMirror{d}, 4 * (int64_t)d * d, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// P [n, k] = ((X - mean) / scale) T^T / sstd for X [n, nx] (1 <= nx <= 1024), mean / scale [nx], sstd [k]; img: the
// image of T [k, nx] by ``ops/kmeans_dense64.centroid_image`` (its tiles-per-block and block count follow from k).
int alink_pca_project_f64(const double* X, int64_t n, int nx, const double* mean, const double* scale,
                          const double* img, int k, const double* sstd, double* P, int grid, void* stream) {
    if (n <= 0) return 0;
    if (nx < 1 || nx > MOMENTS_DMAX || k < 1 || n >= (1ll << 31)) return 1;
    int nt = 1;         // ``tiles(k)``: the power of two that covers k, at most 8
    while (nt < 8 && 16 * nt < k) nt *= 2;
    const int nblk = (k + 16 * nt - 1) / (16 * nt);
    if (X == nullptr || mean == nullptr || scale == nullptr || img == nullptr || sstd == nullptr || P == nullptr)
        return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (nx + DCH - 1) / DCH;
    ALINK_D64_LAUNCH(pca_project_kernel, nt, 1, 2, 4, 8, vec_ok(nx, X), row_blocks(n, grid, 4096), st, X, n, nx, mean,
                     scale, img, k, nblk, ndch, sstd, P);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
